"""tests/body_layout_model.py against brute force, and the steered calls of
tests/test_gpu_body_edges.py against what they are there to reach -- at the
wave counts of three parts (8 waves per compute unit: 64, 256 and 304 units), so
that the GPU tests do not lose a case silently on another device."""
import pytest

from oracle import oracle as O
from tests import body_layout_model as M

WAVES = (512, 2048, 2432)


def test_geometry_brute_force():
    nch, filled = 0, 0  # chunks opened so far, bytes in the last one
    for mlen in range(33, 70001):
        if filled == M.CHUNK or nch == 0:
            nch, filled = nch + 1, 0
        filled += 1  # body byte mlen - 33 goes to the last chunk
        if mlen < M.BODY_MIN_MLEN:
            continue
        blocks = len(range(0, filled, 16))
        assert M.geometry(mlen) == (nch, blocks, filled), mlen
        assert M.mlen_of(nch, filled) == mlen
    assert M.geometry(M.BODY_MIN_MLEN)[0] == 36
    assert [m for m in range(M.BODY_MIN_MLEN, 70001) if M.geometry(m)[0] == 36] == list(range(4577, 4641))
    assert M.geometry(32) == M.geometry(0) == (1, 0, 0)


def test_mlen_is_wire_size_minus_32():
    # (the test frames carry flags 0-3 on sessions without the SUBSCRIBE downgrade: a one-byte header)
    for flags in range(4):
        for P in (4575, 4576, 4639, 65536):
            assert O.wire_size(flags, 0, P) - 32 == P + 1
    assert all(M.mlen_of(36, b) >= M.BODY_MIN_MLEN for b in M.LASTB_36)
    assert M.mlen_of(36, 64) < M.BODY_MIN_MLEN  # (a shorter last chunk stays with the frame kernel)


def test_runs_partition_the_tiles():
    for NW in WAVES:
        for total in (1, 64, 65, 64 * NW - 1, 64 * NW, 64 * NW + 1, 160 * NW + 7):
            r = M.runs(total, NW)
            tiles = (total + 63) // 64
            assert r[0][0] == 0 and r[-1][1] == tiles
            assert all(a[1] == b[0] for a, b in zip(r, r[1:]))
            assert max(e - b for b, e in r) - min(e - b for b, e in r) <= 1


def _brute_classify(c, N, NW):
    """The same classes lane by lane, as k_body's finish sees a tile."""
    total = c * N
    got = {k: 0 for k in M.CLASSES}
    frame_waves = [set() for _ in range(N)]
    frame_tiles = [set() for _ in range(N)]
    for W, (tb, te) in enumerate(M.runs(total, NW)):
        got["runs_of_%d" % min(te - tb, 3)] += 1
        carry_key = None
        for t in range(tb, te):
            key = [(64 * t + l) // c if 64 * t + l < total else None for l in range(64)]
            ch = [(64 * t + l) % c for l in range(64)]
            for l in range(64):
                if key[l] is not None:
                    frame_waves[key[l]].add(W)
                    frame_tiles[key[l]].add(t)
            uniform = key[0] is not None and all(k == key[0] for k in key)
            cin = carry_key is not None and key[0] == carry_key
            firsts = [l for l in range(64) if key[l] is not None and (l == 0 or key[l - 1] != key[l])]
            ends = {f: max(l for l in range(64) if key[l] == key[f]) for f in firsts}
            lf = firsts[-1]
            open_ = ch[ends[lf]] + 1 < c
            powtab = open_ and c - 2 - ch[ends[lf]] >= 64
            last = t + 1 == te
            if uniform:
                got["uniform_carry_in"] += cin
                got["uniform_carry_out"] += open_ and not last
                got["uniform_open_at_run_end"] += open_ and last
                got["uniform_open_at_run_end_powtab"] += powtab and last
                got["uniform_ends_frame"] += not open_
            else:
                got["mixed_2_segments"] += len(firsts) == 2
                got["mixed_3_segments"] += len(firsts) == 3
                got["mixed_carry_in"] += cin
                got["partial_last_tile"] += key[63] is None
                got["mixed_open_carry_out"] += open_ and not last
                got["mixed_open_at_run_end"] += open_ and last
                got["mixed_open_at_run_end_powtab"] += powtab and last
                got["one_chunk_at_lane_0"] += len(firsts) > 1 and ends[0] == 0
                got["one_chunk_at_lane_63"] += key[63] is not None and key[62] != key[63]
            edge = key[63] is not None and ch[63] + 1 == c
            got["frame_end_on_tile_edge"] += edge
            got["frame_end_on_tile_edge_in_run"] += edge and not last
            carry_key = key[lf] if open_ else None
    for i in range(N):
        w = len(frame_waves[i])
        got["frames_in_%s" % ("1_wave", "2_waves", "3_or_more_waves")[min(w, 3) - 1]] += 1
        got["frames_in_1_wave_over_tiles"] += w == 1 and len(frame_tiles[i]) > 1
    got["open_at_run_end_powtab"] = got["uniform_open_at_run_end_powtab"] + got["mixed_open_at_run_end_powtab"]
    return got


@pytest.mark.parametrize("c,N,NW", [(36, 40, 8), (37, 100, 16), (63, 33, 4), (64, 20, 8), (65, 130, 16), (100, 77, 16),
                                    (128, 9, 4), (192, 50, 8), (500, 3, 8), (129, 1, 2), (36, 1, 512)])
def test_classify_brute_force(c, N, NW):
    assert dict(M.classify(c, N, NW)) == _brute_classify(c, N, NW)


@pytest.mark.parametrize("NW", WAVES)
def test_alignment_calls_reach_their_cases(NW):
    for c in (37, 36):
        k = M.classify(c, M.ALIGN_FRAMES, NW)
        assert k["mixed_2_segments"] and k["mixed_3_segments"], (c, M.reached(k))
    # the merged short tail: chunk alignment d (the same for every chunk of a
    # frame: chunks are 8 granules) and a last chunk of b bytes with d + b < 16
    want = {(d, b) for d in range(16) for b in M.LASTB if d + b < 16}
    assert len(want) == 15 + 14 + 1
    assert len(M.LASTB) == len(M.LASTB_36) == 10 and min(M.LASTB_36) == 65 and max(M.LASTB_36) == 128


@pytest.mark.parametrize("NW", WAVES)
def test_small_calls_reach_their_cases(NW):
    ks = {c: M.classify(c, M.small_frames(c), NW) for c in M.SMALL_C}
    for c, k in ks.items():
        assert k["runs_of_2"] == k["runs_of_3"] == 0 and k["runs_of_1"], c  # every wave has at most one tile
    for cls, cs in M.SMALL_MUST.items():
        for c in cs:
            assert ks[c][cls] > 0, (cls, c, M.reached(ks[c]))


@pytest.mark.parametrize("shrunk", [False, True])
@pytest.mark.parametrize("NW", WAVES)
def test_large_calls_reach_their_cases(NW, shrunk):
    must = M.LARGE_MUST_SHRUNK if shrunk else M.LARGE_MUST
    assert set(must) == set(M.LARGE_C)
    for c in M.LARGE_C:
        k = M.classify(c, M.large_frames(c, NW, shrunk), NW)
        for cls in must[c]:
            assert k[cls] > 0, (c, cls, M.reached(k))
        assert k["runs_of_0"] == 0
    union = set().union(*must.values())
    for cls in ("uniform_carry_in", "uniform_carry_out", "mixed_carry_in", "mixed_open_carry_out",
                "frames_in_1_wave_over_tiles", "one_chunk_at_lane_0", "one_chunk_at_lane_63"):
        assert cls in union


@pytest.mark.parametrize("NW", WAVES)
def test_one_frame_calls_reach_their_cases(NW):
    nchs = M.one_frame_chunks()
    assert len(nchs) == 27 and nchs[:3] == [63, 64, 65] and nchs[-1] == (1 << 14) + 1
    # head_powers writes powtab from 65 chunks on (nch - 1 >= 64); a run's end
    # reads it while 64 or more chunks follow
    assert sum(M.classify(n, 1, NW)["open_at_run_end_powtab"] > 0 for n in nchs) >= 20
    k = M.classify(M.two_tile_chunks(NW), 1, NW)
    assert k["runs_of_2"] == 1 and k["uniform_carry_out"] == 1 and k["mixed_carry_in"] == 1, M.reached(k)
    assert k["partial_last_tile"] == 1 and k["open_at_run_end_powtab"] > 0
    assert M.two_tile_chunks(2048) == (1 << 17) + 1


def test_post_segments():
    S = M.post_segments
    assert S(1) == (65536, 1, 1) and S(65536) == (65536, 1, 65536) and S(65537) == (65536, 2, 1)
    assert S(786432) == (65536, 12, 65536) and S(786433) == (69632, 12, 786433 - 11 * 69632)
    assert S(12 * 69632) == (69632, 12, 69632) and S(12 * 69632 + 1) == (73728, 12, 12 * 69632 + 1 - 11 * 73728)
    for L in list(range(1, 300000, 997)) + [1 << 24, (1 << 24) + 1, (1 << 30) + 12345]:
        seg, nseg, last = S(L)
        assert seg % 4096 == 0 and seg >= 65536 and 0 < last <= seg and (nseg - 1) * seg + last == L
        assert nseg <= 12 or seg == 65536
    segs = {L: S(L) for L in M.SEAM_LENGTHS}
    last = lambda L: segs[L][2]
    many = [L for L in segs if segs[L][1] > 1]
    assert any(segs[L][1] == 1 for L in segs)                      # one segment
    assert any(last(L) < 33 for L in many)                         # ns = b - a < 33, a + k < len
    assert any(last(L) == 33 for L in many)
    assert any(last(L) > 33 for L in many)
    assert any(segs[L][0] > 65536 for L in segs)                   # len / 12 rounded up to 4 KiB
    assert any(last(L) % 4096 not in (0,) and last(L) > 4096 for L in many)  # a partial last 4 KiB round
    assert any(last(L) % 4096 == 0 for L in many)                  # and none
    assert 10e6 < 2 * sum(M.SEAM_LENGTHS) < 13e6
