"""The chunked body path (the frame kernel's heads, k_body, k_post) steered to
its tile, run and seam edges; tests/body_layout_model.py says which of them a
call reaches, the CPU oracle says what the bytes must be.

The layout of a call depends on the order in which its big frames arrive at
the list's atomic, so a call with mixed chunk counts runs a different layout
each time and no test can say what it reached.  A call whose big frames all
have the SAME chunk count c is repeatable (chunk_end is c, 2c, ... whatever the
order), and so is a call with one big frame: every case that asserts a class
uses one chunk count per call.  The two calls that mix chunk counts (the
one-frame lengths together, the k_post lengths together) assert bytes only.

Every call goes through the same harness:
* encode on the device; the WHOLE output buffer (0xEE-filled, gaps of 0-31
  bytes between frames, 256 after the last) equals the oracle's wire with
  every byte outside a frame still 0xEE;
* decode of the oracle's wire out of place, the payload buffer held to the
  same rule; then in place at out_off = in_off + 33 and at out_off = in_off;
* status, flags, payloads and peer nonces equal the oracle's sequential decode;
* one frame's MAC is broken and one frame replays a nonce: their regions are
  zero-filled, their neighbours intact.
Frame k's payload starts at k mod 16 (mod 16) and its wire at (k div 16) mod 16,
and its last body chunk holds lastb bytes in rotation, so that 2,560 frames are
every (payload, wire, lastb) triple once.

Out of scope here: the Poly1305 reduction edges of this path
(test_gpu_poly_edges.py::test_body_kernel), VERIFY_FIRST / REPLAY_HOST on big
frames (test_gpu_verify_first.py), the ZMTP, WebSocket and forward entries."""
import time
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle as O
from tests import body_layout_model as M
from tests.test_gpu_configs import _host_threads
from tests.test_gpu_parity import dev, host

pytestmark = pytest.mark.gpu

SENT = 0xEE
SESSIONS = 12  # a call uses three of them (sid_base ..+2)
KEYS = [np.random.default_rng(20261101 + s).integers(0, 256, 32, dtype=np.uint8).tobytes() for s in range(SESSIONS)]
ERR_CRYPTOGRAPHIC, ERR_INVALID_SEQUENCE = 0x11000001, 0x10000002  # (checked against the library's in contexts())


# ---------------------------------------------------------------- batches
def _offsets(lengths, mod16, extra16):
    """Frame i at the next position that is mod16[i] (mod 16), plus 16 where
    extra16[i]: gaps of 0-31 bytes; returns (offsets, buffer size)."""
    off = np.zeros(len(lengths), np.uint64)
    pos = 0
    for i, (ln, m, e) in enumerate(zip(lengths.tolist(), mod16.tolist(), extra16.tolist())):
        pos += (m - pos) % 16 + 16 * e
        off[i] = pos
        pos += ln
    return off, pos + 256


def _mask(off, ln, size):
    """True on the bytes of the regions [off[i], off[i] + ln[i])."""
    d = np.zeros(size + 1, np.int8)
    np.add.at(d, off.astype(np.int64), 1)
    np.add.at(d, off.astype(np.int64) + ln.astype(np.int64), -1)
    return np.cumsum(d[:-1], dtype=np.int8) > 0


def _slices(n, nbytes):
    nt = max(1, min(_host_threads(), n, nbytes >> 19))
    cuts = np.linspace(0, n, nt + 1).astype(np.int64)
    return [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def rotation(k, lastbs):
    """Frame k's (payload offset mod 16, wire offset mod 16, lastb)."""
    a, b = k % 16, (k // 16) % 16
    return a, b, lastbs[(k // 256 + a + b) % len(lastbs)]


def uniform_lengths(c, n, k0=0):
    """Payload lengths of n frames of c body chunks each, lastb in rotation."""
    return [M.mlen_of(c, rotation(k0 + i, M.lastb_set(c))[2]) - 1 for i in range(n)]


def make_batch(P, seed, k0=0, sid_base=0, mac_fail=None, replay=None, tag_only=False):
    """Frames of payload lengths P (frame i counts as frame k0 + i of the
    rotation) with their buffers, and the oracle's encode and sequential
    decode of them, run in slices on the host's cores."""
    t0 = time.perf_counter()
    b = SimpleNamespace()
    P = np.asarray(P, np.int64)
    n = b.n = len(P)
    k = k0 + np.arange(n)
    b.mac_fail = ([n // 3] if n >= 12 else []) if mac_fail is None else list(mac_fail)
    b.replay = ([n // 2 + 3] if n >= 12 else []) if replay is None else list(replay)
    assert not set(b.mac_fail) & set(b.replay)
    b.P = P
    b.sid = (sid_base + k % 3).astype(np.uint32)
    b.nonce = (3 + np.arange(n)).astype(np.uint64)
    for j in b.replay:
        b.nonce[j] = b.nonce[j - 3]  # the same session's frame before it
    b.flags = ((k // 5) % 4).astype(np.uint8)
    extra = (k * 7 + k // 3) % 2
    b.poff, b.psize = _offsets(P, k % 16, extra)
    b.wl = (P + 33).astype(np.uint32)
    b.woff, b.wsize = _offsets(P + 33, (k // 16) % 16, 1 - extra)
    for f, p, w in zip(b.flags[:4], P[:4], b.wl[:4]):
        assert O.wire_size(int(f), 0, int(p)) == int(w)
    b.inp = np.random.default_rng(seed).integers(0, 256, b.psize, dtype=np.uint8)
    b.pmask, b.wmask = _mask(b.poff, P, b.psize), _mask(b.woff, b.wl, b.wsize)
    pend, wend = b.poff + P.astype(np.uint64), b.woff + b.wl.astype(np.uint64)
    sl = _slices(n, int(P.sum()))
    esess = O.make_sessions(KEYS)
    dsess = O.make_sessions(KEYS, dec_prefix=O.CLIENT_PREFIX)

    def enc(a, z):
        pl, ph, wlo, whi = int(b.poff[a]), int(pend[z - 1]), int(b.woff[a]), int(wend[z - 1])
        return O.encode_batch(esess, b.sid[a:z], b.nonce[a:z], b.flags[a:z], b.poff[a:z] - np.uint64(pl),
                              b.wl[a:z] - 33, b.inp[pl:max(ph, pl + 1)], b.woff[a:z] - np.uint64(wlo), whi - wlo)

    def dec(a, z):
        pl, ph, wlo, whi = int(b.poff[a]), int(pend[z - 1]), int(b.woff[a]), int(wend[z - 1])
        peer = np.full(SESSIONS, 2, np.uint64)  # what a sequential decode holds before frame a
        for s in range(SESSIONS):
            peer[s] = max(2, int(b.nonce[:a][b.sid[:a] == s].max(initial=2)))
        out, fl, st = O.decode_batch(dsess, peer, b.sid[a:z], b.woff[a:z] - np.uint64(wlo), b.wl[a:z],
                                     b.wire_in[wlo:whi], b.poff[a:z] - np.uint64(pl), ph - pl)
        return out, fl, st, peer

    with ThreadPoolExecutor(len(sl)) as ex:
        wire = np.zeros(b.wsize, np.uint8)
        for (a, z), w in zip(sl, ex.map(lambda s: enc(*s), sl)):
            wire[int(b.woff[a]):int(wend[z - 1])] = w
        b.wire = np.where(b.wmask, wire, np.uint8(SENT))       # what encode must leave
        b.wire_in = b.wire.copy()                              # what decode is given
        for j in b.mac_fail:                                   # a tag byte, or the last ciphertext byte
            b.wire_in[int(b.woff[j]) + (16 + j % 16 if tag_only or j % 2 == 0 else int(b.wl[j]) - 1)] ^= 0x10
        pay = np.zeros(b.psize, np.uint8)
        b.st, b.fl = np.zeros(n, np.int32), np.zeros(n, np.uint8)
        b.peer = np.full(SESSIONS, 2, np.uint64)
        for (a, z), (out, fl, st, peer) in zip(sl, ex.map(lambda s: dec(*s), sl)):
            pay[int(b.poff[a]):int(pend[z - 1])] = out
            b.fl[a:z], b.st[a:z] = fl, st
            b.peer = np.maximum(b.peer, peer)
        b.pay = np.where(b.pmask, pay, np.uint8(SENT))         # what decode must leave
    failed = np.flatnonzero(b.st != 0).tolist()
    assert failed == sorted(b.mac_fail + b.replay), (failed, b.mac_fail, b.replay)
    assert all(b.st[j] == ERR_CRYPTOGRAPHIC for j in b.mac_fail)
    assert all(b.st[j] == ERR_INVALID_SEQUENCE for j in b.replay)
    for j in failed:
        assert not b.pay[int(b.poff[j]):int(pend[j])].any()
    ok = b.pmask.copy()
    for j in failed:
        ok[int(b.poff[j]):int(pend[j])] = False
    assert np.array_equal(b.pay[ok], b.inp[ok])  # (the oracle's round trip, before the device is asked)
    b.t_oracle = time.perf_counter() - t0
    return b


# ---------------------------------------------------------------- the harness
def contexts(C):
    assert (C.ERR_CRYPTOGRAPHIC, C.ERR_INVALID_SEQUENCE) == (ERR_CRYPTOGRAPHIC, ERR_INVALID_SEQUENCE)
    enc, dec = C.CurveContext(0, SESSIONS), C.CurveContext(0, SESSIONS)
    for s, key in enumerate(KEYS):
        enc.session_set(s, key, O.CLIENT_PREFIX, O.SERVER_PREFIX)
        dec.session_set(s, key, O.SERVER_PREFIX, O.CLIENT_PREFIX, False, 2)
    return enc, dec


def _same(got, want, off, b, what):
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    fr = np.searchsorted(off, bad, side="right") - 1
    i, x = int(fr[0]), int(bad[0])
    nch, _, lastb = M.geometry(int(b.P[max(i, 0)]) + 1)
    raise AssertionError(f"{what}: {bad.size} bytes differ, the first at buffer byte {x} = frame {i} byte "
                         f"{x - int(off[max(i, 0)])} (got {int(got[x]):#x}, want {int(want[x]):#x}; the frame: {nch} "
                         f"chunks, {lastb} bytes in the last, payload at {int(b.poff[max(i, 0)]) % 16} and wire at "
                         f"{int(b.woff[max(i, 0)]) % 16} mod 16); frames {np.unique(fr)[:12].tolist()}")


def start_encode(torch, enc, b):
    out = torch.full((b.wsize,), SENT, dtype=torch.uint8, device="cuda")
    args = [dev(torch, x) for x in (b.sid, b.nonce, b.flags, b.poff, (b.wl - 33).astype(np.uint32), b.inp, b.woff)]
    return lambda: enc.encode_batch(*args, out), out


def check_encode(b, out, what):
    _same(host(out, np.uint8), b.wire, b.woff, b, what + " encode")


def start_decode(torch, dec, b, layout=None):
    """layout None: out of place; 33 / 0: in place at out_off = in_off + layout."""
    fl = torch.full((b.n,), SENT, dtype=torch.uint8, device="cuda")
    st = torch.full((b.n,), -1, dtype=torch.int32, device="cuda")
    buf = dev(torch, b.wire_in)
    if layout is None:
        out, ooff = torch.full((b.psize,), SENT, dtype=torch.uint8, device="cuda"), b.poff
    else:
        out, ooff = buf, b.woff + np.uint64(layout)
    args = [dev(torch, x) for x in (b.sid, b.woff, b.wl)] + [buf, dev(torch, ooff), out, fl, st]
    return lambda: dec.decode_batch(*args), (out, fl, st)


def check_decode(b, res, dec, what, layout=None):
    out, fl, st = res
    what = f"{what} decode {'out of place' if layout is None else 'in place +%d' % layout}"
    gst, gfl = host(st, np.int32), host(fl, np.uint8)
    assert np.array_equal(gst, b.st), (what, [(int(i), hex(int(gst[i]) & 0xffffffff), hex(int(b.st[i]) & 0xffffffff))
                                              for i in np.flatnonzero(gst != b.st)[:8]])
    assert np.array_equal(gfl, b.fl), (what, np.flatnonzero(gfl != b.fl)[:8].tolist())
    got = host(out, np.uint8)
    if layout is None:
        _same(got, b.pay, b.poff, b, what)
    else:
        assert (got[~b.wmask] == SENT).all(), (what, "a byte outside every frame was written",
                                               np.flatnonzero(~b.wmask & (got != SENT))[:8].tolist())
        at = b.woff + np.uint64(layout)
        g, w = got[_mask(at, b.P, b.wsize)], b.pay[b.pmask]  # the payload regions, back to back in frame order
        if not np.array_equal(g, w):
            x = int(np.flatnonzero(g != w)[0])
            i = int(np.searchsorted(np.cumsum(b.P), x, side="right"))
            raise AssertionError(f"{what}: {int((g != w).sum())} payload bytes differ, the first in frame {i} "
                                 f"({int(b.P[i])} bytes) at {x - int(b.P[:i].sum())}")
        for j in np.flatnonzero(b.st != 0).tolist():
            # no plaintext of a failed frame beside its (zero-filled) payload region either
            a, z = int(b.woff[j]), int(b.woff[j]) + int(b.wl[j])
            rest = (a + int(b.P[j]), z) if layout == 0 else (a, a + 33)
            assert not got[rest[0]:rest[1]].any() or np.array_equal(got[rest[0]:rest[1]], b.wire_in[rest[0]:rest[1]]), j
    if dec is not None:
        for s in np.unique(b.sid).tolist():
            assert dec.get_peer_nonce(s) == int(b.peer[s]), (what, s)


def run_case(torch, enc, dec, b, what, layouts=(None, 33, 0), encode=True):
    """The whole harness on one batch; returns the device-side seconds."""
    t0 = time.perf_counter()
    if encode:
        go, out = start_encode(torch, enc, b)
        go()
        torch.cuda.synchronize()
        check_encode(b, out, what)
    for layout in layouts:
        for s in np.unique(b.sid).tolist():
            dec.set_peer_nonce(s, 2)
        go, res = start_decode(torch, dec, b, layout)
        go()
        torch.cuda.synchronize()
        check_decode(b, res, dec, what, layout)
    return time.perf_counter() - t0


def waves(torch):
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count


def chunk_alignments(b):
    """Per frame: lastb, and its body chunks' output alignment on encode (wire
    byte 64 + 128 c) and on out-of-place decode (payload byte 31 + 128 c)."""
    lastb = np.array([M.geometry(int(p) + 1)[2] for p in b.P])
    return lastb, b.woff.astype(np.int64) % 16, (b.poff.astype(np.int64) + 31) % 16


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("c", [37, 36])
def test_alignment_grid(torch_cuda, C, c):
    """Input alignment x output alignment x bytes of the last chunk, all 2,560
    triples, c chunks per frame: the edge-granule merge (cont, prevcont, the
    short tail that ends inside the granule it shares with the chunk before)."""
    torch = torch_cuda
    NW = waves(torch)
    n = M.ALIGN_FRAMES
    k = M.classify(c, n, NW)
    assert k["mixed_2_segments"] and k["mixed_3_segments"], M.reached(k)
    b = make_batch(uniform_lengths(c, n), 1000 + c)
    assert all(M.geometry(int(p) + 1)[0] == c for p in b.P)
    lastb, d_enc, d_dec = chunk_alignments(b)
    trip = set(zip((b.poff % 16).tolist(), (b.woff % 16).tolist(), lastb.tolist()))
    assert len(trip) == n and set(lastb.tolist()) == set(M.lastb_set(c))
    merged = {(d, x) for d in range(16) for x in M.lastb_set(c) if d + x < 16}
    assert merged <= set(zip(d_enc.tolist(), lastb.tolist())) and merged <= set(zip(d_dec.tolist(), lastb.tolist()))
    assert len(merged) == (30 if c == 37 else 0)  # (36 chunks: the last one holds 65 bytes or more)
    t = run_case(torch, *contexts(C), b, f"c = {c}")
    print(f"alignment grid, c = {c}: {n} frames, {int(b.P.sum()) >> 20} MiB, {len(merged)} merged short tails each "
          f"way; {M.reached(k)}; oracle {b.t_oracle:.2f} s, device and checks {t:.2f} s")


# ---------------------------------------------------------------- B
@pytest.mark.parametrize("c", M.SMALL_C)
def test_small_calls(torch_cuda, C, c):
    """About 300 tiles: every wave has at most one tile, so every open segment
    is moved to its frame's end by frame_after_power and combined by atomics."""
    torch = torch_cuda
    NW = waves(torch)
    n = M.small_frames(c)
    k = M.classify(c, n, NW)
    assert k["runs_of_2"] == k["runs_of_3"] == 0
    for cls, cs in M.SMALL_MUST.items():
        assert c not in cs or k[cls] > 0, (cls, M.reached(k))
    b = make_batch(uniform_lengths(c, n), 2000 + c)
    t = run_case(torch, *contexts(C), b, f"small call, c = {c}")
    print(f"small call, c = {c}: {n} frames; {M.reached(k)}; oracle {b.t_oracle:.2f} s, device and checks {t:.2f} s")


# ---------------------------------------------------------------- C
LARGE_SHRUNK = ()        # chunk counts run at 3 NW / 2 + 1 tiles (runs of 1 and 2) to stay within a few seconds
LARGE_ONE_DECODE = ()    # chunk counts whose in-place re-decodes are left out for the same reason


@pytest.mark.parametrize("c", M.LARGE_C)
def test_large_calls(torch_cuda, C, c):
    """5 NW / 2 + 1 tiles: every wave walks 2 or 3 tiles, so frames are carried
    from tile to tile (cfe, carry_key, carry_cnt), whole frames live inside one
    wave, and the LDS double buffer turns over with frame boundaries in it."""
    torch = torch_cuda
    NW = waves(torch)
    shrunk = c in LARGE_SHRUNK
    n = M.large_frames(c, NW, shrunk)
    k = M.classify(c, n, NW)
    for cls in (M.LARGE_MUST_SHRUNK if shrunk else M.LARGE_MUST)[c]:
        assert k[cls] > 0, (cls, M.reached(k))
    b = make_batch(uniform_lengths(c, n), 3000 + c)
    t = run_case(torch, *contexts(C), b, f"large call, c = {c}",
                 layouts=(None,) if c in LARGE_ONE_DECODE else (None, 33, 0))
    print(f"large call, c = {c}: {n} frames, {int(b.P.sum()) >> 20} MiB; {M.reached(k)}; oracle {b.t_oracle:.2f} s, "
          f"device and checks {t:.2f} s")


# ---------------------------------------------------------------- D
def test_one_frame_powers(torch_cuda, C):
    """One frame of 2^k - 1, 2^k, 2^k + 1 chunks per call, k = 6 .. 14: the
    power table's switch from the frame record to powtab (head_powers from 65
    chunks on, frame_after_power at every run's end with 64 or more chunks to
    go).  Then all of them in one call, whose layout depends on arrival order."""
    torch = torch_cuda
    NW = waves(torch)
    enc, dec = contexts(C)
    nchs = M.one_frame_chunks()
    lens, t, tor, pt = [], 0.0, 0.0, 0
    for i, nch in enumerate(nchs):
        k = M.classify(nch, 1, NW)
        pt += k["open_at_run_end_powtab"]
        lens.append(M.mlen_of(nch, (1, 16, 128)[i % 3]) - 1)
        b = make_batch([lens[-1]], 4000 + i, k0=17 * i + 3)
        assert M.geometry(int(b.P[0]) + 1)[0] == nch
        t += run_case(torch, enc, dec, b, f"one frame of {nch} chunks", layouts=(None,))
        tor += b.t_oracle
    assert pt > 0
    b = make_batch(lens, 4100)
    t += run_case(torch, enc, dec, b, "the one-frame lengths in one call", layouts=(None,))
    print(f"one frame per call: {len(nchs)} calls of {nchs[0]} .. {nchs[-1]} chunks, {pt} run ends reading powtab, "
          f"then one call of all {len(nchs)}; oracle {tor + b.t_oracle:.2f} s, device and checks {t:.2f} s")


def test_one_frame_two_tiles(torch_cuda, C):
    """One frame of NW + 1 tiles (2^17 + 1 chunks on an MI355X): the last wave
    carries a uniform tile into a tile of one chunk, every other wave's tile is
    moved over up to 2^17 chunks by powtab."""
    torch = torch_cuda
    NW = waves(torch)
    nch = M.two_tile_chunks(NW)
    k = M.classify(nch, 1, NW)
    assert k["runs_of_2"] == 1 and k["uniform_carry_out"] == 1 and k["mixed_carry_in"] == 1, M.reached(k)
    b = make_batch([M.mlen_of(nch, 16) - 1], 4200, k0=0x5b)
    t = run_case(torch, *contexts(C), b, f"one frame of {nch} chunks", layouts=(None,))
    print(f"one frame of {nch} chunks: {M.reached(k)}; oracle {b.t_oracle:.2f} s, device and checks {t:.2f} s")


# ---------------------------------------------------------------- E
def test_post_seams(torch_cuda, C):
    """In-place decode at out_off = in_off: k_post moves each payload down by 33
    bytes in segments, a 33-byte seam per segment kept aside.  Every length
    once genuine and once with a broken MAC, all in one call (the post list has
    32 entries, segment j of entry e on workgroup (j + e) mod G), then each
    genuine one alone.  A broken frame's whole wire region is zero-filled or
    left as it was beyond the payload region, and the 0xEE around it stays."""
    torch = torch_cuda
    segs = {L: M.post_segments(L) for L in M.SEAM_LENGTHS}
    many = [L for L in segs if segs[L][1] > 1]
    cases = {"one segment": sum(segs[L][1] == 1 for L in segs),
             "last segment < 33": sum(segs[L][2] < 33 for L in many),
             "last segment = 33": sum(segs[L][2] == 33 for L in many),
             "last segment > 33": sum(segs[L][2] > 33 for L in many),
             "segment > 64 KiB": sum(segs[L][0] > 65536 for L in segs),
             "partial last 4 KiB round": sum(segs[L][2] > 4096 and segs[L][2] % 4096 != 0 for L in many)}
    assert all(cases.values()), cases
    enc, dec = contexts(C)
    P = [L for L in M.SEAM_LENGTHS for _ in (0, 1)]
    b = make_batch(P, 5000, mac_fail=range(1, len(P), 2), replay=[], tag_only=True)
    t = run_case(torch, enc, dec, b, "k_post seams, one call", layouts=(0,), encode=False)
    tor = b.t_oracle
    for i, L in enumerate(M.SEAM_LENGTHS):
        one = make_batch([L], 5100 + i, k0=37 * i + 5)
        t += run_case(torch, enc, dec, one, f"k_post seams, {L} bytes alone", layouts=(0,), encode=False)
        tor += one.t_oracle
    print(f"k_post seams: {len(P)} frames in one call, {len(M.SEAM_LENGTHS)} alone, {sum(P) >> 20} MiB; "
          + ", ".join(f"{k}: {v}" for k, v in cases.items()) + f"; oracle {tor:.2f} s, device and checks {t:.2f} s")


# ---------------------------------------------------------------- F
def test_call_state(torch_cuda, C):
    """Four calls back to back on one context and one stream with no
    synchronisation between them: the list counter alternates by epoch parity,
    and k_body returns early when a call has no big frame."""
    torch = torch_cuda
    small = np.random.default_rng(6).choice([0, 1, 31, 32, 33, 200, 1024, 4000, 4574, 4575], 200)
    assert max(small) + 1 < M.BODY_MIN_MLEN
    batches = [make_batch(uniform_lengths(65, M.small_frames(65)), 6001, sid_base=0),
               make_batch(small, 6002, sid_base=3),
               make_batch(uniform_lengths(36, M.small_frames(36)), 6003, sid_base=6),
               make_batch([M.mlen_of(129, 17) - 1], 6004, sid_base=9, k0=0x2c)]
    enc, dec = contexts(C)
    t0 = time.perf_counter()
    encs = [start_encode(torch, enc, b) for b in batches]
    decs = [start_decode(torch, dec, b) for b in batches]
    torch.cuda.synchronize()  # (the uploads; nothing waits from here to the end of the eight calls)
    for go, _ in encs:
        go()
    for go, _ in decs:
        go()
    torch.cuda.synchronize()
    for i, (b, (_, out), (_, res)) in enumerate(zip(batches, encs, decs)):
        check_encode(b, out, f"call {i}")
        check_decode(b, res, dec, f"call {i}")
    print(f"call state: 4 encodes and 4 decodes queued back to back ({', '.join(str(b.n) for b in batches)} frames; "
          f"the second has no big frame); oracle {sum(b.t_oracle for b in batches):.2f} s, device and checks "
          f"{time.perf_counter() - t0:.2f} s")
