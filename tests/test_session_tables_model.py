"""The steered batches of tests/session_tables_steer.py against the oracle and
the plain model of the session tables (tests/session_tables_model.py), with no
GPU.  Per batch: the oracle alone gives the status every frame was built for
(`want`), each steered pair lands at the seam its name says (locate), and the
model, fed the header-valid nonces the oracle's statuses imply, gives the
oracle's replay verdicts, peer nonces and session maxima (for the encode
cases: the sequential counters).  Per seam: a named mutation of the model must
make a batch of its class disagree with the oracle, so that
tests/test_gpu_session_tables_edges.py, which runs the same batches on the
device, is known to guard that seam."""
import os
import re

import numpy as np
import pytest

from tests import session_tables_model as M
from tests import session_tables_steer as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_constants_match_the_kernels():
    from libzmq_amd import curve
    src = open(os.path.join(ROOT, "libzmq_amd", "csrc", "zmqg_curve.hip")).read()
    send = open(os.path.join(ROOT, "libzmq_amd", "csrc", "curve_zmtp_send.hpp")).read()
    m = re.search(r"constexpr uint32_t kReplayRB = (\d+), kReplayMaxTiles = (\d+);", src)
    assert (int(m.group(1)), int(m.group(2))) == (curve.REPLAY_ROW_BLOCK, curve.REPLAY_MAX_TILES) == (64, 4096)
    m = re.search(r"constexpr uint32_t kReplayMaxSessions = (\d+);", src)
    assert int(m.group(1)) == curve.REPLAY_MAX_SESSIONS == 8192
    body = src[src.index("uint32_t replay_tile_frames(uint32_t nn, uint32_t S)"):]
    assert int(re.search(r"uint32_t T = (\d+);", body).group(1)) == curve.REPLAY_TILE_MIN == 256
    assert int(re.search(r"constexpr uint32_t kZsendMaxTiles = (\d+);", send).group(1)) == curve.ZSEND_MAX_TILES
    body = src[src.index("static uint32_t zsend_tile_frames(uint32_t nn, uint32_t keys)"):]
    assert int(re.search(r"uint32_t T = (\d+);", body).group(1)) == 256 and "tiles * keys <= (4ull << 20)" in body
    text = " ".join(open(os.path.join(ROOT, "include", "zmqg_curve.h")).read().replace("*", " ").split())
    assert "still takes its nonce" in text  # zmqg_batch_opts.max_len under ZMQG_OPT_NONCE_AUTO


def test_tile_geometry():
    assert [M.tile_frames(n, s) for n, s in ((1, 1), (10 ** 6, 256), (5, 257), (4096 * 256, 8), (4096 * 256 + 1, 8),
                                             (1, 8192), (2 ** 31 - 1, 2))] == [256, 256, 512, 256, 512, 8192, 2 ** 19]
    assert M.zsend_tile_frames(602, 8192) == 256 and M.zsend_tile_frames(600000, 8192) == 2048
    assert M.locate(0, 1, 1) == (0, 0, 0, 0)
    assert M.locate(64 * 256 - 1, 33025, 256) == (63, 0, 3, 63) and M.locate(64 * 256, 33025, 256) == (64, 1, 0, 0)
    assert M.locate(1023, 2000, 257) == (1, 0, 7, 63)


# ------------------------------------------------------------------ one batch
def check(b):
    """want == the oracle; the model == the oracle."""
    bb, e = b.build(), b.expected()
    bad = np.flatnonzero(e["status"] != bb["want"])
    assert bad.size == 0, (b.name, bad[:5].tolist(), e["status"][bad[:5]].tolist(), bb["want"][bad[:5]].tolist())
    sid, v = b.tables_input()
    got = M.replay(sid, v, b.S, b.peer0)
    disagree = model_disagrees(b, got)
    assert not disagree, (b.name, disagree)
    assert (e["smax"][b.bg] > 0).all() or b.n < 64  # the background is there
    return got


def model_disagrees(b, got):
    """Where the model's verdicts, peer nonces or session maxima differ from the oracle's."""
    e = b.expected()
    for i in e["hv_index"].tolist():
        if got["passes"].get(i, False) != (int(e["status"][i]) in (S.OK, S.CRYPTO)):
            return ("verdict", i)
    if [int(x) for x in e["peer"]] != got["peer"]:
        return ("peer",)
    if [int(x) for x in e["smax"]] != got["smax"]:
        return ("smax",)
    return None


def session_frames(b, i):
    sid = b.build()["sid_dev"]
    return np.flatnonzero(sid == sid[i])


# ------------------------------------------------------------------ landing, model against oracle
def check_tile():
    cases = S.class_tile()
    assert [c.n for c in cases] == [129 * 256 + 1, 64 * 256, 65 * 256, 256, 257, 1]
    for b in cases:
        assert M.tile_frames(b.n, b.S) == 256
        check(b)
        for kind, idx, note in b.marks:
            loc = [M.locate(i, b.n, b.S) for i in idx]
            if note.startswith("edge"):
                k = int(note[4:])
                assert loc[0][0] == k - 1 and loc[-1][0] == k and loc[1][0] == k
                if kind == "kill":
                    assert (loc[0][2], loc[0][3], loc[1][2], loc[1][3]) == (3, 63, 0, 0)
                    assert loc[0][1] != loc[1][1] if k in (64, 128) else loc[0][1] == loc[1][1]
            elif note == "tile0-tile128":
                assert [l[:2] for l in loc] == [(0, 0), (128, 2)] and len(session_frames(b, idx[0])) == 2
            elif note == "blocks0-1-2":
                assert [l[1] for l in loc] == [0, 1, 2]
            elif note == "tile63-tile64":
                assert [l[:2] for l in loc] == [(63, 0), (64, 1)]
    full, one_block, one_row = cases[:3]
    assert {m[2] for m in full.marks} >= {"edge1", "edge64", "edge65", "edge128", "edge129", "tile0-tile128",
                                          "tile63-tile64"}
    assert M.locate(full.n - 1, full.n, 256) == (129, 2, 0, 0)
    assert ("kill", (full.n - 2, full.n - 1), "edge129") in full.marks
    assert (one_block.n + 255) // 256 == M.K()["RB"] and (one_row.n + 255) // 256 == M.K()["RB"] + 1
    assert ("kill", (255, 256), "edge1") in cases[4].marks and not any(m[2].startswith("edge") for m in cases[3].marks)
    return cases


def check_step(Sn=64):
    cases = S.class_step(Sn)
    for b in cases:
        check(b)
        for kind, idx, note in b.marks:
            loc = [M.locate(i, b.n, 64) for i in idx]  # (steps are the same for any session count)
            steps = [(l[0], l[2]) for l in loc]
            lanes = [l[3] for l in loc]
            if note.startswith("lanes"):
                want = [int(x) for x in note[5:].replace("|", ",").split(",")]
                assert lanes == want, (b.name, note)
                assert (len(set(steps)) == 2) == ("|" in note)
            elif kind in ("full", "interleaved", "pairs32"):
                assert lanes == list(range(64)) and len(set(steps)) == 1
                sid = b.build()["sid_dev"][list(idx)]
                per = np.unique(sid, return_counts=True)[1]
                assert sorted(per.tolist()) == dict(full=[64], interleaved=[32, 32], pairs32=[2] * 32)[kind]
            elif kind == "dup":
                first = idx[0] - idx[0] % 64
                per = np.unique(b.build()["sid_dev"][first:first + 64], return_counts=True)[1]
                assert sorted(per.tolist()) == [1] * 62 + [2]
            elif note in ("unknown-between", "forged-between"):
                assert len(set(steps)) == 1
                between = b.build()["sid_dev"][idx[0] + 1:idx[1]]
                st = b.expected()["status"][idx[0] + 1:idx[1]]
                assert (between >= b.S).any() if note[0] == "u" else S.UNEXPECTED in st.tolist()
    assert (cases[0].n % 64, cases[1].n % 64) == (63, 1)
    assert ("kill", (1290, 1342), "last-step-of-63") in cases[0].marks
    assert ("kill", (1279, 1280), "last-step-of-1") in cases[1].marks
    assert {int(v) for v in cases[0].bad.values()} == {Sn, Sn + 1, 0xFFFFFFFF}
    return cases


def check_value():
    (b,) = cases = S.class_value()
    check(b)
    e = b.expected()
    notes = {m[2] for m in b.marks}
    assert notes == {"%x" % (2 ** 32), "%x" % (2 ** 63), "%x" % (2 ** 64 - 1)}
    where = {(k, M.locate(i[0], b.n, b.S)[0] != M.locate(i[1], b.n, b.S)[0]) for k, i, _ in b.marks}
    assert where == {("kill", False), ("kill", True), ("keep", False), ("keep", True)}
    assert int(e["peer"][b.high]) == 10 ** 6 and int(e["smax"][b.high]) == 20
    for k, s in enumerate(b.idle):
        assert int(e["peer"][s]) == 77 + k and int(e["smax"][s]) == 0 and not (b.build()["sid_dev"] == s).any()
    return cases


def check_status(Sn=256):
    cases = S.class_status(Sn)
    seen = set()
    for b in cases:
        check(b)
        for var, (i, j), where in b.marks:
            a, c = M.locate(i, b.n, 256), M.locate(j, b.n, 256)
            assert (a[0] + 1 == c[0]) if where == "tile" else (a[0], a[2]) == (c[0], c[2])
            seen.add((var, where))
            if var.startswith("big"):
                assert b.build()["wl"][j] > 4608  # curve.MAX_LEN_FRAME_KERNEL_DECODE
    assert seen == {(v, w) for v in ("tag_a", "sig_a", "short_a", "both_b", "big_kill", "big_keep", "over_a")
                    for w in ("tile", "step")}
    return cases


def check_geometry():
    a, b, c = cases = [S.geometry_257(), S.geometry_8192(), S.geometry_big()]
    assert [M.tile_frames(x.n, x.S) for x in cases] == [512, 8192, 512]
    assert c.n == M.K()["MAX_TILES"] * 256 + 1 and M.tile_frames(c.n - 1, c.S) == 256
    for x in cases:
        check(x)
        T = M.tile_frames(x.n, x.S)
        for kind, idx, note in x.marks:
            tiles = [M.locate(i, x.n, x.S)[0] for i in idx]
            if note == "T%d" % T:
                assert tiles[0] + 1 == tiles[1] and (idx[1] % T == 0 or kind == "keep")
            elif note == "inside-T512":
                assert len(set(tiles)) == 1 and idx[0] // 256 != idx[-1] // 256
    used = set(b.build()["sid_dev"].tolist())
    assert {0, 255, 256, 8191} <= used and b.n == 2 * 8192 + 1
    real = c.build()["real"]
    assert 3900 < len(real) < 4100 and (c.build()["wl"][np.setdiff1d(np.arange(c.n), real)] == 0).all()
    assert ("kill", (c.n - 2, c.n - 1), "last") in c.marks
    return cases


def check_sort():
    cases = S.class_sort_unknown()
    assert [(int(b.build()["sid_dev"][100]), b.bad[120]) for b in cases] == [
        (0, 16384), (0, 8193 + 8192), (0, 2 ** 31), (0, 0xFFFFFFFF), (1, 16385)]
    for b in cases:
        check(b)
        assert b.S == 8193 > M.K()["MAX_SESSIONS"] and 8192 in b.build()["sid_dev"]
        assert b.expected()["status"][[100, 120, 140]].tolist() == [S.OK, S.ERR_SESSION, S.SEQ]
    b = cases[0]
    assert b.bad[120] % 2 ** 14 == 0  # the low sort bits are session 0's
    return cases


def test_tile():
    check_tile()


def test_step():
    check_step()


def test_value():
    check_value()


def test_status():
    check_status()


def test_geometry():
    check_geometry()


def test_sort():
    check_sort()
    for b in S.class_step(S.SORT_S) + S.class_status(S.SORT_S):
        check(b)
        assert b.n <= 2000 and 8192 in b.build()["sid_dev"][:b.n] or "32x2" in b.name or "62dup" in b.name


# ------------------------------------------------------------------ send nonces
def nonce_cases():
    return [S.nonce_tile()] + S.nonce_step() + [S.nonce_geometry(w) for w in (257, 8192, "big")]


def nonce_disagrees(c, mut=None):
    e = c.expected()
    got = M.nonces(c.sid, c.S, c.send0, mut)
    known = np.flatnonzero(e["known"]).tolist()
    if [got["nonce"][i] for i in known] != [int(x) for x in e["nonce"][known]]:
        return "nonce"
    if any(got["nonce"][i] is not None for i in np.flatnonzero(~e["known"]).tolist()):
        return "unknown"
    return None if got["send"] == [int(x) for x in e["send"]] else "send"


def test_nonce_cases():
    cases = nonce_cases()
    for c in cases:
        assert nonce_disagrees(c) is None, c.name
        e = c.expected()
        if c.over.any():  # a frame above max_len takes its nonce: the next frame of its session is two on
            i = int(np.flatnonzero(c.over)[0])
            mine = np.flatnonzero(c.sid == c.sid[i])
            k = int(np.searchsorted(mine, i))
            assert 0 < k < len(mine) - 1 and int(e["nonce"][mine[k + 1]]) - int(e["nonce"][mine[k - 1]]) == 2
            assert e["status"][i] == S.ERR_BOUND
    starts = {int(x) for c in cases for x in c.send0}
    assert {1, 2 ** 32 - 2, 2 ** 63 - 2} <= starts
    assert any((c.sid >= c.S).any() for c in cases)
    # counters that cross 2^32 and 2^63 inside a batch
    c = cases[0]
    e = c.expected()
    assert int(e["send"][c.send0 == 2 ** 32 - 2][0]) > 2 ** 32 and int(e["send"][c.send0 == 2 ** 63 - 2][0]) > 2 ** 63


def test_send_multi_case_geometry():
    cs = S.send_multi_case()
    assert M.zsend_tile_frames(cs["n"], S.SEND_MULTI_S) == 256 < S.SEND_MULTI_S and (cs["n"] + 255) // 256 == 3
    sid = np.asarray(S.SEND_MULTI_STREAM_SID)[cs["frame_stream"]]
    assert sid[255] == sid[256] == sid[254] == sid[257] == 255 and sid[511] == sid[512]
    assert set(sid.tolist()) == set(cs["send"]) and len(cs["send"]) == 5
    send = np.ones(S.SEND_MULTI_S, np.uint64)
    for s, v in cs["send"].items():
        send[s] = v
    got = M.nonces(sid, S.SEND_MULTI_S, send, T=256)
    ctr = {s: v for s, v in cs["send"].items()}
    for i, s in enumerate(sid.tolist()):
        assert got["nonce"][i] == ctr[s] % 2 ** 64
        ctr[s] += 1


# ------------------------------------------------------------------ mutations
def _replay_killed(cases, mut):
    for b in cases:
        sid, v = b.tables_input()
        if model_disagrees(b, M.replay(sid, v, b.S, b.peer0, mut)):
            return True
    return False


MUTATION_CLASSES = [("blkprefix_short", "tile"), ("colscan_inclusive", "tile"), ("tile_end_short", "tile"),
                    ("tile_end_long", "tile"), ("dup_ignored", "step"), ("dup_all_lanes", "step"),
                    ("lane0_self", "step"), ("update_before_read", "step"), ("cmp32", "value"), ("cmp_signed", "value"),
                    ("popcount_all", "nonce"), ("update_by_one", "nonce"), ("blkprefix_short", "nonce"),
                    ("colscan_inclusive", "nonce"), ("tile_end_short", "nonce"), ("tile_end_long", "nonce")]


@pytest.mark.parametrize("mut,cls", MUTATION_CLASSES)
def test_a_mutated_model_is_caught(mut, cls):
    """Each seam is guarded: the model with one named mistake disagrees with
    the oracle on a batch of the seam's class."""
    assert mut in M.MUTATIONS
    if cls == "nonce":
        cases = S.nonce_step() if mut in ("popcount_all", "update_by_one") else [S.nonce_tile()]
        assert any(nonce_disagrees(c, mut) for c in cases)
    else:
        cases = dict(tile=lambda: S.class_tile()[:1], step=S.class_step, value=S.class_value)[cls]()
        assert _replay_killed(cases, mut)


def test_every_mutation_is_tried():
    assert {m for m, _ in MUTATION_CLASSES} == set(M.MUTATIONS)
