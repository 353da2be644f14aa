"""tests/zmtp_send_model.py (the checker of zmqg_encode_zmtp_multi) against a
brute-force restatement -- every connection's _outpos built on its own, as
stream_engine_base_t::out_event does -- on tiny cases; every stream's region
parsed back by the ZMTP oracle; the out_bytes cut."""
import errno

import numpy as np
import pytest

from oracle import oracle as O
from oracle import zmtp_oracle as Z
from tests import zmtp_send_model as M
from tests.helpers import pack

SIZES = [0, 1, 100, 221, 222, 223, 250, 300, 1024]
DOWN = [False, True, False, False]
STREAM_SID = [0, 1, 2, 3, 1]  # streams 1 and 4 share session 1 (the downgrade_sub one)


def _precoms(rng, n):
    return [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]


def _brute(precoms, down, stream_sid, b, out_bytes, out_size, send=None):
    """Per connection: its frames in arrival order appended at its own write
    position, the connections' buffers then laid end to end; a frame is kept
    when it ends within out_bytes.  Nonces by a walk in arrival order."""
    n_streams, ns = len(stream_sid), len(precoms)
    sessions = M.oracle_sessions(precoms, down)
    # arrival order: which frames are sealed, and with which nonce
    per = [[] for _ in range(n_streams)]
    for i in range(b["n"]):
        s = int(b["frame_stream"][i])
        if s < n_streams and stream_sid[s] < ns:
            per[s].append(i)
    region_len = [sum(M.frame_bytes(b["flags"][i], down[stream_sid[s]], b["lens"][i]) for i in per[s])
                  for s in range(n_streams)]
    starts = [sum(region_len[:s]) for s in range(n_streams)]
    where = {}
    for s in range(n_streams):
        p = starts[s]
        for i in per[s]:
            where[i] = p
            p += M.frame_bytes(b["flags"][i], down[stream_sid[s]], b["lens"][i])
    counters = list(send) if send is not None else None
    out = np.full(out_size, M.SENTINEL, np.uint8)
    kept = [0] * n_streams
    kept_bytes = [0] * n_streams
    for i in range(b["n"]):  # arrival order
        if i not in where:
            continue
        s = int(b["frame_stream"][i])
        sid = stream_sid[s]
        F = M.frame_bytes(b["flags"][i], down[sid], b["lens"][i])
        if where[i] + F > out_bytes:
            continue
        if counters is None:
            nc = int(b["nonce"][i])
        else:
            nc, counters[sid] = counters[sid], counters[sid] + 1
        inp, in_off = pack([b["payloads"][i]])
        w = O.wire_size(int(b["flags"][i]), int(down[sid]), int(b["lens"][i]))
        body = O.encode_batch(sessions, [sid], [nc], [b["flags"][i]], in_off, [b["lens"][i]], inp, [0], w)
        fr = Z.frame(body.tobytes())
        assert len(fr) == F
        out[where[i]:where[i] + F] = np.frombuffer(fr, np.uint8)
        kept[s] += 1
        kept_bytes[s] += F
    return dict(out=out, where=where, starts=starts, kept=kept, kept_bytes=kept_bytes, counters=counters,
                total=sum(region_len), per=per)


def _case(seed, n, n_streams=5):
    rng = np.random.default_rng(seed)
    precoms = _precoms(rng, 4)
    b = M.make_batch(rng, n, n_streams, SIZES)
    return precoms, b


@pytest.mark.parametrize("n", [0, 1, 7, 40])
@pytest.mark.parametrize("auto", [False, True])
def test_model_equals_brute_force(n, auto):
    precoms, b = _case(11 + n, n)
    total = sum(M.frame_bytes(f, DOWN[STREAM_SID[int(s)]], l) for f, s, l in zip(b["flags"], b["frame_stream"],
                                                                                   b["lens"]))
    send = [5, 2 ** 32 - 2, 2 ** 40, 9] if auto else None
    for cap in sorted({total, max(total - 1, 0), total // 2, 0}):
        m = M.model(precoms, DOWN, STREAM_SID, b["frame_stream"], None if auto else b["nonce"], b["flags"], b["lens"],
                    b["payloads"], cap, total + 16, send=send)
        r = _brute(precoms, DOWN, STREAM_SID, b, cap, total + 16, send=send)
        assert (m["out"] == r["out"]).all()
        assert m["frame_off"][:n] == [r["where"][i] for i in range(n)] and m["frame_off"][n] == r["total"] == total
        assert [x["frames"] for x in m["results"]] == r["kept"]
        assert [x["out_bytes"] for x in m["results"]] == r["kept_bytes"]
        assert [x["out_off"] for x in m["results"]] == r["starts"]
        assert [x["error"] for x in m["results"]] == [errno.ENOBUFS if r["kept"][s] < len(r["per"][s]) else 0
                                                      for s in range(5)]
        assert m["status"] == [0 if f else M.ERR_BOUND for f in m["fit"]]
        if auto:
            assert m["send"] == r["counters"]
            assert [m["send"][s] - send[s] for s in range(4)] == [
                sum(r["kept"][t] for t in range(5) if STREAM_SID[t] == s) for s in range(4)]
        assert (m["out"][cap:] == M.SENTINEL).all()


def test_regions_parse_back_to_their_frames():
    """zmtp_oracle.parse over out[out_off .. +out_bytes) of each stream: exactly
    that stream's frames, in arrival order, and they decode to the payloads."""
    precoms, b = _case(5, 60)
    n = b["n"]
    m = M.model(precoms, DOWN, STREAM_SID, b["frame_stream"], b["nonce"], b["flags"], b["lens"], b["payloads"],
                2 ** 40, 2 ** 17)
    assert all(m["fit"]) and m["frame_off"][n] <= 2 ** 17
    dec = np.concatenate([O.make_sessions([p], O.SERVER_PREFIX, O.CLIENT_PREFIX, bool(d))
                          for p, d in zip(precoms, DOWN)])
    ends = sorted((r["out_off"], r["out_off"] + r["out_bytes"]) for r in m["results"])
    assert ends[0][0] == 0 and all(a[1] == c[0] for a, c in zip(ends, ends[1:])) and ends[-1][1] == m["frame_off"][n]
    for s, r in enumerate(m["results"]):
        mine = [i for i in range(n) if int(b["frame_stream"][i]) == s]
        region = m["out"][r["out_off"]:r["out_off"] + r["out_bytes"]]
        p = Z.parse(region.tobytes())
        assert p["error"] == 0 and p["consumed"] == r["out_bytes"] and len(p["frames"]) == len(mine) == r["frames"]
        for (zf, body, size), i in zip(p["frames"], mine):
            assert r["out_off"] + body - (9 if size > 255 else 2) == m["frame_off"][i]
            assert zf == (Z.LARGE if size > 255 else 0)
            peer = np.zeros(4, np.uint64)
            out, fl, st = O.decode_batch(dec, peer, [STREAM_SID[s]], [body], [size], region, [0], max(size, 1))
            want, got = b["payloads"][i], out[:size - 33].tobytes()
            assert st[0] == 0 and got.endswith(want)
            if b["flags"][i] < 4:  # (SUBSCRIBE / CANCEL carry their command name or byte in front)
                assert got == want and fl[0] == b["flags"][i]


def test_out_bytes_cut_leaves_a_prefix_per_stream():
    precoms, b = _case(9, 50)
    n = b["n"]
    full = M.model(precoms, DOWN, STREAM_SID, b["frame_stream"], b["nonce"], b["flags"], b["lens"], b["payloads"],
                   2 ** 40, 2 ** 17)
    total = full["frame_off"][n]
    mid = full["results"][2]["out_off"] + full["results"][2]["out_bytes"] // 2
    for cap in (total, total - 1, mid, 0):
        m = M.model(precoms, DOWN, STREAM_SID, b["frame_stream"], b["nonce"], b["flags"], b["lens"], b["payloads"],
                    cap, 2 ** 17)
        assert m["frame_off"] == full["frame_off"]  # the layout does not depend on the capacity
        for s in range(5):
            mine = [i for i in range(n) if int(b["frame_stream"][i]) == s]
            fits = [m["fit"][i] for i in mine]
            k = sum(fits)
            assert fits == [True] * k + [False] * (len(mine) - k)
            assert m["results"][s]["frames"] == k
            assert m["results"][s]["error"] == (errno.ENOBUFS if k < len(mine) else 0)
        # what fits is byte-identical to the uncut run; the rest is untouched
        written = np.zeros(2 ** 17, bool)
        for i in range(n):
            if m["fit"][i]:
                written[m["frame_off"][i]:m["frame_off"][i] + m["F"][i]] = True
        assert (m["out"][written] == full["out"][written]).all() and (m["out"][~written] == M.SENTINEL).all()
        assert not written[cap:].any()
    assert sum(1 for f in M.model(precoms, DOWN, STREAM_SID, b["frame_stream"], b["nonce"], b["flags"], b["lens"],
                                  b["payloads"], total - 1, 2 ** 17)["fit"] if not f) == 1


def test_invalid_frames_and_streams_take_no_room():
    precoms, b = _case(21, 30, n_streams=6)
    sid = [0, 9, 2, 3, 1, 0]  # stream 1 names a session the ctx does not have
    b["frame_stream"][4] = 6  # no such stream
    m = M.model(precoms, DOWN, sid, b["frame_stream"], b["nonce"], b["flags"], b["lens"], b["payloads"], 2 ** 40,
                2 ** 17)
    keep = [i for i in range(30) if b["frame_stream"][i] not in (1, 6)]
    sub = dict(n=len(keep), frame_stream=b["frame_stream"][keep], lens=b["lens"][keep], flags=b["flags"][keep],
               payloads=[b["payloads"][i] for i in keep], nonce=b["nonce"][keep])
    w = M.model(precoms, DOWN, sid, sub["frame_stream"], sub["nonce"], sub["flags"], sub["lens"], sub["payloads"],
                2 ** 40, 2 ** 17)
    assert (m["out"] == w["out"]).all()
    assert [m["frame_off"][i] for i in keep] == w["frame_off"][:-1] and m["frame_off"][30] == w["frame_off"][-1]
    bad = [i for i in range(30) if i not in keep]
    assert bad and all(m["frame_off"][i] == M.UINT64_MAX and m["status"][i] == M.ERR_SESSION for i in bad)
    assert m["results"][1] == dict(frames=0, out_off=m["results"][2]["out_off"], out_bytes=0, error=errno.EINVAL)
