"""zmqg_encode_zmtp_multi: frames that arrive interleaved over many connections
encoded and framed in one call, every connection's frames in a region of its
own, against tests/zmtp_send_model.py.  Every test prefills `out` with 0xEE
and compares every byte with the model, the untouched ones included, and
frame_off, the statuses, the per-stream results and the send counters."""
import errno
import functools

import numpy as np
import pytest

from oracle import zmtp_oracle as Z
from tests import zmtp_send_model as M
from tests.helpers import pack

LENS = [0, 1, 100, 221, 222, 223, 250, 300, 1024, 5000, 70000]
LENS_P = [0.1] * 9 + [0.07, 0.03]  # (the two large-frame lengths less often: they dominate the bytes)
DOWN = [False, True, False, False]  # session 1 with downgrade_sub
STREAM_SID = [0, 1, 2, 3, 1]       # 5 streams over 4 sessions: streams 1 and 4 share session 1
PAD = 64                           # bytes of `out` behind the capacity, to see that they stay untouched


def _precoms(rng, n):
    return [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _batch(n, seed=0, n_streams=5):
    rng = np.random.default_rng(1000 + 7 * n + seed)
    precoms = _precoms(rng, 4)
    b = M.make_batch(rng, n, n_streams, [0])
    b["lens"] = rng.choice(LENS, n, p=LENS_P).astype(np.uint32)
    if n >= len(LENS):  # every length at least once
        b["lens"][rng.permutation(n)[:len(LENS)]] = LENS
    b["payloads"] = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in b["lens"]]
    return precoms, b


def _ctx(C, precoms, down, send=None, enc=None, dec=None):
    ctx = C.CurveContext(0, len(precoms))
    for s, p in enumerate(precoms):
        ctx.session_set(s, p, enc or C.CLIENT_PREFIX, dec or C.SERVER_PREFIX, down[s])
        if send is not None:
            ctx.set_nonce(s, send[s])
    return ctx


def _run(torch, C, precoms, down, stream_sid, b, out_bytes, out_size, send=None, with_status=True, ctx=None):
    """One call on a fresh ctx (or `ctx`); send: the counters' start, and the
    call takes its nonces from them."""
    dev = torch.device("cuda", 0)
    own = ctx is None
    if own:
        ctx = _ctx(C, precoms, down, send)
    t = lambda a, dt, vt: torch.from_numpy(np.ascontiguousarray(a, dt).view(vt)).to(dev)
    n, S = b["n"], len(stream_sid)
    inp, in_off = pack(b["payloads"])
    d_out = torch.full((max(out_size, 1),), M.SENTINEL, dtype=torch.uint8, device=dev)
    d_foff = torch.full((n + 1,), -2, dtype=torch.int64, device=dev)
    d_st = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev) if with_status else None
    res = torch.full((S, 4), -1, dtype=torch.int64, device=dev)
    ctx.encode_zmtp_multi(t(stream_sid, np.uint32, np.int32), t(b["frame_stream"], np.uint32, np.int32),
                          None if send is not None else t(b["nonce"], np.uint64, np.int64),
                          t(b["flags"], np.uint8, np.uint8), t(in_off, np.uint64, np.int64),
                          t(b["lens"], np.uint32, np.int32), torch.from_numpy(inp).to(dev), d_out, d_foff, d_st, res,
                          out_bytes=out_bytes)
    torch.cuda.synchronize()
    got = dict(out=d_out.cpu().numpy()[:out_size], frame_off=[int(x) for x in d_foff.cpu().numpy().view(np.uint64)],
               status=None if d_st is None else [int(x) & 0xffffffff for x in d_st.cpu().numpy()[:n]],
               results=ctx.zmtp_send_results(res), send=[ctx.get_nonce(s) for s in range(len(precoms))], d_out=d_out,
               res=res)
    if own:
        ctx.close()
    return got


def _compare(got, ref, out_bytes=None):
    assert got["frame_off"] == ref["frame_off"]
    if got["status"] is not None:
        assert got["status"] == ref["status"]
    assert got["results"] == ref["results"]
    bad = np.nonzero(got["out"] != ref["out"])[0]
    assert bad.size == 0, (bad[:8].tolist(), got["out"][bad[:8]].tolist(), ref["out"][bad[:8]].tolist())
    if out_bytes is not None:
        assert (got["out"][out_bytes:] == M.SENTINEL).all()


def _total(ref):
    return ref["frame_off"][-1]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 513])
def test_interleaved_streams_match_the_model(torch_cuda, C, n):
    """Random streams per frame, every payload length class (both sides of the
    255-byte body, with and without the SUBSCRIBE / CANCEL extras, the
    large-frame kernels), n around the 64-lane group and the 256-frame tile,
    explicit nonces with 2^32 - 1, 2^32 and 2^64 - 1."""
    precoms, b = _batch(n)
    ref = M.model(precoms, DOWN, STREAM_SID, b["frame_stream"], b["nonce"], b["flags"], b["lens"], b["payloads"],
                  2 ** 62, 0)
    size = _total(ref) + PAD
    ref = M.model(precoms, DOWN, STREAM_SID, b["frame_stream"], b["nonce"], b["flags"], b["lens"], b["payloads"],
                  size - PAD, size)
    assert all(ref["fit"])
    if n >= 63:
        assert {2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1} <= set(ref["nonce"]) and set(b["flags"]) == {0, 1, 2, 3, 12, 16}
        assert len(set(int(x) for x in b["frame_stream"])) == 5
    got = _run(torch_cuda, C, precoms, DOWN, STREAM_SID, b, size - PAD, size)
    _compare(got, ref, size - PAD)
    if n == 65:  # status_out may be NULL
        _compare(_run(torch_cuda, C, precoms, DOWN, STREAM_SID, b, size - PAD, size, with_status=False), ref)


@pytest.mark.gpu
def test_same_bytes_as_encode_zmtp_on_the_sorted_batch(torch_cuda, C):
    """The frames stably sorted by stream on the host and given to
    zmqg_encode_zmtp: out[:total] is byte-identical, and each frame's offset
    is the sorted frame's."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    precoms, b = _batch(257)
    n = b["n"]
    ref = M.model(precoms, DOWN, STREAM_SID, b["frame_stream"], b["nonce"], b["flags"], b["lens"], b["payloads"],
                  2 ** 62, 0, encode=False)
    total = _total(ref)
    got = _run(torch, C, precoms, DOWN, STREAM_SID, b, total, total)
    order = np.argsort(b["frame_stream"], kind="stable")
    inp, in_off = pack(b["payloads"])
    t = lambda a, dt, vt: torch.from_numpy(np.ascontiguousarray(a, dt).view(vt)).to(dev)
    ctx = _ctx(C, precoms, DOWN)
    d_out = torch.full((total,), M.SENTINEL, dtype=torch.uint8, device=dev)
    d_foff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    ctx.encode_zmtp(t(np.asarray(STREAM_SID, np.uint32)[b["frame_stream"][order]], np.uint32, np.int32),
                    t(b["nonce"][order], np.uint64, np.int64), t(b["flags"][order], np.uint8, np.uint8),
                    t(in_off[order], np.uint64, np.int64), t(b["lens"][order], np.uint32, np.int32),
                    torch.from_numpy(inp).to(dev), d_out, d_foff)
    torch.cuda.synchronize()
    foff = d_foff.cpu().numpy().view(np.uint64)
    ctx.close()
    assert int(foff[n]) == total == got["frame_off"][n]
    assert [got["frame_off"][int(i)] for i in order] == [int(x) for x in foff[:n]]
    assert (d_out.cpu().numpy() == got["out"]).all()


def _wire_nonce(out, off, F):
    hdr = 9 if F > 257 else 2
    body = out[off + hdr:off + hdr + 16].tobytes()
    assert body[:8] == Z.MESSAGE
    return int.from_bytes(body[8:16], "big")


@pytest.mark.gpu
def test_device_nonces_in_batch_order(torch_cuda, C):
    """nonce = NULL: every session's counter, preset to its own value, is taken
    in batch order -- across the two streams that share session 1 -- and
    advances by the session's frames."""
    precoms, b = _batch(257, seed=1)
    n = b["n"]
    send = [7, 2 ** 32 - 20, 2 ** 40 + 1, 2 ** 63]
    ref = M.model(precoms, DOWN, STREAM_SID, b["frame_stream"], None, b["flags"], b["lens"], b["payloads"], 2 ** 62, 0,
                  send=send, encode=False)
    total = _total(ref)
    ref = M.model(precoms, DOWN, STREAM_SID, b["frame_stream"], None, b["flags"], b["lens"], b["payloads"], total,
                  total + PAD, send=send)
    got = _run(torch_cuda, C, precoms, DOWN, STREAM_SID, b, total, total + PAD, send=send)
    _compare(got, ref, total)
    per = [sum(1 for fs in b["frame_stream"] if STREAM_SID[int(fs)] == s) for s in range(4)]
    assert min(per) > 0 and got["send"] == ref["send"] == [send[s] + per[s] for s in range(4)]
    # the nonces on the wire, session by session, in batch order
    for s in range(4):
        mine = [i for i in range(n) if STREAM_SID[int(b["frame_stream"][i])] == s]
        wire = [_wire_nonce(got["out"], got["frame_off"][i], ref["F"][i]) for i in mine]
        assert wire == list(range(send[s], send[s] + len(mine)))
    shared = [int(b["frame_stream"][i]) for i in range(n) if STREAM_SID[int(b["frame_stream"][i])] == 1]
    assert {1, 4} == set(shared) and shared != sorted(shared)  # (the two streams really interleave)


@pytest.mark.gpu
@pytest.mark.parametrize("cut", ["total", "total-1", "mid", "zero"])
def test_capacity(torch_cuda, C, cut):
    """out_bytes = the total, one byte less, a value inside stream 2's region,
    and 0, with device nonces: ZMQG_ERR_BOUND, ENOBUFS and the prefix counts,
    no nonce taken by a frame that does not fit, no byte at or behind
    out_bytes written (`out` is larger)."""
    precoms, b = _batch(130, seed=2)
    n = b["n"]
    send = [11, 2 ** 32 - 5, 3, 2 ** 50]
    full = M.model(precoms, DOWN, STREAM_SID, b["frame_stream"], None, b["flags"], b["lens"], b["payloads"], 2 ** 62, 0,
                   send=send, encode=False)
    total = _total(full)
    r2 = full["results"][2]
    cap = dict(total=total, mid=r2["out_off"] + r2["out_bytes"] // 2, zero=0).get(cut, total - 1)
    ref = M.model(precoms, DOWN, STREAM_SID, b["frame_stream"], None, b["flags"], b["lens"], b["payloads"], cap,
                  total + PAD, send=send)
    unfit = n - sum(ref["fit"])
    if cut == "total":
        assert unfit == 0 and all(r["error"] == 0 for r in ref["results"])
    elif cut == "total-1":
        assert unfit == 1 and [r["error"] for r in ref["results"]] == [0, 0, 0, 0, errno.ENOBUFS]
    elif cut == "mid":
        assert [r["error"] for r in ref["results"]] == [0, 0] + [errno.ENOBUFS] * 3
        assert 0 < ref["results"][2]["frames"] < full["results"][2]["frames"] and ref["results"][3]["frames"] == 0
    else:
        assert unfit == n and ref["send"] == send and (ref["out"] == M.SENTINEL).all()
    assert ref["frame_off"] == full["frame_off"] and sum(ref["send"]) - sum(send) == n - unfit
    got = _run(torch_cuda, C, precoms, DOWN, STREAM_SID, b, cap, total + PAD, send=send)
    _compare(got, ref, cap)
    assert got["send"] == ref["send"]
    assert got["status"].count(C.ERR_BOUND) == unfit and got["status"].count(0) == n - unfit


@pytest.mark.gpu
def test_invalid_frames_streams_and_arguments(torch_cuda, C):
    """A frame of a stream that does not exist, a stream on a session the ctx
    does not have, an empty stream in the middle; n = 0; -EINVAL."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    precoms, b0 = _batch(200, seed=3, n_streams=7)
    b = dict(b0, frame_stream=b0["frame_stream"].copy())
    sid = [0, 9, 2, 3, 1, 0, 2]  # stream 1: no such session
    b["frame_stream"][b["frame_stream"] == 3] = 5  # stream 3 stays empty
    b["frame_stream"][[4, 77, 199]] = [7, 2 ** 31, 2 ** 32 - 1]  # no such streams
    ref = M.model(precoms, DOWN, sid, b["frame_stream"], b["nonce"], b["flags"], b["lens"], b["payloads"], 2 ** 62, 0,
                  encode=False)
    total = _total(ref)
    ref = M.model(precoms, DOWN, sid, b["frame_stream"], b["nonce"], b["flags"], b["lens"], b["payloads"], total,
                  total + PAD)
    R = ref["results"]
    assert R[1] == dict(frames=0, out_off=R[2]["out_off"], out_bytes=0, error=errno.EINVAL)
    assert R[3] == dict(frames=0, out_off=R[4]["out_off"], out_bytes=0, error=0)
    bad = [i for i in range(200) if b["frame_stream"][i] in (1, 7, 2 ** 31, 2 ** 32 - 1)]
    assert len(bad) > 10 and all(ref["status"][i] == C.ERR_SESSION and ref["frame_off"][i] == M.UINT64_MAX for i in bad)
    got = _run(torch, C, precoms, DOWN, sid, b, total, total + PAD)
    _compare(got, ref, total)
    # the neighbours' layout: as if the invalid frames and stream were absent
    keep = [i for i in range(200) if i not in bad]
    sub = dict(n=len(keep), frame_stream=b["frame_stream"][keep], lens=b["lens"][keep], flags=b["flags"][keep],
               payloads=[b["payloads"][i] for i in keep], nonce=b["nonce"][keep])
    alone = _run(torch, C, precoms, DOWN, sid, sub, total, total + PAD)
    assert (alone["out"] == got["out"]).all() and alone["results"] == got["results"]
    assert alone["frame_off"] == [got["frame_off"][i] for i in keep] + [total]

    # n = 0: frame_off[0] = 0 and every stream's result filled
    empty = dict(n=0, frame_stream=np.zeros(0, np.uint32), lens=np.zeros(0, np.uint32), flags=np.zeros(0, np.uint8),
                 payloads=[], nonce=np.zeros(0, np.uint64))
    got0 = _run(torch, C, precoms, DOWN, sid, empty, 64, 64)
    assert got0["frame_off"] == [0] and (got0["out"] == M.SENTINEL).all()
    assert got0["results"] == [dict(frames=0, out_off=0, out_bytes=0, error=errno.EINVAL if s == 1 else 0)
                               for s in range(7)]

    # -EINVAL, with nothing queued
    ctx = _ctx(C, precoms, DOWN)
    z32 = torch.zeros(8193, dtype=torch.int32, device=dev)
    z64 = torch.zeros(8193, dtype=torch.int64, device=dev)
    buf = torch.full((256,), M.SENTINEL, dtype=torch.uint8, device=dev)
    res = torch.full((8193, 4), -1, dtype=torch.int64, device=dev)
    call = lambda ns, n, foff=z64, r=res, c=ctx._ctx, fs=z32: C._lib.zmqg_encode_zmtp_multi(
        c, ns, C._ptr(z32), n, None if fs is None else C._ptr(fs), C._ptr(z64), C._ptr(buf), C._ptr(z64), C._ptr(z32),
        C._ptr(buf), C._ptr(buf), 256, None if foff is None else C._ptr(foff), C._ptr(z32),
        None if r is None else C._ptr(r), C._stream_handle(None))
    assert call(8193, 4) == -22
    assert call(0, 4) == -22
    assert call(3, 4, foff=None) == -22
    assert call(3, 4, r=None) == -22
    assert call(3, 4, fs=None) == -22
    assert call(3, 4, c=None) == -22
    assert call(3, 2 ** 31) == -22
    torch.cuda.synchronize()
    assert bool((res == -1).all()) and bool((buf == M.SENTINEL).all())
    z64[0] = 5
    assert call(0, 0) == 0  # no streams, no frames: the total alone
    torch.cuda.synchronize()
    assert int(z64[0]) == 0 and bool((res == -1).all())
    ctx.close()


@pytest.mark.gpu
def test_round_trip_through_decode_zmtp_multi(torch_cuda, C):
    """results' out_off / out_bytes are the peer's stream_off / stream_len:
    zmqg_decode_zmtp_multi on a ctx with the prefixes swapped returns every
    payload and flag, every status 0, consumed == out_bytes per stream."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    precoms = _precoms(rng, 5)
    down, stream_sid = [False, True, False, False, False], [3, 0, 4, 1, 2]
    n = 300
    b = M.make_batch(rng, n, 5, LENS[:-1], flag_choices=(0, 1, 2, 3))
    b["lens"][:len(LENS)] = LENS
    b["payloads"] = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in b["lens"]]
    ref = M.model(precoms, down, stream_sid, b["frame_stream"], b["nonce"], b["flags"], b["lens"], b["payloads"],
                  2 ** 62, 0, encode=False)
    total = _total(ref)
    got = _run(torch, C, precoms, down, stream_sid, b, total, total)
    assert got["results"] == ref["results"] and got["frame_off"] == ref["frame_off"]
    peer = _ctx(C, precoms, down, enc=C.SERVER_PREFIX, dec=C.CLIENT_PREFIX)
    per = [[i for i in range(n) if int(b["frame_stream"][i]) == s] for s in range(5)]
    max_frames = max(len(p) for p in per)
    slots = 5 * max_frames
    t = lambda a, dt, vt: torch.from_numpy(np.ascontiguousarray(a, dt).view(vt)).to(dev)
    res = got["res"].cpu().numpy().view(np.uint64)
    d_foff = torch.zeros(slots, dtype=torch.int64, device=dev)
    d_flen = torch.zeros(slots, dtype=torch.int32, device=dev)
    d_poff = torch.zeros(slots, dtype=torch.int64, device=dev)
    d_pay = torch.full((total,), 0x77, dtype=torch.uint8, device=dev)
    d_fl = torch.full((slots,), 0xEE, dtype=torch.uint8, device=dev)
    d_st = torch.full((slots,), -1, dtype=torch.int32, device=dev)
    dres = torch.full((5, 4), -1, dtype=torch.int64, device=dev)
    peer.decode_zmtp_multi(t(stream_sid, np.uint32, np.int32), t(res[:, 1], np.uint64, np.int64),
                           t(res[:, 2].astype(np.uint32), np.uint32, np.int32), got["d_out"], -1, max_frames, d_foff,
                           d_flen, d_poff, d_pay, d_fl, d_st, dres)
    torch.cuda.synchronize()
    back = peer.zmtp_results(dres)
    peer.close()
    pay, poff = d_pay.cpu().numpy(), d_poff.cpu().numpy()
    st, fl, flen = d_st.cpu().numpy(), d_fl.cpu().numpy(), d_flen.cpu().numpy()
    for s in range(5):
        assert back[s]["frames"] == len(per[s]) and back[s]["error"] == 0
        assert back[s]["consumed"] == got["results"][s]["out_bytes"]
        for j, i in enumerate(per[s]):
            k = s * max_frames + j
            assert st[k] == 0 and fl[k] == b["flags"][i] and flen[k] == 33 + int(b["lens"][i])
            assert pay[int(poff[k]):int(poff[k]) + int(b["lens"][i])].tobytes() == b["payloads"][i]


@pytest.mark.gpu
def test_many_streams(torch_cuda, C):
    """n_streams = 8192 (the LDS row's limit), n = 8192 + 37 with the 37 extra
    frames in stream 5; the layout invariants everywhere, all bytes against
    the model."""
    rng = np.random.default_rng(88)
    precoms = _precoms(rng, 8)
    down = [False, True] + [False] * 6
    S, n = 8192, 8192 + 37
    stream_sid = (np.arange(S) % 8).astype(np.uint32)
    fs = np.concatenate([rng.permutation(S), np.full(37, 5)]).astype(np.uint32)
    fs = fs[rng.permutation(n)]
    b = M.make_batch(rng, n, S, [0, 64, 222, 223, 300], frame_stream=fs)
    ref = M.model(precoms, down, stream_sid, fs, b["nonce"], b["flags"], b["lens"], b["payloads"], 2 ** 62, 0,
                  encode=False)
    total = _total(ref)
    ref = M.model(precoms, down, stream_sid, fs, b["nonce"], b["flags"], b["lens"], b["payloads"], total, total + PAD)
    got = _run(torch_cuda, C, precoms, down, stream_sid, b, total, total + PAD)
    # invariants: regions back to back in stream order, every stream's frames back to back in batch order
    R = got["results"]
    assert R[0]["out_off"] == 0 and all(R[s]["out_off"] + R[s]["out_bytes"] == R[s + 1]["out_off"] for s in range(S - 1))
    assert R[S - 1]["out_off"] + R[S - 1]["out_bytes"] == total == got["frame_off"][n]
    assert R[5]["frames"] == 38 and sum(r["frames"] for r in R) == n and all(r["error"] == 0 for r in R)
    nxt = [r["out_off"] for r in R]
    for i in range(n):
        assert got["frame_off"][i] == nxt[int(fs[i])]
        nxt[int(fs[i])] += ref["F"][i]
    assert nxt == [r["out_off"] + r["out_bytes"] for r in R]
    _compare(got, ref, total)
    for i in rng.choice(n, 64, replace=False):  # a sample of frames, spelled out
        a, F = got["frame_off"][i], ref["F"][i]
        assert (got["out"][a:a + F] == ref["out"][a:a + F]).all() and got["status"][i] == 0
        assert _wire_nonce(got["out"], a, F) == int(b["nonce"][i])
