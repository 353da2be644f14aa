"""zmqg_encode_ws_multi: frames that arrive interleaved over many connections
encoded and wrapped in WebSocket binary frames in one call, against
tests/ws_send_model.py (tests/zmtp_send_model.py's layout rules with the
WebSocket frame size, and tests/ws_model.frame, which tests/test_ws_model.py
pins to the reference's ws_encoder_t).  Every test prefills `out` with 0xEE
and compares every byte with the model, the untouched ones included, and
frame_off, the statuses, the per-stream results and the send counters."""
import errno
import functools

import numpy as np
import pytest

from tests import ws_model as W
from tests import ws_send_model as M
from tests.helpers import pack

# W + 1 on both sides of 125 / 126 and of 65,535 / 65,536 (W = 33 + len with
# flags 0), one frame above the 4.5 KiB of the frame kernels
LENS = [0, 1, 90, 91, 92, 93, 300, 1024, 5000, 65500, 65501, 65502, 65503]
LENS_P = [0.11] * 8 + [0.06] + [0.015] * 4
DOWN = [False, True, False, False]  # session 1 with downgrade_sub
STREAM_SID = [0, 1, 2, 3, 1]       # 5 streams over 4 sessions: streams 1 and 4 share session 1
PAD = 64                           # bytes of `out` behind the capacity, to see that they stay untouched


def _precoms(rng, n):
    return [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _batch(n, seed=0, n_streams=5, flag_choices=(0, 1, 2, 3, 12, 16)):
    rng = np.random.default_rng(2000 + 7 * n + seed)
    precoms = _precoms(rng, 4)
    b = M.make_batch(rng, n, n_streams, [0], flag_choices=flag_choices)
    b["lens"] = rng.choice(LENS, n, p=LENS_P).astype(np.uint32)
    if n >= len(LENS):  # every length at least once, on a plain message
        where = rng.permutation(n)[:len(LENS)]
        b["lens"][where] = LENS
        b["flags"][where] = 0
    b["payloads"] = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in b["lens"]]
    b["mask"] = rng.integers(0, 2 ** 32, n).astype(np.uint32)
    b["mask"][:3] = [0, 0xFFFFFFFF, 0x37FA213D][:min(n, 3)]
    return precoms, b


def _ctx(C, precoms, down, send=None, enc=None, dec=None):
    ctx = C.CurveContext(0, len(precoms))
    for s, p in enumerate(precoms):
        ctx.session_set(s, p, enc or C.CLIENT_PREFIX, dec or C.SERVER_PREFIX, down[s])
        if send is not None:
            ctx.set_nonce(s, send[s])
    return ctx


def _run(torch, C, precoms, down, stream_sid, b, masked, out_bytes, out_size, send=None, zmtp=False):
    """One call on a fresh ctx; send: the counters' start, and the call takes
    its nonces from them.  zmtp: zmqg_encode_zmtp_multi on the same batch."""
    dev = torch.device("cuda", 0)
    ctx = _ctx(C, precoms, down, send)
    t = lambda a, dt, vt: torch.from_numpy(np.ascontiguousarray(a, dt).view(vt)).to(dev)
    n, S = b["n"], len(stream_sid)
    inp, in_off = pack(b["payloads"])
    d_out = torch.full((max(out_size, 1),), M.SENTINEL, dtype=torch.uint8, device=dev)
    d_foff = torch.full((n + 1,), -2, dtype=torch.int64, device=dev)
    d_st = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    res = torch.full((S, 4), -1, dtype=torch.int64, device=dev)
    head = (t(stream_sid, np.uint32, np.int32), t(b["frame_stream"], np.uint32, np.int32),
            None if send is not None else t(b["nonce"], np.uint64, np.int64), t(b["flags"], np.uint8, np.uint8),
            t(in_off, np.uint64, np.int64), t(b["lens"], np.uint32, np.int32), torch.from_numpy(inp).to(dev))
    if zmtp:
        ctx.encode_zmtp_multi(*head, d_out, d_foff, d_st, res, out_bytes=out_bytes)
    else:
        ctx.encode_ws_multi(*head, t(b["mask"], np.uint32, np.int32) if masked else None, d_out, d_foff, d_st, res,
                            out_bytes=out_bytes)
    torch.cuda.synchronize()
    got = dict(out=d_out.cpu().numpy()[:out_size], frame_off=[int(x) for x in d_foff.cpu().numpy().view(np.uint64)],
               status=[int(x) & 0xffffffff for x in d_st.cpu().numpy()[:n]], results=ctx.zmtp_send_results(res),
               send=[ctx.get_nonce(s) for s in range(len(precoms))], d_out=d_out, res=res)
    ctx.close()
    return got


def _model(precoms, down, stream_sid, b, masked, out_bytes, out_size, send=None, encode=True):
    return M.model(precoms, down, stream_sid, b["frame_stream"], None if send is not None else b["nonce"], b["flags"],
                   b["lens"], b["payloads"], b["mask"] if masked else None, out_bytes, out_size, send=send,
                   encode=encode)


def _compare(got, ref, out_bytes=None):
    assert got["frame_off"] == ref["frame_off"]
    assert got["status"] == ref["status"]
    assert got["results"] == ref["results"]
    bad = np.nonzero(got["out"] != ref["out"])[0]
    assert bad.size == 0, (bad[:8].tolist(), got["out"][bad[:8]].tolist(), ref["out"][bad[:8]].tolist())
    if out_bytes is not None:
        assert (got["out"][out_bytes:] == M.SENTINEL).all()


def _total(ref):
    return ref["frame_off"][-1]


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [1, 65, 300])
def test_interleaved_streams_match_the_model(torch_cuda, C, masked, n):
    """Frames interleaved over 5 streams, sizes on both sides of 125 / 126 and
    of 65,535 / 65,536, the large-frame kernels, per-frame keys."""
    precoms, b = _batch(n)
    total = _total(_model(precoms, DOWN, STREAM_SID, b, masked, 2 ** 62, 0))
    ref = _model(precoms, DOWN, STREAM_SID, b, masked, total, total + PAD)
    assert all(ref["fit"])
    if n == 300:
        plain = [i for i in range(n) if b["flags"][i] == 0]
        key = 4 if masked else 0
        assert {ref["hdr"][i] - key for i in plain} == {3, 5, 11} and max(ref["F"]) > 65536 + 10
        assert {33 + int(b["lens"][i]) + 1 for i in plain} >= {124, 125, 126, 127, 65534, 65535, 65536, 65537}
        assert len(set(int(x) for x in b["frame_stream"])) == 5
    got = _run(torch_cuda, C, precoms, DOWN, STREAM_SID, b, masked, total, total + PAD)
    _compare(got, ref, total)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("cut", ["total-1", "mid", "zero"])
def test_capacity(torch_cuda, C, masked, cut):
    """out_bytes one byte short, inside stream 2's region, and 0, with device
    nonces: the frames that do not fit are neither written nor masked and take
    no nonce; no byte at or behind out_bytes is written."""
    precoms, b = _batch(130, seed=2)
    n = b["n"]
    send = [11, 2 ** 32 - 5, 3, 2 ** 50]
    full = _model(precoms, DOWN, STREAM_SID, b, masked, 2 ** 62, 0, send=send)
    total = _total(full)
    r2 = full["results"][2]
    cap = dict(mid=r2["out_off"] + r2["out_bytes"] // 2, zero=0).get(cut, total - 1)
    ref = _model(precoms, DOWN, STREAM_SID, b, masked, cap, total + PAD, send=send)
    unfit = n - sum(ref["fit"])
    if cut == "total-1":
        assert unfit == 1 and [r["error"] for r in ref["results"]] == [0, 0, 0, 0, errno.ENOBUFS]
    elif cut == "mid":
        assert [r["error"] for r in ref["results"]] == [0, 0] + [errno.ENOBUFS] * 3
        assert 0 < ref["results"][2]["frames"] < full["results"][2]["frames"] and ref["results"][3]["frames"] == 0
    else:
        assert unfit == n and ref["send"] == send and (ref["out"] == M.SENTINEL).all()
    assert ref["frame_off"] == full["frame_off"] and sum(ref["send"]) - sum(send) == n - unfit
    got = _run(torch_cuda, C, precoms, DOWN, STREAM_SID, b, masked, cap, total + PAD, send=send)
    _compare(got, ref, cap)
    assert got["send"] == ref["send"]
    assert got["status"].count(C.ERR_BOUND) == unfit and got["status"].count(0) == n - unfit


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_invalid_streams_and_device_nonces(torch_cuda, C, masked):
    """A frame of a stream that does not exist, a stream on a session the ctx
    does not have, an empty stream in the middle, nonce == NULL; n = 0;
    -EINVAL."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    precoms, b0 = _batch(200, seed=3, n_streams=7)
    b = dict(b0, frame_stream=b0["frame_stream"].copy())
    sid = [0, 9, 2, 3, 1, 0, 2]  # stream 1: no such session
    b["frame_stream"][b["frame_stream"] == 3] = 5  # stream 3 stays empty
    b["frame_stream"][[4, 77, 199]] = [7, 2 ** 31, 2 ** 32 - 1]  # no such streams
    send = [5, 2 ** 32 - 3, 2 ** 40, 9]
    total = _total(_model(precoms, DOWN, sid, b, masked, 2 ** 62, 0, send=send))
    ref = _model(precoms, DOWN, sid, b, masked, total, total + PAD, send=send)
    R = ref["results"]
    assert R[1] == dict(frames=0, out_off=R[2]["out_off"], out_bytes=0, error=errno.EINVAL)
    assert R[3] == dict(frames=0, out_off=R[4]["out_off"], out_bytes=0, error=0)
    bad = [i for i in range(200) if b["frame_stream"][i] in (1, 7, 2 ** 31, 2 ** 32 - 1)]
    assert len(bad) > 10 and all(ref["status"][i] == C.ERR_SESSION and ref["frame_off"][i] == M.UINT64_MAX for i in bad)
    got = _run(torch, C, precoms, DOWN, sid, b, masked, total, total + PAD, send=send)
    _compare(got, ref, total)
    assert got["send"] == ref["send"] and sum(ref["send"]) - sum(send) == 200 - len(bad)

    empty = dict(n=0, frame_stream=np.zeros(0, np.uint32), lens=np.zeros(0, np.uint32), flags=np.zeros(0, np.uint8),
                 payloads=[], nonce=np.zeros(0, np.uint64), mask=np.zeros(0, np.uint32))
    got0 = _run(torch, C, precoms, DOWN, sid, empty, masked, 64, 64)
    assert got0["frame_off"] == [0] and (got0["out"] == M.SENTINEL).all()
    assert got0["results"] == [dict(frames=0, out_off=0, out_bytes=0, error=errno.EINVAL if s == 1 else 0)
                               for s in range(7)]

    ctx = _ctx(C, precoms, DOWN)
    z32 = torch.zeros(8193, dtype=torch.int32, device=dev)
    z64 = torch.zeros(8193, dtype=torch.int64, device=dev)
    buf = torch.full((256,), M.SENTINEL, dtype=torch.uint8, device=dev)
    res = torch.full((8193, 4), -1, dtype=torch.int64, device=dev)
    call = lambda ns, n, foff=z64, r=res, c=ctx._ctx, fs=z32: C._lib.zmqg_encode_ws_multi(
        c, ns, C._ptr(z32), n, None if fs is None else C._ptr(fs), C._ptr(z64), C._ptr(buf), C._ptr(z64), C._ptr(z32),
        C._ptr(buf), C._ptr(z32) if masked else None, C._ptr(buf), 256, None if foff is None else C._ptr(foff),
        C._ptr(z32), None if r is None else C._ptr(r), C._stream_handle(None))
    assert call(8193, 4) == -22
    assert call(0, 4) == -22
    assert call(3, 4, foff=None) == -22
    assert call(3, 4, r=None) == -22
    assert call(3, 4, fs=None) == -22
    assert call(3, 4, c=None) == -22
    assert call(3, 2 ** 31) == -22
    torch.cuda.synchronize()
    assert bool((res == -1).all()) and bool((buf == M.SENTINEL).all())
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_round_trip_through_decode_ws_multi(torch_cuda, C, masked):
    """results' out_off / out_bytes are the peer's stream_off / stream_len:
    zmqg_decode_ws_multi with must_mask = masked, on a ctx with the prefixes
    swapped, returns every payload and flag, every status 0, consumed ==
    out_bytes per stream."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    S = 4  # one session each: a stream's nonces rise, and the decode replays the streams one after the other
    precoms, b = _batch(300, seed=4, n_streams=S, flag_choices=(0, 1, 2, 3))
    n, down, stream_sid = b["n"], [False] * 4, [3, 0, 2, 1]
    total = _total(_model(precoms, down, stream_sid, b, masked, 2 ** 62, 0))
    got = _run(torch, C, precoms, down, stream_sid, b, masked, total, total)
    assert all(s == 0 for s in got["status"])
    peer = _ctx(C, precoms, down, enc=C.SERVER_PREFIX, dec=C.CLIENT_PREFIX)
    per = [[i for i in range(n) if int(b["frame_stream"][i]) == s] for s in range(S)]
    max_frames = max(len(p) for p in per)
    slots = S * max_frames
    t = lambda a, dt, vt: torch.from_numpy(np.ascontiguousarray(a, dt).view(vt)).to(dev)
    res = got["res"].cpu().numpy().view(np.uint64)
    d_foff = torch.zeros(slots, dtype=torch.int64, device=dev)
    d_flen = torch.zeros(slots, dtype=torch.int32, device=dev)
    d_poff = torch.zeros(slots, dtype=torch.int64, device=dev)
    d_pay = torch.full((total,), 0x77, dtype=torch.uint8, device=dev)
    d_fl = torch.full((slots,), 0xEE, dtype=torch.uint8, device=dev)
    d_st = torch.full((slots,), -1, dtype=torch.int32, device=dev)
    dres = torch.full((S, 6), -1, dtype=torch.int64, device=dev)
    peer.decode_ws_multi(t(stream_sid, np.uint32, np.int32), t(res[:, 1], np.uint64, np.int64),
                         t(res[:, 2].astype(np.uint32), np.uint32, np.int32), got["d_out"], masked, -1, max_frames,
                         d_foff, d_flen, d_poff, d_pay, d_fl, d_st, dres)
    torch.cuda.synchronize()
    back = peer.ws_results(dres)
    peer.close()
    pay, poff = d_pay.cpu().numpy(), d_poff.cpu().numpy()
    st, fl, flen = d_st.cpu().numpy(), d_fl.cpu().numpy(), d_flen.cpu().numpy()
    for s in range(S):
        assert back[s]["frames"] == len(per[s]) and back[s]["error"] == 0 and back[s]["ctl_opcode"] == 0
        assert back[s]["consumed"] == got["results"][s]["out_bytes"]
        for j, i in enumerate(per[s]):
            k = s * max_frames + j
            assert st[k] == 0 and fl[k] == b["flags"][i] and flen[k] == 33 + int(b["lens"][i])
            assert pay[int(poff[k]):int(poff[k]) + int(b["lens"][i])].tobytes() == b["payloads"][i]


@pytest.mark.gpu
def test_frame_arithmetic_against_encode_zmtp_multi(torch_cuda, C):
    """The unmasked output of a batch against zmqg_encode_zmtp_multi's on the
    same batch: the same MESSAGE commands frame by frame, only the headers
    (and so the offsets) differ; the masked output is the unmasked one under
    each frame's key."""
    precoms, b = _batch(300)
    n = b["n"]
    ws_total = _total(_model(precoms, DOWN, STREAM_SID, b, False, 2 ** 62, 0))
    ws = _run(torch_cuda, C, precoms, DOWN, STREAM_SID, b, False, ws_total, ws_total)
    zm = _run(torch_cuda, C, precoms, DOWN, STREAM_SID, b, False, ws_total + 9 * n, ws_total + 9 * n, zmtp=True)
    mk_total = ws_total + 4 * n
    mk = _run(torch_cuda, C, precoms, DOWN, STREAM_SID, b, True, mk_total, mk_total)
    assert mk["frame_off"][n] == mk_total and all(s == 0 for s in ws["status"] + zm["status"] + mk["status"])
    for i in range(n):
        w = C.wire_size(int(b["flags"][i]), DOWN[STREAM_SID[int(b["frame_stream"][i])]], int(b["lens"][i]))
        zh, wh = 9 if w > 255 else 2, W.header_bytes(w, False)
        a, z, m = ws["frame_off"][i], zm["frame_off"][i], mk["frame_off"][i]
        cmd = zm["out"][z + zh:z + zh + w].tobytes()
        assert ws["out"][a + wh:a + wh + w].tobytes() == cmd
        assert ws["out"][a:a + wh].tobytes() == W.header(w + 1, False) + b"\x00"
        assert mk["out"][m:m + wh + 4 + w].tobytes() == W.frame(cmd, int(b["mask"][i]))
