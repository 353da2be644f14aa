"""zmqg_forward_framed_multi: the four forward rules with a framing chosen per
side, against tests/forward_framed_model.py bit for bit.  Compared everywhere:
the receive side's outputs (also against zmqg_decode_ws_multi itself, run on a
second ctx with the same sessions), fwd, pair_off, pair_status, dst_results,
match_out / dest_out / lb_cur where the mode has them, every byte of `out`
(prefilled with a sentinel), `plain`, and every session's peer and send nonce.
The helpers are tests/test_gpu_forward.py's and its per-mode siblings'."""
import ctypes
import errno
import functools

import numpy as np
import pytest

from tests import forward_framed_model as FM
from tests import forward_lb_model as FL
from tests import forward_model as F
from tests import forward_router_model as FR
from tests import test_gpu_forward as TF
from tests import test_gpu_forward_lb as TFL
from tests import test_gpu_forward_router as TFR
from tests import test_gpu_forward_sub as TFS
from tests import ws_model as W
from tests import zmtp_send_model as M

MORE, CMD, LAST = F.MORE, F.COMMAND, 0
PAD, FILL, PEER0 = TF.PAD, TF.FILL, TF.PEER0
ZMTP, WS, WSM = FM.ZMTP, FM.WS_PLAIN, FM.WS_MASKED
STATIC, SUB, ROUTER, LB = FM.STATIC, FM.SUB, FM.ROUTER, FM.LB
RES_FILL = -1          # what the result array of the framing that is not chosen holds before and after
PLAN_FILL = 0x5B       # match_out / dest_out before the call (bytes)

_rng_bytes, _case, _ctx, _t, _tamper = TF._rng_bytes, TF._case, TF._ctx, TF._t, TF._tamper


def _keys(rng, n, masked):
    return [int(k) for k in rng.integers(0, 2 ** 32, n)] if masked else [None] * n


def _ws_stream(rng, precom, parts, masked, wsflags=None, tamper=(), nonce0=3):
    """The WebSocket frames of one connection: parts sealed as MESSAGE commands
    (the msg_t flags inside the box), frame i's flags byte wsflags[i]; one
    bytes object per frame."""
    bodies = FM.bodies(precom, parts, nonce0)
    for i in tamper:
        bodies[i] = _tamper(bodies[i])
    return [W.frame(b, k, wsflags[i] if wsflags else 0) for i, (b, k) in enumerate(zip(bodies,
                                                                                       _keys(rng, len(bodies), masked)))]


def _pair_count(C, c, mode, kw):
    ci = [0] + [int(x) for x in np.cumsum([len(x) for x in c["carry"]])]
    ri = [0] + [int(x) for x in np.cumsum([len(x) for x in c["routes"]])]
    if mode == ROUTER:
        return C.CurveContext.forward_router_pair_base(kw["flags"], ri, ci, c["max_frames"])[-1]
    if mode == LB:
        return C.CurveContext.forward_lb_pair_base(kw["flags"], ci, c["max_frames"], len(c["offs"]))[-1]
    return C.CurveContext.forward_pair_base(ri, ci, c["max_frames"])[-1]


def _mask_of(N):
    return [(0x01020304 * (p + 1)) & 0xffffffff for p in range(N)]


def _model(c, mode, recv, send, out_bytes=None, out_size=PAD, in_place=False, mask=None, **kw):
    """The model's result for case c; out_bytes None: everything fits, PAD bytes behind it."""
    return FM.model(mode, recv, send, c["precoms"], c["down"], c["arena"], c["offs"], c["lens"], c["sids"], c["peer"],
                    -1, c["max_frames"], c["carry"], None if in_place else TF._plain_init(c), c["dst_sid"], c["send"],
                    out_bytes, out_size, routes=None if mode == LB else c["routes"], mask=mask, **kw)


def _plan_tensors(torch, C, mode, N, kw):
    """The mode's table arguments as device tensors, and what reads its plan outputs back."""
    dev = torch.device("cuda", 0)
    some = lambda a, dt, vt: _t(torch, a if len(a) else np.zeros(1, dt), dt, vt)
    ids = {}
    if kw.get("src_ids") is not None:
        ids = dict(src_id_off=_t(torch, [o for o, _ in kw["src_ids"]], np.uint64, np.int64),
                   src_id_len=_t(torch, [n for _, n in kw["src_ids"]], np.uint32, np.int32))
    if mode == SUB:
        t = TFS._table(kw["subs"])
        d_match = torch.full((max(N, 1),), PLAN_FILL, dtype=torch.uint8, device=dev)
        return dict(sub_idx=some(t["idx"], np.uint32, np.int32), sub_off=some(t["off"], np.uint64, np.int64),
                    sub_len=some(t["len"], np.uint32, np.int32), sub_bytes=some(t["raw"], np.uint8, np.uint8),
                    n_subs=t["n_subs"], sub_bytes_len=t["bytes_len"], invert=kw.get("invert", False),
                    match_out=d_match), lambda: dict(match=[int(x) for x in d_match.cpu().numpy()[:N]])
    d_dest = torch.full((N + 1,), PLAN_FILL * 0x01010101, dtype=torch.int32, device=dev)
    dest = lambda: [int(x) & 0xffffffff for x in d_dest.cpu().numpy()[:N]]
    if mode == ROUTER:
        t, tab = kw.get("table"), {}
        if t is not None:
            tab = dict(id_off=some(t["off"], np.uint64, np.int64), id_len=some(t["len"], np.uint32, np.int32),
                       id_dst=some(t["dst"], np.uint32, np.int32),
                       id_bytes=some(np.frombuffer(bytes(t["raw"]), np.uint8).copy(), np.uint8, np.uint8),
                       n_ids=t["n_ids"], id_bytes_len=t["bytes_len"])
        return dict(flags=kw["flags"], dest_out=d_dest, **ids, **tab), lambda: dict(dest=dest())
    assert mode == LB
    t = kw["table"]
    d_idx, d_dst, d_cur = (some(np.asarray(t[k], np.uint32), np.uint32, np.int32)
                           for k in ("grp_idx", "lb_dst", "lb_cur"))
    G = len(t["lb_cur"])
    return (dict(flags=kw["flags"], stream_group=kw["stream_group"], grp_idx=d_idx, lb_dst=d_dst, lb_cur=d_cur,
                 n_groups=G, n_lb=t["n_lb"], dest_out=d_dest, **ids),
            lambda: dict(dest=dest(), lb_cur=[int(x) for x in d_cur.cpu().numpy().view(np.uint32)[:G]]))


def _framed(torch, C, c, mode, recv, send, N, out_bytes, out_size, in_place=False, ctx=None, d_plain=None, mask=None,
            **kw):
    """One zmqg_forward_framed_multi call on a fresh ctx (or `ctx`, which stays open)."""
    dev = torch.device("cuda", 0)
    own = ctx is None
    ctx = ctx or _ctx(C, c)
    S, D = len(c["offs"]), len(c["dst_sid"])
    assert _pair_count(C, c, mode, kw) == N
    b = TF._recv_buffers(torch, c, in_place, d_plain)
    wres = torch.full((max(S, 1), 6), RES_FILL, dtype=torch.int64, device=dev)
    ci = [0] + [int(x) for x in np.cumsum([len(x) for x in c["carry"]])]
    ri = [0] + [int(x) for x in np.cumsum([len(x) for x in c["routes"]])]
    flat = [e for x in c["carry"] for e in x]
    d_out = torch.full((max(out_size, 1),), M.SENTINEL, dtype=torch.uint8, device=dev)
    d_poff = torch.full((N + 1,), -2, dtype=torch.int64, device=dev)
    d_pst = torch.full((max(N, 1),), -1, dtype=torch.int32, device=dev)
    d_dres = torch.full((max(D, 1), 4), -1, dtype=torch.int64, device=dev)
    d_fwd = torch.full((max(S, 1), 4), -1, dtype=torch.int64, device=dev)
    d_mask = None if mask is None else _t(torch, mask if len(mask) else [0], np.uint32, np.int32)
    plan, read_plan = _plan_tensors(torch, C, mode, N, kw) if mode != STATIC else ({}, dict)
    ctx.forward_framed_multi(
        recv, send, mode, b["sid"], b["off"], b["len"], b["inp"], -1, c["max_frames"], b["foff"], b["flen"], b["poff"],
        b["plain"], b["fl"], b["st"], b["res"], _t(torch, c["dst_sid"], np.uint32, np.int32) if D else None,
        None if mode == LB else ri, None if mode == LB else [d for r in c["routes"] for d in r], d_out, d_poff, d_pst,
        d_dres, d_fwd, ws_results=wres, mask=d_mask, carry_idx=ci if flat else None,
        carry_off=_t(torch, [e[0] for e in flat], np.uint64, np.int64) if flat else None,
        carry_len=_t(torch, [e[1] for e in flat], np.uint32, np.int32) if flat else None,
        carry_flags=_t(torch, [e[2] for e in flat], np.uint8, np.uint8) if flat else None, out_bytes=out_bytes, **plan)
    torch.cuda.synchronize()
    got = TF._recv_outputs(C, ctx, b, c)
    # the result array of the framing that was not chosen is untouched
    if recv == ZMTP:
        assert bool((wres == RES_FILL).all())
    else:
        assert bool((b["res"] == -1).all())
        got["results"] = ctx.ws_results(wres)[:S]
    got.update(fwd=ctx.forward_results(d_fwd)[:S], pair_off=[int(x) for x in d_poff.cpu().numpy().view(np.uint64)],
               pair_status=[int(x) & 0xffffffff for x in d_pst.cpu().numpy()[:N]],
               dst_results=ctx.zmtp_send_results(d_dres)[:D], out=d_out.cpu().numpy()[:out_size],
               send=[ctx.get_nonce(s) for s in range(len(c["precoms"]))], d_out=d_out, d_plain=b["plain"],
               inp=b["inp"].cpu().numpy())
    got.update(read_plan())
    if own:
        ctx.close()
    return got


def _decode_ws_only(torch, C, c, masked, in_place=False):
    """zmqg_decode_ws_multi on a ctx of its own with the same sessions and arguments."""
    ctx = _ctx(C, c)
    b = TF._recv_buffers(torch, c, in_place)
    wres = torch.full((len(c["offs"]), 6), RES_FILL, dtype=torch.int64, device=torch.device("cuda", 0))
    ctx.decode_ws_multi(b["sid"], b["off"], b["len"], b["inp"], masked, -1, c["max_frames"], b["foff"], b["flen"],
                        b["poff"], b["plain"], b["fl"], b["st"], wres)
    torch.cuda.synchronize()
    got = TF._recv_outputs(C, ctx, b, c)
    got["results"] = ctx.ws_results(wres)
    ctx.close()
    return got


def _written_only_where_allowed(got, m, c, in_place):
    """Outside the returned bodies and the control payloads `plain` keeps what it held; `in` is never written
    when plain is not in."""
    rest = ~(m["recv"]["body"] | m["recv"]["ctl"])
    assert (got["plain"][:len(c["arena"])][rest] == (c["arena"][rest] if in_place else FILL)).all()
    if not in_place:
        assert (got["inp"] == c["arena"]).all()


PLAN_OUT = {STATIC: (), SUB: ("match",), ROUTER: ("dest",), LB: ("dest", "lb_cur")}


def _compare(got, m, c, mode=STATIC):
    TF._compare(got, m, c)
    for k in PLAN_OUT[mode]:
        assert got[k] == m[k], k
    # a pair that is not live: no stream, ZMQG_ERR_SESSION, UINT64_MAX, whatever the send framing is
    for p in range(m["N"]):
        if m["frame_stream"][p] == F.NO_STREAM:
            assert got["pair_status"][p] == M.ERR_SESSION and got["pair_off"][p] == M.UINT64_MAX


def _twin_case(c, m, **over):
    """The ZMTP twin of case c as a case of its own: the same sessions, routes and counters."""
    arena, offs, lens = m["twin"]
    streams = [arena[o:o + n].tobytes() for o, n in zip(offs, lens)]
    return _case(c["precoms"], c["sids"], streams, c["routes"], c["dst_sid"], c["max_frames"], c["send"],
                 peer=c["peer"], **over)


# 1 ------------------------------------------------------------------------------------------------------------------

IDS = [b"peerA", b"nobody", b"\x00peerC"]


@functools.lru_cache(maxsize=None)
def _modes_parts():
    """3 sources on sessions 0-2, 3 destinations on sessions 3-5, max_frames 4.
    s0: a two-part message whose head is a known address and topic, then a
    one-part message; s1: an unknown address, a command, a held tail; s2: a
    one-part message first, then a two-part one."""
    rng = np.random.default_rng(8801)
    precoms = [_rng_bytes(rng, 32) for _ in range(6)]
    pay = lambda n: _rng_bytes(rng, n)
    parts = [[(MORE, b"idA"), (LAST, pay(20)), (LAST, b"solo" + pay(5))],
             [(MORE, b"idX"), (LAST, pay(30)), (CMD, pay(4)), (MORE, pay(3))],
             [(LAST, b"idB" + pay(2)), (MORE, b"idB"), (LAST, pay(9))]]
    return precoms, parts


MODES_ROUTES = [[0, 1, 2], [2, 0], [1, 0]]
MODES_SEND = [1, 1, 1, 7, 2 ** 32 - 2, 2 ** 40]


def _mode_kw(mode, src_ids, lb_flags=FL.PREPEND):
    if mode == SUB:
        return dict(subs=[[b"idA", b"so"], [b"idB"], []])
    if mode == ROUTER:
        return dict(flags=FR.PREPEND | FR.ROUTE, src_ids=src_ids,
                    table=FR.table_of([(IDS[0], 2), (IDS[2], 0), (b"zzz", 1)]))
    if mode == LB:  # group 0: streams 0 and 2 over two destinations from cursor 1 (it wraps); group 1: one destination
        return dict(flags=lb_flags, src_ids=src_ids if lb_flags else None, stream_group=[0, 1, 0],
                    table=dict(grp_idx=[0, 2, 3], lb_dst=[0, 1, 2], lb_cur=[1, 5], n_lb=3))
    return {}


def _own_call(torch, C, mode, c, kw, N, cap, size):
    """The mode's own call on a ctx of its own."""
    if mode == STATIC:
        return TF._forward(torch, C, c, N, cap, size)
    if mode == SUB:
        return TFS._forward_sub(torch, C, c, N, cap, size, TFS._table(kw["subs"]))
    if mode == ROUTER:
        return TFR._forward_router(torch, C, c, kw["flags"], N, cap, size, kw["src_ids"], kw["table"])
    return TFL._forward_lb(torch, C, c, kw["flags"], kw["stream_group"], kw["table"], N, cap, size, kw["src_ids"])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [STATIC, SUB, ROUTER, LB])
def test_both_zmtp_is_the_modes_own_call(torch_cuda, C, mode):
    """recv == send == ZMTP: every output is the mode's own call's, run on a
    second ctx with the same sessions, and the model's."""
    precoms, parts = _modes_parts()
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in enumerate(parts)]
    c = _case(precoms, [0, 1, 2], streams, MODES_ROUTES, [3, 4, 5], 4, MODES_SEND)
    kw = _mode_kw(mode, TFR._park(c, IDS))
    m = _model(c, mode, ZMTP, ZMTP, **kw)
    assert sum(p[3] for p in m["pairs"]) > 0
    got = _framed(torch_cuda, C, c, mode, ZMTP, ZMTP, m["N"], m["cap"], m["size"], **kw)
    _compare(got, m, c, mode)
    own = _own_call(torch_cuda, C, mode, c, kw, m["N"], m["cap"], m["size"])
    for k in ("results", "peer", "send", "fwd", "pair_off", "pair_status", "dst_results") + PLAN_OUT[mode]:
        assert got[k] == own[k], k
    for k in TF.RECV_KEYS + ("out",):
        assert got[k].shape == own[k].shape and (got[k] == own[k]).all(), k


# 2 ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ws_recv_case(masked):
    """6 source streams (two workgroups of the per-stream scan) at max_frames
    72; 2 destinations on sessions 6, 7."""
    rng = np.random.default_rng(8802 + masked)
    precoms = [_rng_bytes(rng, 32) for _ in range(8)]
    pay = lambda n: _rng_bytes(rng, n)
    ws = lambda s, parts, **k: b"".join(_ws_stream(rng, precoms[s], parts, masked, **k))
    streams = [
        ws(0, [(LAST, pay(int(rng.integers(0, 9)))) for _ in range(70)]),    # two steps of the scan
        ws(1, [(LAST, pay(20)), (LAST, pay(21)), (LAST, pay(22)), (LAST, pay(23))], tamper=(2,)),
        ws(2, [(LAST, pay(10)), (LAST, pay(33))], wsflags=[0, W.MORE]),     # ends on an open message: held
        ws(3, [(LAST, pay(12)), (LAST, pay(5)), (LAST, pay(40))], wsflags=[0, W.COMMAND, 0]),
        b"",
        ws(5, [(LAST, pay(5))])]                                             # its session is not the ctx's
    return _case(precoms, [0, 1, 2, 3, 4, 99], streams, [[0], [1, 0], [0], [1], [1], [0]], [6, 7], 72,
                 send=[1] * 6 + [11, 2 ** 32 - 2])


@pytest.mark.gpu
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_ws_receive_zmtp_send(torch_cuda, C, masked, in_place):
    """The receive side is zmqg_decode_ws_multi's, the plan and `out` are the
    ZMTP twin's zmqg_forward_zmtp_multi's, args->results is not touched."""
    c = _ws_recv_case(masked)
    recv = WSM if masked else WS
    m = _model(c, STATIC, recv, ZMTP, in_place=in_place)
    f, r = m["fwd"], m["recv"]
    assert [x["frames"] for x in r["results"]] == [70, 4, 2, 3, 0, 1] and m["N"] == 72 * 7
    assert r["status"][72 + 2] != 0 and r["status"][72 + 3] == 0 and r["flags"][3 * 72 + 1] & CMD
    assert (f[0]["forwarded"], f[1]["forwarded"], f[1]["failed"], f[2]["held_first"], f[2]["seq"]) == (70, 2, 1, 1, 2)
    assert (f[3]["forwarded"], f[3]["held_first"], f[4]["seq"], f[5]["failed"], f[5]["forwarded"]) == (2, 3, 0, 1, 0)
    got = _framed(torch_cuda, C, c, STATIC, recv, ZMTP, m["N"], m["cap"], m["size"], in_place=in_place)
    _compare(got, m, c)
    _written_only_where_allowed(got, m, c, in_place)
    dec = _decode_ws_only(torch_cuda, C, c, masked, in_place)
    TF._same_receive_side(got, dec)
    # the twin: the same bodies in ZMTP frames through zmqg_forward_zmtp_multi
    c2 = _twin_case(c, m)
    twin = TF._forward(torch_cuda, C, c2, m["N"], m["cap"], m["size"])
    for k in ("peer", "send", "fwd", "pair_off", "pair_status", "dst_results"):
        assert got[k] == twin[k], k
    assert (got["out"] == twin["out"]).all() and (got["status"] == twin["status"]).all()
    assert (got["flags"] == twin["flags"]).all()


# 3 ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ws_send_case():
    """3 ZMTP sources on sessions 0-2, 3 destinations on sessions 3-5,
    max_frames 5.  Payloads 91 / 92 (WebSocket size 125 / 126: the header goes
    from 2 to 4 bytes) and 65,501 / 65,502 (65,535 / 65,536: 4 to 10 bytes).
    Routes of 2 and 3 destinations and one destination named twice.  s0's
    command, its held tail and the slots past every seq are dead pairs between
    live ones."""
    rng = np.random.default_rng(8803)
    precoms = [_rng_bytes(rng, 32) for _ in range(6)]
    pay = lambda n: _rng_bytes(rng, n)
    parts = [[(LAST, pay(91)), (CMD, pay(10)), (LAST, pay(92)), (MORE, pay(5))],
             [(LAST, pay(65501))],
             [(LAST, pay(65502)), (LAST, pay(20))]]
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in enumerate(parts)]
    return _case(precoms, [0, 1, 2], streams, [[0, 1], [0, 1, 2], [2, 2]], [3, 4, 5], 5,
                 send=[1, 1, 1, 7, 2 ** 32 - 2, 2 ** 40])


@functools.lru_cache(maxsize=None)
def _ws_send_model(masked, out_bytes=None, out_size=PAD):
    c = _ws_send_case()
    return _model(c, STATIC, ZMTP, WSM if masked else WS, out_bytes=out_bytes, out_size=out_size,
                  mask=_mask_of(35) if masked else None)


def _encode_ws_only(torch, C, c, m, mask, cap, size):
    """zmqg_encode_ws_multi over the model's pair frames on a ctx of its own."""
    dev = torch.device("cuda", 0)
    ctx = _ctx(C, c)
    N, D = m["N"], len(c["dst_sid"])
    lens = np.array(m["lens"], np.uint32)
    off = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
    inp = np.frombuffer(b"".join(m["payloads"]) + b"\x00", np.uint8).copy()
    d_out = torch.full((size,), M.SENTINEL, dtype=torch.uint8, device=dev)
    d_foff = torch.full((N + 1,), -2, dtype=torch.int64, device=dev)
    d_st = torch.full((N,), -1, dtype=torch.int32, device=dev)
    d_res = torch.full((D, 4), -1, dtype=torch.int64, device=dev)
    ctx.encode_ws_multi(_t(torch, c["dst_sid"], np.uint32, np.int32), _t(torch, m["frame_stream"], np.uint32, np.int32),
                        None, _t(torch, m["flags"], np.uint8, np.uint8), _t(torch, off, np.uint64, np.int64),
                        _t(torch, lens, np.uint32, np.int32), _t(torch, inp, np.uint8, np.uint8),
                        None if mask is None else _t(torch, mask, np.uint32, np.int32), d_out, d_foff, d_st, d_res,
                        out_bytes=cap)
    torch.cuda.synchronize()
    got = dict(out=d_out.cpu().numpy(), pair_off=[int(x) for x in d_foff.cpu().numpy().view(np.uint64)],
               pair_status=[int(x) & 0xffffffff for x in d_st.cpu().numpy()], dst_results=ctx.zmtp_send_results(d_res),
               send=[ctx.get_nonce(s) for s in range(len(c["precoms"]))])
    ctx.close()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_zmtp_receive_ws_send(torch_cuda, C, masked):
    """`out` is zmqg_encode_ws_multi's over the model's pair frames and the
    model's; the key of a masked pair is mask[p], p the pair index."""
    c, m = _ws_send_case(), _ws_send_model(masked)
    mask = _mask_of(m["N"]) if masked else None
    live = [p for p in range(m["N"]) if m["pairs"][p][3]]
    assert m["N"] == 35 and live == [0, 1, 4, 5, 10, 11, 12, 25, 26, 27, 28]  # dead pairs between live ones
    hdr = lambda p: m["enc"]["hdr"][p] - 1 - (4 if masked else 0)
    assert [hdr(p) for p in live] == [2, 2, 4, 4, 4, 4, 4, 10, 10, 2, 2]
    got = _framed(torch_cuda, C, c, STATIC, ZMTP, WSM if masked else WS, m["N"], m["cap"], m["size"], mask=mask)
    _compare(got, m, c)
    if masked:  # the key bytes on the wire are the pair's own, not the live ordinal's
        for p in live:
            a = got["pair_off"][p] + hdr(p)
            assert got["out"][a:a + 4].tobytes() == W.key_bytes(mask[p])
    enc = _encode_ws_only(torch_cuda, C, c, m, mask, m["cap"], m["size"])
    for k in ("pair_off", "pair_status", "dst_results", "send"):
        assert got[k] == enc[k], k
    assert (got["out"] == enc["out"]).all()
    # each destination's run is what a peer's zmqg_decode_ws_multi takes as a stream
    for t, r in enumerate(got["dst_results"]):
        p = W.parse(got["out"][r["out_off"]:r["out_off"] + r["out_bytes"]].tobytes(), masked)
        assert (len(p["frames"]), p["consumed"], p["error"]) == (r["frames"], r["out_bytes"], 0)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_ws_send_fit(torch_cuda, C, masked):
    """out_bytes cuts destination 1's run between its second and third frame:
    ZMQG_ERR_BOUND on the suffix, ENOBUFS, no nonce for a frame that did not
    fit, the sentinel intact at and past out_bytes."""
    c, full = _ws_send_case(), _ws_send_model(masked)
    mine = [p for p in range(full["N"]) if full["frame_stream"][p] == 1]
    assert len(mine) == 3
    cap = full["enc"]["frame_off"][mine[2]]
    size = full["total"] + PAD
    m = _ws_send_model(masked, cap, size)
    got = _framed(torch_cuda, C, c, STATIC, ZMTP, WSM if masked else WS, m["N"], cap, size,
                  mask=_mask_of(m["N"]) if masked else None)
    _compare(got, m, c)
    R = got["dst_results"]
    assert [r["error"] for r in R] == [0, errno.ENOBUFS, errno.ENOBUFS] and [r["frames"] for r in R] == [3, 2, 0]
    assert [got["pair_status"][p] for p in mine] == [0, 0, C.ERR_BOUND]
    assert all(got["pair_status"][p] == C.ERR_BOUND for p in range(m["N"]) if full["frame_stream"][p] == 2)
    assert got["send"][3:] == [c["send"][3] + 3, c["send"][4] + 2, c["send"][5]]
    assert (got["out"][cap:] == M.SENTINEL).all()
    assert got["pair_off"] == full["enc"]["frame_off"]  # a pair that does not fit keeps its offset


# 4 ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _control_calls():
    """Masked WebSocket sources A-D (sessions 0-3), all routed to one
    destination (session 4), max_frames 4.  A: message, ping, a two-part
    message.  B: a ping between the two parts of a message.  C: a message, then
    a close frame.  D: a message, then a frame with the MASK bit clear.  Call 2
    submits every stream from its `consumed`."""
    rng = np.random.default_rng(8804)
    precoms = [_rng_bytes(rng, 32) for _ in range(5)]
    pay = lambda n: _rng_bytes(rng, n)
    pa, pb, pc, pd = [pay(11), pay(40), pay(41)], [pay(50), pay(51)], [pay(7)], [pay(8), pay(9)]
    fa = _ws_stream(rng, precoms[0], [(LAST, pa[0]), (MORE, pa[1]), (LAST, pa[2])], True)
    fb = _ws_stream(rng, precoms[1], [(MORE, pb[0]), (LAST, pb[1])], True)
    fc = _ws_stream(rng, precoms[2], [(LAST, pc[0])], True)
    fd = _ws_stream(rng, precoms[3], [(LAST, pd[0])], True) + _ws_stream(rng, precoms[3], [(LAST, pd[1])], False,
                                                                           nonce0=4)
    ping = lambda: W.frame(b"PING", int(rng.integers(1, 2 ** 32)), opcode=W.OP_PING)
    close = W.frame(b"\x03\xe8", 0xCAFEF00D, opcode=W.OP_CLOSE)
    streams = [fa[0] + ping() + fa[1] + fa[2], fb[0] + ping() + fb[1], fc[0] + close, fd[0] + fd[1]]
    c1 = _case(precoms, [0, 1, 2, 3], streams, [[0]] * 4, [4], 4, send=[1, 1, 1, 1, 9])
    m1 = _model(c1, STATIC, WSM, ZMTP)
    res = m1["recv"]["results"]
    cons = [r["consumed"] for r in res]
    assert cons == [len(fa[0]) + 10, len(fb[0]) + 10, len(streams[2]), len(fd[0])]
    # the host's bookkeeping between the calls: B's held part becomes its carry
    assert m1["fwd"][1] == dict(seq=1, held_first=0, forwarded=0, failed=0, live=[False])
    k = 1 * 4 + 0
    held = (int(m1["recv"]["f_off"][k]), int(m1["recv"]["f_len"][k]) - 33, int(m1["recv"]["flags"][k]))
    assert held[1:] == (50, MORE)
    plain2 = TF._plain_init(c1)
    plain2[held[0]:held[0] + held[1]] = m1["recv"]["out"][held[0]:held[0] + held[1]]
    c2 = dict(c1, offs=[o + n for o, n in zip(c1["offs"], cons)], lens=[n - k for n, k in zip(c1["lens"], cons)],
              carry=[[], [held], [], []], plain=plain2, peer=m1["recv"]["peer"], send=m1["enc"]["send"])
    return c1, m1, c2, _model(c2, STATIC, WSM, ZMTP), (pa, pb, pc, pd)


@pytest.mark.gpu
def test_control_frames(torch_cuda, C):
    torch = torch_cuda
    c1, m1, c2, m2, (pa, pb, pc, pd) = _control_calls()
    r1, r2 = m1["recv"]["results"], m2["recv"]["results"]
    assert [(r["frames"], r["ctl_opcode"], r["ctl_len"], r["error"]) for r in r1] == [
        (1, 9, 4, 0), (1, 9, 4, 0), (1, 8, 2, 0), (1, 0, 0, W.EPROTO)]
    assert [f["forwarded"] for f in m1["fwd"]] == [1, 0, 1, 1] and [f["failed"] for f in m1["fwd"]] == [0] * 4
    assert [(r["frames"], r["ctl_opcode"], r["error"]) for r in r2] == [(2, 0, 0), (1, 0, 0), (0, 0, 0),
                                                                        (0, 0, W.EPROTO)]
    assert [(f["seq"], f["forwarded"]) for f in m2["fwd"]] == [(2, 2), (2, 2), (0, 0), (0, 0)]
    assert r2[3]["consumed"] == 0 and c2["lens"][2] == 0
    ctx = _ctx(C, c1)
    d_plain = torch.full((len(c1["arena"]),), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
    g1 = _framed(torch, C, c1, STATIC, WSM, ZMTP, m1["N"], m1["cap"], m1["size"], ctx=ctx, d_plain=d_plain)
    _compare(g1, m1, c1)
    _written_only_where_allowed(g1, m1, c1, False)
    for s in (0, 1):  # the ping's payload, unmasked, where the result says
        a = g1["results"][s]["ctl_off"]
        assert g1["plain"][a:a + 4].tobytes() == b"PING"
    a = g1["results"][2]["ctl_off"]
    assert g1["plain"][a:a + 2].tobytes() == b"\x03\xe8"
    g2 = _framed(torch, C, c2, STATIC, WSM, ZMTP, m2["N"], m2["cap"], m2["size"], ctx=ctx, d_plain=d_plain)
    ctx.close()
    _compare(g2, m2, c2)
    assert m2["N"] == 4 + 5 + 4 + 4
    # the destination's two runs, one behind the other, through a peer: B's parts are contiguous
    d1, d2 = g1["dst_results"][0], g2["dst_results"][0]
    both = torch.cat([g1["d_out"][d1["out_off"]:d1["out_off"] + d1["out_bytes"]],
                      g2["d_out"][d2["out_off"]:d2["out_off"] + d2["out_bytes"]]])
    msgs = TF._peer_decode(torch, C, c1["precoms"], [4], [(0, d1["out_bytes"] + d2["out_bytes"])], both, 8,
                           [PEER0] * 5)[0]
    assert msgs == [(LAST, pa[0]), (LAST, pc[0]), (LAST, pd[0]), (MORE, pa[1]), (LAST, pa[2]), (MORE, pb[0]),
                    (LAST, pb[1])]


# 5 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode,lb_flags", [(SUB, 0), (ROUTER, 0), (LB, 0), (LB, FL.PREPEND)])
def test_each_mode_with_websocket_on_both_sides(torch_cuda, C, mode, lb_flags):
    """A WebSocket server broker: masked receive side, unmasked send side.  The
    plan outputs are the mode's ZMTP call's on the ZMTP twin, `out` the model's."""
    precoms, parts = _modes_parts()
    rng = np.random.default_rng(8805)
    streams = [b"".join(_ws_stream(rng, precoms[s], p, True)) for s, p in enumerate(parts)]
    c = _case(precoms, [0, 1, 2], streams, MODES_ROUTES, [3, 4, 5], 4, MODES_SEND)
    kw = _mode_kw(mode, TFR._park(c, IDS), lb_flags)
    m = _model(c, mode, WSM, WS, **kw)
    assert sum(p[3] for p in m["pairs"]) > 0 and 0 < sum(p[3] for p in m["pairs"]) < m["N"]
    if mode == SUB:
        forwarded = [p for p, (s, q, _, _) in enumerate(m["pairs"]) if q < m["fwd"][s]["seq"] and m["fwd"][s]["live"][q]]
        assert 0 < sum(m["match"][p] for p in forwarded) < len(forwarded)  # some destinations are not subscribed
    if mode == ROUTER:
        assert {2, FR.UNKNOWN, 0} <= set(m["dest"])
    if mode == LB:
        assert m["msgs"] == [4, 1] and m["picks"][0] == [1, 0, 1, 0] and m["lb_cur"] == [1, 0]
    got = _framed(torch_cuda, C, c, mode, WSM, WS, m["N"], m["cap"], m["size"], **kw)
    _compare(got, m, c, mode)
    # the twin through the mode's own ZMTP call (its ids parked in its own plain)
    c2 = _twin_case(c, m)
    kw2 = _mode_kw(mode, TFR._park(c2, IDS), lb_flags)
    twin = _own_call(torch_cuda, C, mode, c2, kw2, m["N"], 2 ** 20, 2 ** 20)
    for k in ("peer", "send", "fwd", "pair_status") + PLAN_OUT[mode]:
        assert got[k] == twin[k], k
    assert [r["frames"] for r in got["dst_results"]] == [r["frames"] for r in twin["dst_results"]]


# 6 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_degenerate_sizes(torch_cuda, C):
    """n_streams == 0; N == 0; max_frames == 0 with carried parts, flushed in WebSocket framing."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    precoms, parts = _modes_parts()
    rng = np.random.default_rng(8806)
    streams = [b"".join(_ws_stream(rng, precoms[s], p, True)) for s, p in enumerate(parts)]
    # N == 0 (no routes at all): the receive side and fwd are done, pair_off[0] = 0, dst_results as for n == 0
    c = _case(precoms, [0, 1, 2], streams, [[], [], []], [3, 4, 5], 4, MODES_SEND)
    m = _model(c, STATIC, WSM, WSM, mask=[])
    assert m["N"] == 0 and [f["forwarded"] for f in m["fwd"]] == [3, 2, 3]
    got = _framed(torch, C, c, STATIC, WSM, WSM, 0, m["cap"], m["size"], mask=None)
    _compare(got, m, c)
    assert got["pair_off"] == [0] and got["dst_results"] == [dict(frames=0, out_off=0, out_bytes=0, error=0)] * 3
    assert [r["frames"] for r in got["results"]] == [3, 4, 3] and (got["out"] == M.SENTINEL).all()
    # max_frames == 0 with carried parts: ws_results zero-filled, the carries flushed in WebSocket framing
    plain = rng.integers(0, 256, 600, dtype=np.uint8)
    c = _case(precoms, [0, 1], [b"\x82" * 4, b"\x82" * 4], [[0], [1, 0]], [3, 4], 0, MODES_SEND,
              carry=[[(3, 223, MORE), (301, 0, CMD), (400, 1, LAST), (500, 9, MORE)], [(250, 40, LAST)]], plain=plain)
    m = _model(c, STATIC, WSM, WS)
    assert m["N"] == 4 + 2 and [f["forwarded"] for f in m["fwd"]] == [2, 1]
    got = _framed(torch, C, c, STATIC, WSM, WS, m["N"], m["cap"], m["size"])
    _compare(got, m, c)
    zero = dict(frames=0, consumed=0, out_bytes=0, error=0, ctl_opcode=0, ctl_off=0, ctl_len=0)
    assert got["results"] == [zero] * 2 and (got["plain"] == plain).all()
    run = got["out"][:got["dst_results"][0]["out_bytes"]].tobytes()
    assert len(W.parse(run, False)["frames"]) == 3 and run[0] == 0x82
    # n_streams == 0: nothing is written
    ctx = _ctx(C, c)
    keep = torch.full((16,), -3, dtype=torch.int64, device=dev)
    a = C.ForwardZmtp(ctypes.sizeof(C.ForwardZmtp), 0)
    a.fwd, a.pair_off, a.dst_results, a.n_dst, a.max_frames = C._ptr(keep), C._ptr(keep), C._ptr(keep), 1, 6
    fr = C.ForwardFraming(ctypes.sizeof(C.ForwardFraming), 0, WSM, WSM, STATIC, 0, None, C._ptr(keep), C._ptr(keep))
    assert C._lib.zmqg_forward_framed_multi(ctx._ctx, ctypes.byref(a), ctypes.byref(fr), C._stream_handle(None)) == 0
    torch.cuda.synchronize()
    assert bool((keep == -3).all())
    ctx.close()


# 7 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_einval(torch_cuda, C):
    """Every -EINVAL case of the header, with nothing queued: all outputs keep what they held."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    precoms, _ = _modes_parts()
    ctx = C.CurveContext(0, 4)
    big = C.CurveContext(0, 8193)
    z32 = torch.zeros(64, dtype=torch.int32, device=dev)
    z64 = torch.zeros(64, dtype=torch.int64, device=dev)
    buf = torch.full((256,), M.SENTINEL, dtype=torch.uint8, device=dev)
    res = torch.full((16, 6), -1, dtype=torch.int64, device=dev)
    ri, rd, ci = np.array([0, 1, 2], np.uint32), np.array([0, 1], np.uint32), np.array([0, 1, 1], np.uint32)
    sg = np.array([0, 0], np.uint32)
    keepalive = []

    def plan_of(mode, **pk):
        """A valid plan struct of the mode, then the overrides."""
        if mode == SUB:
            p = C.ForwardSubs(ctypes.sizeof(C.ForwardSubs), 0, 1, C._ptr(z32), C._ptr(z64), C._ptr(z32), C._ptr(buf),
                              0, None)
        elif mode == ROUTER:
            p = C.ForwardRouter(ctypes.sizeof(C.ForwardRouter), C.ROUTER_PREPEND | C.ROUTER_ROUTE, C._ptr(z64),
                                C._ptr(z32), 1, C._ptr(z64), C._ptr(z32), C._ptr(z32), C._ptr(buf), 0, None)
        else:
            p = C.ForwardLb(ctypes.sizeof(C.ForwardLb), C.LB_PREPEND, C._ptr(z64), C._ptr(z32), 1, sg.ctypes.data,
                            C._ptr(z32), 1, C._ptr(z32), C._ptr(z32), None)
        for k, v in pk.items():
            setattr(p, k, v)
        return p

    def call(mode=STATIC, recv=WSM, send=WSM, c=ctx._ctx, null_args=False, null_framing=False, plan="own", fr=None,
             pk=None, **kw):
        a = C.ForwardZmtp(ctypes.sizeof(C.ForwardZmtp), 0)
        a.n_streams, a.max_frames, a.max_msg_size, a.n_dst, a.out_bytes = 2, 3, -1, 2, 256
        for k in ("stream_sid", "stream_len", "frame_len", "status_out", "carry_len", "dst_sid", "pair_status"):
            setattr(a, k, C._ptr(z32))
        for k in ("stream_off", "frame_in_off", "plain_off", "carry_off", "pair_off"):
            setattr(a, k, C._ptr(z64))
        for k in ("inp", "plain", "flags_out", "carry_flags", "out"):
            setattr(a, k, C._ptr(buf))
        for k in ("results", "dst_results", "fwd"):
            setattr(a, k, C._ptr(res))
        a.route_idx, a.route_dst, a.carry_idx = ri.ctypes.data, rd.ctypes.data, ci.ctypes.data
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                keepalive.append(v)
                v = v.ctypes.data
            setattr(a, k, v)
        p = None
        if plan == "own" and mode in (SUB, ROUTER, LB):
            p = plan_of(mode, **(pk or {}))
        elif plan not in ("own", None):
            p = plan
        f = C.ForwardFraming(ctypes.sizeof(C.ForwardFraming), 0, recv, send, mode, 0,
                             None if p is None else ctypes.addressof(p), C._ptr(res), C._ptr(z32))
        for k, v in (fr or {}).items():
            setattr(f, k, v)
        return C._lib.zmqg_forward_framed_multi(c, None if null_args else ctypes.byref(a),
                                                None if null_framing else ctypes.byref(f), C._stream_handle(None))

    u32 = lambda *x: np.array(x, np.uint32)
    E = -errno.EINVAL
    # the framing struct
    assert call(null_framing=True) == E
    assert call(fr=dict(size=40)) == E and call(fr=dict(size=0)) == E and call(fr=dict(size=56)) == E
    assert call(fr=dict(reserved=1)) == E and call(fr=dict(reserved2=1)) == E
    assert call(recv=3) == E and call(send=3) == E and call(mode=4) == E and call(recv=2 ** 31) == E
    assert call(mode=STATIC, plan=plan_of(SUB)) == E
    for mode in (SUB, ROUTER, LB):
        assert call(mode=mode, plan=None) == E, mode
    # the plan struct's own size / flag cases
    assert call(mode=SUB, pk=dict(size=0)) == E and call(mode=SUB, pk=dict(flags=2)) == E
    assert call(mode=ROUTER, pk=dict(size=8)) == E and call(mode=ROUTER, pk=dict(flags=4)) == E
    assert call(mode=LB, pk=dict(size=8)) == E and call(mode=LB, pk=dict(flags=2)) == E
    assert call(mode=SUB, pk=dict(sub_idx=None)) == E and call(mode=ROUTER, pk=dict(src_id_off=None)) == E
    assert call(mode=LB, pk=dict(lb_cur=None)) == E and call(mode=LB, pk=dict(stream_group=None)) == E
    # the result array and the mask of the chosen framing
    assert call(recv=WS, fr=dict(ws_results=None)) == E and call(recv=WSM, fr=dict(ws_results=None)) == E
    assert call(recv=ZMTP, results=None) == E
    assert call(send=WSM, fr=dict(mask=None)) == E
    for mode in (SUB, ROUTER, LB):
        assert call(mode=mode, send=WSM, fr=dict(mask=None)) == E, mode
    # the mode's own cases, under WebSocket framing
    assert call(c=None) == E and call(null_args=True) == E
    assert call(size=ctypes.sizeof(C.ForwardZmtp) - 8) == E and call(reserved=1) == E
    assert call(max_frames=2 ** 31) == E and call(n_streams=2 ** 31) == E
    assert call(n_streams=2 ** 16, max_frames=2 ** 15) == E
    for k in ("stream_sid", "stream_off", "stream_len", "inp", "frame_in_off", "frame_len", "plain_off", "plain",
              "flags_out", "status_out"):
        assert call(**{k: None}) == E, k
    assert call(n_dst=8193) == E and call(c=big._ctx) == E
    assert call(dst_sid=None) == E and call(dst_results=None) == E and call(pair_off=None) == E
    assert call(out=None) == E and call(fwd=None) == E
    assert call(route_idx=None) == E and call(route_idx=u32(1, 1, 2)) == E and call(route_idx=u32(0, 2, 1)) == E
    assert call(route_dst=u32(0, 2)) == E and call(route_dst=None) == E
    assert call(carry_idx=u32(0, 2, 1)) == E and call(carry_idx=u32(1, 1, 1)) == E
    assert call(carry_off=None) == E and call(carry_len=None) == E and call(carry_flags=None) == E
    assert call(n_streams=1, max_frames=2 ** 30, route_idx=u32(0, 2), carry_idx=None) == E
    torch.cuda.synchronize()
    assert bool((res == -1).all()) and bool((buf == M.SENTINEL).all()) and bool((z64 == 0).all())
    assert bool((z32 == 0).all())
    # members a framing does not use may be NULL: these are valid, on outputs of their own.  The two
    # streams are empty (stream_len 0), so nothing is parsed: fwd reports the one carried part alone.
    o64 = [torch.zeros(64, dtype=torch.int64, device=dev) for _ in range(3)]
    o32 = [torch.zeros(64, dtype=torch.int32, device=dev) for _ in range(3)]
    o8 = [torch.zeros(256, dtype=torch.uint8, device=dev) for _ in range(3)]
    own = dict(frame_in_off=C._ptr(o64[0]), plain_off=C._ptr(o64[1]), pair_off=C._ptr(o64[2]),
               frame_len=C._ptr(o32[0]), status_out=C._ptr(o32[1]), pair_status=C._ptr(o32[2]), plain=C._ptr(o8[0]),
               flags_out=C._ptr(o8[1]), out=C._ptr(o8[2]), dst_results=C._ptr(o64[1][32:]))
    wres = torch.full((2, 6), -1, dtype=torch.int64, device=dev)
    assert call(recv=WSM, send=WS, results=None, fr=dict(ws_results=C._ptr(wres), mask=None), **own) == 0
    torch.cuda.synchronize()
    zero = dict(frames=0, consumed=0, out_bytes=0, error=0, ctl_opcode=0, ctl_off=0, ctl_len=0)
    assert ctx.ws_results(wres) == [zero] * 2
    assert ctx.forward_results(res.flatten()[:8]) == [dict(seq=1, held_first=0, forwarded=0, failed=0),
                                                             dict(seq=0, held_first=0, forwarded=0, failed=0)]
    assert call(recv=ZMTP, send=ZMTP, results=C._ptr(o64[0][32:]), fr=dict(ws_results=None, mask=None), **own) == 0
    torch.cuda.synchronize()
    ctx.close()
    big.close()
