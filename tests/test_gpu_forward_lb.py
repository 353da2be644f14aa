"""zmqg_forward_zmtp_lb_multi: zmqg_forward_zmtp_multi for a proxy whose send
side is a DEALER or a PUSH socket, against tests/forward_lb_model.py bit for
bit.  Compared everywhere: the receive side's outputs, fwd, pair_off,
pair_status, dest_out, dst_results, every byte of `out` (prefilled with 0xEE),
every session's peer and send nonce, and lb_cur; grp_idx, lb_dst and the guard
words around all three table arrays are unchanged after every call.  The
helpers are tests/test_gpu_forward.py's.  Payloads are 1 to 40 bytes."""
import ctypes
import errno
import functools

import numpy as np
import pytest

from tests import forward_lb_model as FL
from tests import forward_model as F
from tests import forward_router_model as FR
from tests import test_gpu_forward as TF
from tests import test_gpu_forward_router as TR
from tests import zmtp_send_model as M

MORE, CMD, LAST = F.MORE, F.COMMAND, 0
PAD, FILL = TF.PAD, TF.FILL
PREPEND, NO_GROUP, NONE, NO_PEER = FL.PREPEND, FL.NO_GROUP, FL.NONE, FL.NO_PEER
DEST_FILL = 0x5B5B5B5B  # what dest_out holds before the call
GUARD, GUARDS = 0x6B6B6B6B, 4  # the words in front of and behind each table array

_rng_bytes, _case, _ctx, _t, _tamper = TF._rng_bytes, TF._case, TF._ctx, TF._t, TF._tamper


def _pay(rng, lo=1, hi=40):
    return _rng_bytes(rng, int(rng.integers(lo, hi + 1)))


def _table(groups, cur, pad=0):
    """forward_lb_model's table for lists of destinations, `pad` entries in front."""
    idx, dst = [pad], [0x7fffffff] * pad
    for g in groups:
        dst += list(g)
        idx.append(len(dst))
    return dict(grp_idx=idx, lb_dst=dst, lb_cur=list(cur), n_lb=len(dst))


def _model(c, flags, group, table, src_ids=None, out_bytes=None, in_place=False):
    """The model's result for case c; out_bytes None: everything fits."""
    args = (c["precoms"], c["down"], c["arena"], c["offs"], c["lens"], c["sids"], c["peer"], -1, c["max_frames"],
            c["carry"], None if in_place else c["plain"], c["dst_sid"], c["send"], flags, src_ids, group, table)
    total = FL.model(*args, 2 ** 62, 0, encode=False)["enc"]["frame_off"][-1]
    cap = total if out_bytes is None else out_bytes
    m = FL.model(*args, cap, max(total, cap) + PAD)
    m["total"], m["cap"] = total, cap
    return m


def _dev_table(torch, table):
    """The three table arrays on the device, each between guard words."""
    guard = np.full(GUARDS, GUARD, np.uint32)
    return {k: _t(torch, np.concatenate([guard, np.asarray(table[k], np.uint32), guard]), np.uint32, np.int32)
            for k in ("grp_idx", "lb_dst", "lb_cur")}


def _table_after(d_table, table):
    """The table arrays read back, the guards checked; grp_idx and lb_dst are unchanged."""
    out = {}
    for k in ("grp_idx", "lb_dst", "lb_cur"):
        a = d_table[k].cpu().numpy().view(np.uint32)
        assert (a[:GUARDS] == GUARD).all() and (a[-GUARDS:] == GUARD).all(), k
        out[k] = [int(x) for x in a[GUARDS:-GUARDS]]
    assert out["grp_idx"] == [int(x) for x in table["grp_idx"]] and out["lb_dst"] == [int(x) for x in table["lb_dst"]]
    return out["lb_cur"]


def _forward_lb(torch, C, c, flags, group, table, N, out_bytes, out_size, src_ids=None, in_place=False, ctx=None,
                d_plain=None, want_dest=True, d_table=None):
    """One zmqg_forward_zmtp_lb_multi call on a fresh ctx (or `ctx`, which stays
    open).  table: forward_lb_model's dict; lb_dst may be longer than n_lb
    states.  d_table: the device table of an earlier call, used as it stands."""
    dev = torch.device("cuda", 0)
    own = ctx is None
    ctx = ctx or _ctx(C, c)
    S, D, G = len(c["offs"]), len(c["dst_sid"]), len(table["lb_cur"])
    b = TF._recv_buffers(torch, c, in_place, d_plain)
    ci = [0] + [int(x) for x in np.cumsum([len(x) for x in c["carry"]])]
    assert C.CurveContext.forward_lb_pair_base(flags, ci, c["max_frames"], S)[-1] == N
    flat = [e for x in c["carry"] for e in x]
    d_out = torch.full((max(out_size, 1),), M.SENTINEL, dtype=torch.uint8, device=dev)
    d_poff = torch.full((N + 1,), -2, dtype=torch.int64, device=dev)
    d_pst = torch.full((max(N, 1),), -1, dtype=torch.int32, device=dev)
    d_dres = torch.full((max(D, 1), 4), -1, dtype=torch.int64, device=dev)
    d_fwd = torch.full((max(S, 1), 4), -1, dtype=torch.int64, device=dev)
    d_dest = torch.full((N + 1,), DEST_FILL, dtype=torch.int32, device=dev) if want_dest else None
    d_table = d_table or _dev_table(torch, table)
    inner = lambda k: d_table[k][GUARDS:d_table[k].numel() - GUARDS]
    kw = {}
    if src_ids is not None:
        kw.update(src_id_off=_t(torch, [o for o, _ in src_ids], np.uint64, np.int64),
                  src_id_len=_t(torch, [n for _, n in src_ids], np.uint32, np.int32))
    ctx.forward_zmtp_lb_multi(
        b["sid"], b["off"], b["len"], b["inp"], -1, c["max_frames"], b["foff"], b["flen"], b["poff"], b["plain"],
        b["fl"], b["st"], b["res"], _t(torch, c["dst_sid"], np.uint32, np.int32) if D else None, d_out, d_poff, d_pst,
        d_dres, d_fwd, flags, group, inner("grp_idx"), inner("lb_dst"), inner("lb_cur"), n_groups=G,
        n_lb=table["n_lb"], dest_out=d_dest, carry_idx=ci if flat else None,
        carry_off=_t(torch, [e[0] for e in flat], np.uint64, np.int64) if flat else None,
        carry_len=_t(torch, [e[1] for e in flat], np.uint32, np.int32) if flat else None,
        carry_flags=_t(torch, [e[2] for e in flat], np.uint8, np.uint8) if flat else None, out_bytes=out_bytes, **kw)
    torch.cuda.synchronize()
    got = TF._recv_outputs(C, ctx, b, c)
    dest = d_dest.cpu().numpy() if want_dest else None
    assert dest is None or int(dest[N]) == DEST_FILL  # nothing behind the N entries
    got.update(fwd=ctx.forward_results(d_fwd)[:S], pair_off=[int(x) for x in d_poff.cpu().numpy().view(np.uint64)],
               pair_status=[int(x) & 0xffffffff for x in d_pst.cpu().numpy()[:N]],
               dst_results=ctx.zmtp_send_results(d_dres)[:D], out=d_out.cpu().numpy()[:out_size],
               send=[ctx.get_nonce(s) for s in range(len(c["precoms"]))], d_out=d_out, d_plain=b["plain"],
               dest=[int(x) & 0xffffffff for x in dest[:N]] if want_dest else None,
               lb_cur=_table_after(d_table, table), d_table=d_table)
    if own:
        ctx.close()
    return got


def _compare(got, m, c):
    TF._compare(got, m, c)
    assert got["dest"] is None or got["dest"] == m["dest"]
    assert got["lb_cur"] == m["lb_cur"]
    # a pair that is not live: no stream, ZMQG_ERR_SESSION, UINT64_MAX
    for p, d in enumerate(m["dest"]):
        if d >= NO_PEER:
            assert got["pair_status"][p] == M.ERR_SESSION and got["pair_off"][p] == M.UINT64_MAX


def _run(torch, C, c, flags, group, table, src_ids=None, out_bytes=None, **kw):
    """The call against the model; returns (got, m)."""
    m = _model(c, flags, group, table, src_ids, out_bytes=out_bytes, in_place=kw.get("in_place", False))
    got = _forward_lb(torch, C, c, flags, group, table, m["N"], m["cap"], m["total"] + PAD, src_ids, **kw)
    _compare(got, m, c)
    return got, m


def _runs(got):
    return [(r["out_off"], r["out_bytes"]) for r in got["dst_results"]]


def _data(parts):
    return [(fl & MORE, p) for fl, p in parts if not fl & CMD]


def _simple(seed, parts_per_stream, n_dst, max_frames=None, send0=1):
    """Streams on sessions 0 .. S - 1, destinations on the sessions behind them."""
    rng = np.random.default_rng(seed)
    S = len(parts_per_stream)
    precoms = [_rng_bytes(rng, 32) for _ in range(S + n_dst)]
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in enumerate(parts_per_stream)]
    mf = max_frames if max_frames is not None else max(len(p) for p in parts_per_stream) + 1
    return _case(precoms, list(range(S)), streams, [[] for _ in range(S)], list(range(S, S + n_dst)), mf,
                 send=[send0 + 3 * i for i in range(S + n_dst)])


# 1 ------------------------------------------------------------------------------------------------------------------

CORE_CARRIED = 29  # bytes of the carried head


@functools.lru_cache(maxsize=None)
def _core():
    """4 sources on sessions 0-3, 3 destinations on sessions 4-6, max_frames 8,
    one group {d2, d0, d1} with the cursor at 1.  The carried head lies in the
    gap in front of the first stream, in `in` and in `plain` alike."""
    rng = np.random.default_rng(7001)
    precoms = [_rng_bytes(rng, 32) for _ in range(7)]
    pay = lambda: _pay(rng)
    # s0: a single part; a 3-part message with a command between its parts; a single part; a held tail
    p0 = [(LAST, pay()), (MORE, pay()), (CMD, pay()), (MORE, pay()), (LAST, pay()), (LAST, pay()), (MORE, pay())]
    # s1: a carried head whose message these frames complete; then a single part
    p1 = [(MORE, pay()), (LAST, pay()), (LAST, pay())]
    # s2: a whole message, then a tampered tag inside the next one, valid frames behind it
    p2 = [(MORE, pay()), (LAST, pay()), (MORE, pay()), (LAST, pay()), (LAST, pay())]
    # s3: two single parts behind a command
    p3 = [(CMD, pay()), (LAST, pay()), (LAST, pay())]
    f2 = F.source_frames(precoms[2], p2)
    f2[3] = _tamper(f2[3])
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in ((0, p0), (1, p1))] + [b"".join(f2)] + [
        b"".join(F.source_frames(precoms[3], p3))]
    c = _case(precoms, [0, 1, 2, 3], streams, [[], [], [], []], [4, 5, 6], 8,
              send=[1, 1, 1, 1, 7, 2 ** 32 - 2, 2 ** 40], base_off=64)
    carried = _rng_bytes(rng, CORE_CARRIED)
    c["arena"][3:3 + CORE_CARRIED] = np.frombuffer(carried, np.uint8)
    c["plain"] = np.full(len(c["arena"]), FILL, np.uint8)
    c["plain"][3:3 + CORE_CARRIED] = c["arena"][3:3 + CORE_CARRIED]
    c["carry"][1] = [(3, CORE_CARRIED, MORE)]
    return c, (p0, p1, p2, p3, carried)


CORE_TABLE = dict(groups=[[2, 0, 1]], cur=[1])


@pytest.mark.gpu
@pytest.mark.parametrize("in_place", [False, True])
def test_core(torch_cuda, C, in_place):
    """Multi-part messages, a command between parts, a held tail, a failing
    frame and a carried head; eight messages on a ring of three, which wraps
    twice.  Every run decoded by a client ctx holds the messages the ring gave
    that destination, in stream order."""
    c, (p0, p1, p2, p3, carried) = _core()
    table = _table(CORE_TABLE["groups"], CORE_TABLE["cur"])
    m = _model(c, 0, [0] * 4, table, in_place=in_place)
    f = m["fwd"]
    assert [x["frames"] for x in m["recv"]["results"]] == [7, 3, 5, 3] and m["recv"]["status"][16 + 3] != 0
    assert (f[0]["held_first"], f[0]["forwarded"], f[0]["failed"]) == (6, 5, 0)
    assert (f[1]["seq"], f[1]["held_first"], f[1]["forwarded"]) == (4, 4, 4)
    assert (f[2]["held_first"], f[2]["forwarded"], f[2]["failed"]) == (2, 2, 1)
    assert m["N"] == 8 + 9 + 8 + 8 and m["base"] == [0, 8, 17, 25, 33]
    assert m["msgs"] == [8] and m["picks"] == [[1, 2, 0, 1, 2, 0, 1, 2]] and m["lb_cur"] == [0]
    got = _forward_lb(torch_cuda, C, c, 0, [0] * 4, table, m["N"], m["cap"], m["total"] + PAD, in_place=in_place)
    _compare(got, m, c)
    # ring entries 1, 2, 0 are destinations 0, 1, 2
    assert got["dest"][:8] == [0, 1, NONE, 1, 1, 2, NONE, NONE]
    assert got["dest"][8:17] == [0, 0, 0, 1] + [NONE] * 5
    assert got["dest"][17:25] == [2, 2] + [NONE] * 6 and got["dest"][25:] == [NONE, 0, 1] + [NONE] * 5
    # without dest_out the same outputs
    again = _forward_lb(torch_cuda, C, c, 0, [0] * 4, table, m["N"], m["cap"], m["total"] + PAD, in_place=in_place,
                        want_dest=False)
    assert (again["out"] == got["out"]).all() and again["pair_status"] == got["pair_status"]
    assert again["lb_cur"] == got["lb_cur"] == [0]
    msgs = TF._peer_decode(torch_cuda, C, c["precoms"], c["dst_sid"], _runs(got), got["d_out"], 16, [TF.PEER0] * 7)
    assert msgs[0] == _data(p0[:1]) + [(MORE, carried)] + _data(p1[:2]) + _data(p3[1:2])
    assert msgs[1] == _data(p0[1:5]) + _data(p1[2:]) + _data(p3[2:])
    assert msgs[2] == _data(p0[5:6]) + _data(p2[:2])


# 2 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_equals_the_host_routed_call(torch_cuda, C):
    """One message per stream, A = 4: every output equals
    zmqg_forward_zmtp_multi's on a second ctx with route_dst[s] the model's
    pick -- with one message a stream the host can make the choice."""
    rng = np.random.default_rng(7002)
    parts = [[(MORE, _pay(rng)), (LAST, _pay(rng))] if s % 2 else [(LAST, _pay(rng))] for s in range(6)]
    c = _simple(7002, parts, 4, max_frames=3)
    table = _table([[3, 1, 0, 2]], [2])
    got, m = _run(torch_cuda, C, c, 0, [0] * 6, table)
    pick = [m["dest"][m["base"][s]] for s in range(6)]
    assert pick == [0, 2, 3, 1, 0, 2] and got["lb_cur"] == [0]
    cp = dict(c, routes=[[t] for t in pick])
    pm = TF._model(cp)
    par = TF._forward(torch_cuda, C, cp, pm["N"], pm["cap"], pm["total"] + PAD)
    TF._compare(par, pm, cp)
    assert pm["N"] == m["N"]
    for k in ("results", "peer", "send", "fwd", "pair_off", "pair_status", "dst_results"):
        assert got[k] == par[k], k
    for k in TF.RECV_KEYS + ("out",):
        assert got[k].shape == par[k].shape and (got[k] == par[k]).all(), k


# 3 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_single_destination_with_prepend_equals_the_router_call(torch_cuda, C):
    """A = 1 with PREPEND: byte for byte zmqg_forward_zmtp_router_multi's
    PREPEND with every stream routed to that destination."""
    c, _ = _core()
    c = dict(c, carry=[list(x) for x in c["carry"]])
    src_ids = TR._park(c, [b"\x00\x00\x00\x00\x07", b"client-B", b"\x00k", b""])
    table = _table([[1]], [5])
    got, m = _run(torch_cuda, C, c, PREPEND, [0] * 4, table, src_ids)
    assert got["lb_cur"] == [0] and m["N"] == 2 * 33
    cr = dict(c, routes=[[1]] * 4)
    rm = TR._model(cr, FR.PREPEND, src_ids)
    rt = TR._forward_router(torch_cuda, C, cr, FR.PREPEND, rm["N"], rm["cap"], rm["total"] + PAD, src_ids)
    TR._compare(rt, rm, cr)
    for k in ("results", "peer", "send", "fwd", "pair_off", "pair_status", "dst_results", "dest"):
        assert got[k] == rt[k], k
    for k in TF.RECV_KEYS + ("out",):
        assert got[k].shape == rt[k].shape and (got[k] == rt[k]).all(), k


# 4 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 64, 65, 130])
@pytest.mark.parametrize("shift", [0, 1])
def test_rank_pass_wave_edges(torch_cuda, C, n, shift):
    """One stream of n one-byte frames in two-part messages.  shift 0: a head
    sits at element 64 (the first lane of the second step).  shift 1: a single
    part in front, so that one message's parts are elements 63 and 64."""
    rng = np.random.default_rng(7004)
    more = [(i + shift) % 2 == 0 and not (shift and i == 0) for i in range(n)]
    parts = [(MORE if x else LAST, _rng_bytes(rng, 1)) for x in more]
    c = _simple(7004, [parts], 3, max_frames=n + 1)
    got, m = _run(torch_cuda, C, c, 0, [0], _table([[1, 2, 0]], [2]))
    head = m["head"][0]
    if m["fwd"][0]["held_first"] > 64:  # (n = 65 without the shift: element 64 opens a message and is held)
        assert head[64] == (64 if shift == 0 else 63) and head[63] == (62 if shift == 0 else 63)
    whole = sum(1 for q in range(n) if not more[q])
    assert m["msgs"] == [whole] and got["lb_cur"] == [(2 + whole) % 3]
    # every part of a message where its head went, the heads in turn
    ring = [1, 2, 0]
    want, k = [], 2
    for q in range(m["fwd"][0]["held_first"]):
        want.append(ring[k % 3])
        k += not more[q]
    assert got["dest"][:len(want)] == want and set(got["dest"][len(want):]) <= {NONE}


# 5 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 63, 64, 65, 129])
def test_group_pass_wave_edges(torch_cuda, C, S):
    """One group of S streams with one or two messages each, max_frames 2: the
    group's wave walks them 64 a step, the sum carried across the steps."""
    rng = np.random.default_rng(7005 + S)
    parts = [[(LAST, _pay(rng, 1, 8))] * 1 if rng.integers(0, 2) else [(LAST, _pay(rng, 1, 8)), (LAST, _pay(rng, 1, 8))]
             for _ in range(S)]
    c = _simple(7005, parts, 5, max_frames=2)
    ring = [4, 0, 3, 1, 2]
    got, m = _run(torch_cuda, C, c, 0, [0] * S, _table([ring], [3], pad=1))
    total = sum(len(p) for p in parts)
    assert m["msgs"] == [total] and got["lb_cur"] == [(3 + total) % 5]
    live = [d for d in got["dest"] if d != NONE]
    assert live == [ring[(3 + i) % 5] for i in range(total)]


# 6 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 2, 3, 7])
def test_cursors(torch_cuda, C, A):
    """M below, at and above A from a cursor of 0, A - 1, A and 0xffffffff: four
    groups over copies of one ring, a stream each, one call per M."""
    rng = np.random.default_rng(7006 + A)
    ring = [int(x) for x in rng.permutation(A)]
    starts = [0, A - 1, A, 0xffffffff]
    for Mn in (A - 1, A, A + 2):
        parts = [[(LAST, _pay(rng, 1, 6)) for _ in range(Mn)] for _ in range(4)]
        c = _simple(7006, parts, A, max_frames=Mn + 1)
        got, m = _run(torch_cuda, C, c, 0, [0, 1, 2, 3], _table([ring] * 4, starts))
        assert got["lb_cur"] == [(s % A + Mn) % A for s in starts]
        for g, s in enumerate(starts):
            assert got["dest"][m["base"][g]:m["base"][g] + Mn] == [ring[(s % A + i) % A] for i in range(Mn)]


# 7 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_two_groups_an_empty_one_and_one_without_streams(torch_cuda, C):
    """Groups 0 and 1 with interleaved streams, a stream without a group, group
    2 with a stream and no destination (its messages NO_PEER, its cursor 0),
    group 3 with destinations and no stream (its cursor clamped, else kept)."""
    rng = np.random.default_rng(7007)
    group = [0, 1, 0, 1, NO_GROUP, 2, 0, 1]
    parts = [[(MORE, _pay(rng)), (LAST, _pay(rng)), (LAST, _pay(rng))] if s % 3 == 0 else
             [(LAST, _pay(rng)), (CMD, _pay(rng)), (LAST, _pay(rng)), (MORE, _pay(rng))] for s in range(8)]
    c = _simple(7007, parts, 4, max_frames=5)
    table = _table([[0, 1], [3, 2, 1], [], [0, 1, 2]], [3, 1, 9, 0xfffffff0])
    got, m = _run(torch_cuda, C, c, 0, group, table)
    assert m["msgs"] == [6, 6, 2, 0]
    assert got["lb_cur"] == [(1 + 6) % 2, (1 + 6) % 3, 0, 0xfffffff0 % 3]
    for s, g in enumerate(group):
        mine = got["dest"][m["base"][s]:m["base"][s + 1]]
        live = [d for d in mine if d != NONE]
        assert len(live) == m["fwd"][s]["forwarded"] == (3 if s % 3 == 0 else 2)
        if g in (NO_GROUP, 2):
            assert set(live) == {NO_PEER}
        else:
            assert set(live) <= set(table["lb_dst"][table["grp_idx"][g]:table["grp_idx"][g + 1]])
    msgs = TF._peer_decode(torch_cuda, C, c["precoms"], c["dst_sid"], _runs(got), got["d_out"], 24, [TF.PEER0] * 12)
    # group 0's ring {0, 1} from entry 1: s0's two messages to 1, 0; s2's to 1, 0; s6's to 1, 0
    d = lambda s, a, b: _data(parts[s][a:b])
    assert msgs[0] == d(0, 2, 3) + d(2, 2, 3) + d(6, 2, 3)
    # group 1's ring {3, 2, 1} from entry 1: s1's to 2, 1; s3's to 3, 2; s7's to 1, 3
    assert msgs[3] == d(3, 0, 2) + d(7, 2, 3)


# 8 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_untrusted_table(torch_cuda, C):
    """grp_idx falling and above n_lb; an lb_dst entry >= n_dst (NO_PEER, the
    turn consumed); a destination whose session the ctx has not (reported in
    dest_out, ZMQG_ERR_SESSION from the encode); lb_dst longer than n_lb with
    entries behind it that would be picked; the guards unchanged."""
    rng = np.random.default_rng(7008)
    parts = [[(LAST, _pay(rng)), (MORE, _pay(rng)), (LAST, _pay(rng)), (LAST, _pay(rng)), (LAST, _pay(rng))],
             [(LAST, _pay(rng))], [(LAST, _pay(rng)), (LAST, _pay(rng))]]
    c = _simple(7008, parts, 3, max_frames=6)
    c = dict(c, dst_sid=[3, 99, 5])
    # group 0: [1, 2^31) clamped to n_lb = 5: entries {9, 1, 0, 2}; group 1: [2^31, 2) falls: empty; group 2:
    # [2, 4) = {1, 0}.  lb_dst[5 ..] lies behind n_lb.
    table = dict(grp_idx=[1, 2 ** 31, 2, 4], lb_dst=[0, 9, 1, 0, 2, 0, 0, 0], lb_cur=[4, 7, 2 ** 32 - 1], n_lb=5)
    assert [FL.group_range(table, g) for g in range(3)] == [(1, 4), (5, 0), (2, 2)]
    got, m = _run(torch_cuda, C, c, 0, [0, 1, 2], table)
    # group 0 from entry 4 mod 4 = 0: 9 (no destination), 1, 0, 2
    assert got["dest"][:6] == [NO_PEER, 1, 1, 0, 2, NONE] and got["dest"][6] == NO_PEER
    # group 2 from entry (2^32 - 1) mod 2 = 1: 0, 1
    assert got["dest"][12:14] == [0, 1] and got["lb_cur"] == [0, 0, 1]
    # destination 1's session is not the ctx's: the pairs are live for dest_out, the encode reports the session
    for p in (1, 2, 13):
        assert m["pairs"][p][3] and got["pair_status"][p] == M.ERR_SESSION and got["pair_off"][p] == M.UINT64_MAX
    assert got["dst_results"][1]["error"] == errno.EINVAL and got["dst_results"][1]["frames"] == 0
    assert [r["frames"] for r in got["dst_results"]] == [2, 0, 1]


# 9 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("in_place", [False, True])
def test_prepend(torch_cuda, C, in_place):
    """Ids at odd offsets, one of length 0; the id slots are live only in front
    of heads, and an id part goes where its message goes."""
    rng = np.random.default_rng(7009)
    ids = [_rng_bytes(rng, 5), b"", _rng_bytes(rng, 40)]
    parts = [[(MORE, _pay(rng)), (CMD, _pay(rng)), (LAST, _pay(rng)), (LAST, _pay(rng)), (MORE, _pay(rng))],
             [(LAST, _pay(rng)), (LAST, _pay(rng))], [(MORE, _pay(rng)), (MORE, _pay(rng)), (LAST, _pay(rng))]]
    precoms = [_rng_bytes(rng, 32) for _ in range(5)]
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in enumerate(parts)]
    c = _case(precoms, [0, 1, 2], streams, [[], [], []], [3, 4], 5, send=[1, 1, 1, 7, 9], base_off=64 if in_place else 0)
    if in_place:
        src_ids = [(1, 5), (7, 0), (9, 40)]
        c["arena"][1:6] = np.frombuffer(ids[0], np.uint8)
        c["arena"][9:49] = np.frombuffer(ids[2], np.uint8)
    else:
        src_ids = TR._park(c, ids)
    assert all(off % 2 == 1 for off, _ in src_ids)
    got, m = _run(torch_cuda, C, c, PREPEND, [0, 0, 0], _table([[1, 0]], [0]), src_ids, in_place=in_place)
    assert m["N"] == 30 and m["msgs"] == [5] and got["lb_cur"] == [1]
    # s0: [id a1 cmd a2] -> 1, [id b] -> 0, the tail held; s1: -> 1, 0; s2: -> 1
    assert got["dest"][:10] == [1, 1, NONE, NONE, NONE, 1, 0, 0, NONE, NONE]
    assert got["dest"][10:20] == [1, 1, 0, 0] + [NONE] * 6 and got["dest"][20:] == [1, 1, NONE, 1, NONE, 1] + [NONE] * 4
    msgs = TF._peer_decode(torch_cuda, C, c["precoms"], c["dst_sid"], _runs(got), got["d_out"], 16, [TF.PEER0] * 5)
    i0, i1, i2 = [(MORE, i) for i in ids]
    assert msgs[1] == [i0] + _data(parts[0][:3]) + [i1] + _data(parts[1][:1]) + [i2] + _data(parts[2])
    assert msgs[0] == [i0] + _data(parts[0][3:4]) + [i1] + _data(parts[1][1:])


# 10 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_fit(torch_cuda, C):
    """out_bytes cuts destination 1's run in the middle of a message: the
    fitting frames are a prefix, the rest ZMQG_ERR_BOUND with no nonce taken,
    the destination ENOBUFS, nothing at or past out_bytes.  The cursor still
    advances by M: a turn is a turn."""
    rng = np.random.default_rng(7010)
    parts = [[(LAST, _pay(rng)), (MORE, _pay(rng)), (LAST, _pay(rng)), (LAST, _pay(rng)), (LAST, _pay(rng))],
             [(LAST, _pay(rng)), (LAST, _pay(rng))]]
    c = _simple(7010, parts, 2, max_frames=5)
    table = _table([[0, 1]], [0])
    group = [0, 0]
    full = _model(c, 0, group, table)
    assert full["msgs"] == [6] and [r["frames"] for r in full["enc"]["results"]] == [3, 4]
    mine = [p for p in range(full["N"]) if full["frame_stream"][p] == 1]  # [b1 b2] [d] [f]
    cap = full["enc"]["frame_off"][mine[1]] + 7
    got, m = _run(torch_cuda, C, c, 0, group, table, out_bytes=cap)
    R = got["dst_results"]
    assert (R[0]["frames"], R[0]["error"]) == (3, 0) and (R[1]["frames"], R[1]["error"]) == (1, errno.ENOBUFS)
    assert [got["pair_status"][p] for p in mine] == [0] + [C.ERR_BOUND] * 3
    assert got["send"][2:] == [c["send"][2] + 3, c["send"][3] + 1]
    assert got["pair_off"] == full["enc"]["frame_off"] and got["dest"] == full["dest"]
    assert (got["out"][cap:] == M.SENTINEL).all()
    assert got["lb_cur"] == full["lb_cur"] == [0]


# 11 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_two_calls_on_one_ctx(torch_cuda, C):
    """The second call continues the first's cursor and nonces on the same
    device table, and a message the first held is carried into the second."""
    torch = torch_cuda
    rng = np.random.default_rng(7011)
    precoms = [_rng_bytes(rng, 32) for _ in range(5)]
    pa = [(LAST, _pay(rng)), (MORE, _pay(rng)), (LAST, _pay(rng)), (LAST, _pay(rng))]
    pb = [(LAST, _pay(rng)), (LAST, _pay(rng)), (LAST, _pay(rng))]
    fa, fb = F.source_frames(precoms[0], pa), F.source_frames(precoms[1], pb)
    table = _table([[2, 0, 1]], [2])
    c1 = _case(precoms, [0, 1], [b"".join(fa[:2]), b"".join(fb[:2])], [[], []], [2, 3, 4], 4, send=[1, 1, 9, 2 ** 32 - 2, 5])
    m1 = _model(c1, 0, [0, 0], table)
    assert m1["fwd"][0]["held_first"] == 1 and m1["msgs"] == [3] and m1["lb_cur"] == [2]
    k = 0 * 4 + 1
    held = (int(m1["recv"]["f_off"][k]), int(m1["recv"]["f_len"][k]) - 33, int(m1["recv"]["flags"][k]))
    assert held[2] == MORE
    L1 = len(c1["arena"])
    c2 = _case(precoms, [0, 1], [b"".join(fa[2:]), fb[2]], [[], []], [2, 3, 4], 4, send=m1["enc"]["send"],
               peer=m1["recv"]["peer"], carry=[[held], []], base_off=L1)
    plain2 = np.full(len(c2["arena"]), FILL, np.uint8)
    plain2[held[0]:held[0] + held[1]] = m1["recv"]["out"][held[0]:held[0] + held[1]]
    c2["plain"] = plain2
    m2 = _model(c2, 0, [0, 0], dict(table, lb_cur=m1["lb_cur"]))
    assert m2["msgs"] == [3] and m2["picks"] == [[2, 0, 1]] and m2["lb_cur"] == [2]
    ctx = _ctx(C, c1)
    d_plain = torch.full((len(c2["arena"]),), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
    g1 = _forward_lb(torch, C, c1, 0, [0, 0], table, m1["N"], m1["cap"], m1["total"] + PAD, ctx=ctx,
                     d_plain=d_plain[:L1])
    _compare(g1, m1, c1)
    g2 = _forward_lb(torch, C, c2, 0, [0, 0], table, m2["N"], m2["cap"], m2["total"] + PAD, ctx=ctx, d_plain=d_plain,
                     d_table=g1["d_table"])
    ctx.close()
    _compare(g2, m2, c2)
    # call 1 from entry 2: a0 -> 1, b0 -> 2, b1 -> 0; call 2 from entry 2 again: [a1 a2] -> 1, a3 -> 2, b2 -> 0
    assert g1["dest"][:2] == [1, NONE] and g1["dest"][4:6] == [2, 0]
    assert g2["dest"][:3] == [1, 1, 2] and g2["dest"][5] == 0
    runs = []
    for t in range(3):
        r1, r2 = g1["dst_results"][t], g2["dst_results"][t]
        runs.append(torch.cat([g1["d_out"][r1["out_off"]:r1["out_off"] + r1["out_bytes"]],
                               g2["d_out"][r2["out_off"]:r2["out_off"] + r2["out_bytes"]]]))
    both = torch.cat(runs)
    offs = [0, int(runs[0].numel()), int(runs[0].numel() + runs[1].numel())]
    msgs = TF._peer_decode(torch, C, precoms, [2, 3, 4], [(o, int(r.numel())) for o, r in zip(offs, runs)], both, 8,
                           [TF.PEER0] * 5)
    assert msgs == [_data(pb[1:2]) + _data(pb[2:]), _data(pa[:1]) + _data(pa[1:3]), _data(pb[:1]) + _data(pa[3:])]


# 12 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_broker_loop(torch_cuda, C):
    """A ROUTER/DEALER broker, three clients and two workers.  Requests go
    through PREPEND and the load balancer: each worker's run, decoded as the
    peer, holds exactly [id, parts] of the messages the ring gave it.  The
    workers' replies [id, parts] come back through
    zmqg_forward_zmtp_router_multi's ROUTE to the right clients."""
    torch = torch_cuda
    rng = np.random.default_rng(7012)
    precoms = [_rng_bytes(rng, 32) for _ in range(5)]  # sessions 0-2: the clients, 3-4: the workers
    cids = [b"\x00\x00\x00\x10\x01", b"\x00\x00\x00\x10\x02", b"client-3"]
    req = lambda: [(MORE, b""), (LAST, _pay(rng))]
    requests = [req() + req(), req(), req()]  # client 0 asks twice
    c1 = _case(precoms, [0, 1, 2], [b"".join(F.source_frames(precoms[s], r)) for s, r in enumerate(requests)],
               [[], [], []], [3, 4], 5, send=[40, 41, 42, 50, 51])
    L1 = len(c1["arena"])
    src_ids = TR._park(c1, cids)
    table = _table([[0, 1]], [1])
    m1 = _model(c1, PREPEND, [0, 0, 0], table, src_ids)
    ctx = _ctx(C, c1)
    g1 = _forward_lb(torch, C, c1, PREPEND, [0, 0, 0], table, m1["N"], m1["cap"], m1["total"] + PAD, src_ids, ctx=ctx)
    _compare(g1, m1, c1)
    assert g1["lb_cur"] == [1]
    seen = TF._peer_decode(torch, C, precoms, [3, 4], _runs(g1), g1["d_out"], 12, [TF.PEER0] * 5)
    # the ring from entry 1: client 0's requests to workers 1 and 0, client 1's to 1, client 2's to 0
    i0, i1, i2 = [(MORE, i) for i in cids]
    assert seen[1] == [i0] + requests[0][:2] + [i1] + requests[1]
    assert seen[0] == [i0] + requests[0][2:] + [i2] + requests[2]
    # every worker answers each request it saw: [id, "", payload]
    replies, answers = [[], []], {0: [], 1: [], 2: []}
    for w in (0, 1):
        for k in range(0, len(seen[w]), 3):
            who = cids.index(seen[w][k][1])
            body = [(MORE, b""), (LAST, b"re:" + seen[w][k + 2][1][:30])]
            replies[w] += [(MORE, cids[who])] + body
            answers[who] += body
    c2 = _case(precoms, [3, 4], [b"".join(F.source_frames(precoms[3 + w], replies[w])) for w in (0, 1)], [[], []],
               [0, 1, 2], 7, send=m1["enc"]["send"], peer=m1["recv"]["peer"], base_off=L1)
    rtable = FR.table_of([(cid, k) for k, cid in enumerate(cids)])
    m2 = TR._model(c2, FR.ROUTE, None, rtable)
    g2 = TR._forward_router(torch, C, c2, FR.ROUTE, m2["N"], m2["cap"], m2["total"] + PAD, None, rtable, ctx=ctx,
                            no_routes=True)
    ctx.close()
    TR._compare(g2, m2, c2)
    back = TF._peer_decode(torch, C, precoms, [0, 1, 2], _runs(g2), g2["d_out"], 8, [TF.PEER0] * 5)
    # every client gets the replies to its own requests and nothing else (in pair order: worker 0's before worker 1's)
    for who in range(3):
        assert back[who] == answers[who] and len(back[who]) == len(requests[who])
    assert g2["send"][:3] == [40 + 4, 41 + 2, 42 + 2] and g1["send"][3:] == [50 + 6, 51 + 6]


# 13 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_einval(torch_cuda, C):
    """Every -EINVAL case of the header, the parent call's included, with nothing queued."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    core, _ = _core()
    ctx = _ctx(C, core)
    big = C.CurveContext(0, 8193)
    z32 = torch.zeros(64, dtype=torch.int32, device=dev)
    z64 = torch.zeros(64, dtype=torch.int64, device=dev)
    buf = torch.full((256,), M.SENTINEL, dtype=torch.uint8, device=dev)
    res = torch.full((16, 4), -1, dtype=torch.int64, device=dev)
    dout = torch.full((64,), DEST_FILL, dtype=torch.int32, device=dev)
    gidx = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    ldst = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    lcur = torch.full((8,), 0x6B6B, dtype=torch.int32, device=dev)
    ci = np.array([0, 1, 1], np.uint32)
    sg = np.array([0, 1], np.uint32)
    keepalive = []
    LB_KEYS = ("lb_size", "flags", "src_id_off", "src_id_len", "n_groups", "stream_group", "grp_idx", "n_lb", "lb_dst",
               "lb_cur", "dest_out")

    def call(flags, c=ctx._ctx, null_args=False, null_lb=False, **kw):
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
        a.carry_idx = ci.ctypes.data  # (route_idx / route_dst stay NULL)
        lb = C.ForwardLb(ctypes.sizeof(C.ForwardLb), flags, C._ptr(z64), C._ptr(z32), 2, sg.ctypes.data, C._ptr(gidx), 2,
                         C._ptr(ldst), C._ptr(lcur), C._ptr(dout))
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                keepalive.append(v)
                v = v.ctypes.data
            if k in LB_KEYS:
                setattr(lb, "size" if k == "lb_size" else k, v)
            else:
                setattr(a, k, v)
        return C._lib.zmqg_forward_zmtp_lb_multi(c, None if null_args else ctypes.byref(a),
                                                 None if null_lb else ctypes.byref(lb), C._stream_handle(None))

    u32 = lambda *x: np.array(x, np.uint32)
    E = -errno.EINVAL
    for fl in (0, PREPEND):
        # the struct's cases
        assert call(fl, null_lb=True) == E
        assert call(fl, lb_size=ctypes.sizeof(C.ForwardLb) - 8) == E and call(fl, lb_size=0) == E
        assert call(fl | 2) == E and call(fl | 4) == E and call(fl | 2 ** 31) == E
        assert call(fl, n_groups=2 ** 31) == E and call(fl, n_lb=2 ** 31) == E
        assert call(fl, grp_idx=None) == E and call(fl, lb_cur=None) == E and call(fl, lb_dst=None) == E
        assert call(fl, stream_group=None) == E
        assert call(fl, stream_group=u32(0, 2)) == E and call(fl, stream_group=u32(2 ** 32 - 2, 0)) == E
        assert call(fl, n_groups=0, grp_idx=None, lb_cur=None) == E  # stream_group names groups 0 and 1
        assert call(fl, n_dst=0) == E  # frames and no streams
        # the parent call's
        assert call(fl, c=None) == E and call(fl, null_args=True) == E
        assert call(fl, size=ctypes.sizeof(C.ForwardZmtp) - 8) == E and call(fl, reserved=1) == E
        assert call(fl, results=None) == E and call(fl, max_frames=2 ** 31) == E and call(fl, n_streams=2 ** 31) == E
        assert call(fl, n_streams=2 ** 16, max_frames=2 ** 15, stream_group=np.zeros(2 ** 16, np.uint32),
                    carry_idx=None) == E
        for k in ("stream_sid", "stream_off", "stream_len", "inp", "frame_in_off", "frame_len", "plain_off", "plain",
                  "flags_out", "status_out"):
            assert call(fl, **{k: None}) == E, k
        assert call(fl, n_dst=8193) == E and call(fl, c=big._ctx) == E
        assert call(fl, dst_sid=None) == E and call(fl, dst_results=None) == E and call(fl, pair_off=None) == E
        assert call(fl, out=None) == E and call(fl, fwd=None) == E
        assert call(fl, carry_idx=u32(0, 2, 1)) == E and call(fl, carry_idx=u32(1, 1, 1)) == E
        assert call(fl, carry_off=None) == E and call(fl, carry_len=None) == E and call(fl, carry_flags=None) == E
    assert call(PREPEND, src_id_off=None) == E and call(PREPEND, src_id_len=None) == E
    # N as this pair space counts it: one route slot a stream, twice the slots under PREPEND
    assert call(0, n_streams=2, max_frames=2 ** 30, carry_idx=None) == E
    assert call(PREPEND, n_streams=1, max_frames=2 ** 30, carry_idx=None, stream_group=u32(0)) == E
    torch.cuda.synchronize()
    assert bool((res == -1).all()) and bool((buf == M.SENTINEL).all()) and bool((z64 == 0).all())
    assert bool((dout == DEST_FILL).all()) and bool((z32 == 0).all()) and bool((lcur == 0x6B6B).all())
    # what is no error (with outputs of their own): the arguments the cases above start from; arbitrary routes
    # (not read); a null dest_out; null ids without PREPEND; no groups with every stream NO_GROUP
    o64 = [torch.zeros(64, dtype=torch.int64, device=dev) for _ in range(3)]
    o32 = [torch.zeros(64, dtype=torch.int32, device=dev) for _ in range(3)]
    o8 = [torch.zeros(256, dtype=torch.uint8, device=dev) for _ in range(3)]
    own = dict(frame_in_off=C._ptr(o64[0]), plain_off=C._ptr(o64[1]), pair_off=C._ptr(o64[2]),
               frame_len=C._ptr(o32[0]), status_out=C._ptr(o32[1]), pair_status=C._ptr(o32[2]), plain=C._ptr(o8[0]),
               flags_out=C._ptr(o8[1]), out=C._ptr(o8[2]), results=C._ptr(o64[0][32:]),
               dst_results=C._ptr(o64[1][32:]))
    for fl in (0, PREPEND):
        assert call(fl, **own) == 0
    torch.cuda.synchronize()
    assert lcur.tolist() == [0, 0] + [0x6B6B] * 6  # 0x6B6B mod 1, both groups
    assert call(0, route_idx=u32(7, 1, 0), route_dst=u32(9, 9), **own) == 0
    assert call(0, src_id_off=None, src_id_len=None, dest_out=None, **own) == 0
    assert call(0, n_groups=0, grp_idx=None, lb_cur=None, n_lb=0, lb_dst=None,
                stream_group=u32(NO_GROUP, NO_GROUP), **own) == 0
    torch.cuda.synchronize()
    assert ctx.forward_results(res[:2]) == [dict(seq=1, held_first=0, forwarded=0, failed=0),
                                            dict(seq=0, held_first=0, forwarded=0, failed=0)]
    # N = (1 + 3) + 3 pairs, twice as many under PREPEND, none forwarded; nothing behind them is written
    assert bool((dout[:14] == -1).all()) and bool((dout[14:] == DEST_FILL).all())
    ctx.close()
    big.close()


@pytest.mark.gpu
def test_edges(torch_cuda, C):
    """n_streams == 0; N == 0; max_frames == 0 with carries; no groups with
    every stream NO_GROUP; dest_out NULL (test_core)."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    core, _ = _core()
    table = _table([[2, 0, 1], [1]], [7, 0xfffffffe])
    # N == 0 (max_frames == 0, no carries): the receive side and fwd are done, pair_off[0] = 0, dst_results as for
    # n == 0, dest_out untouched; the cursors are still clamped
    for dst_sid in ([], core["dst_sid"]):
        c = dict(core, carry=[[], [], [], []], dst_sid=dst_sid, max_frames=0)
        got, m = _run(torch, C, c, 0, [0, 0, 1, NO_GROUP], table)
        assert m["N"] == 0 and got["pair_off"] == [0] and got["dest"] == [] and got["lb_cur"] == [1, 0]
        assert got["results"] == [dict(frames=0, consumed=0, out_bytes=0, error=0)] * 4
        assert (got["out"] == M.SENTINEL).all()
    # max_frames == 0 with carries: the carried messages take their turns and are flushed
    rng = np.random.default_rng(5)
    plain = rng.integers(0, 256, 600, dtype=np.uint8)
    c = _case(core["precoms"], [0, 1], [b"\x00" * 4, b"\x00" * 4], [[], []], [4, 5, 6], 0, core["send"],
              carry=[[(3, 23, MORE), (301, 1, CMD), (400, 1, LAST), (401, 9, LAST), (500, 9, MORE)], [(250, 40, LAST)]],
              plain=plain)
    got, m = _run(torch, C, c, 0, [0, 0], table)
    assert m["N"] == 5 + 1 and got["dest"] == [0, NONE, 0, 1, NONE, 2] and got["lb_cur"] == [1, 0]
    assert (got["plain"] == plain).all() and [r["frames"] for r in got["dst_results"]] == [2, 1, 1]
    # no groups, every stream NO_GROUP: every forwarded part NO_PEER, nothing sent
    got, m = _run(torch, C, c, 0, [NO_GROUP, NO_GROUP], dict(grp_idx=[0], lb_dst=[], lb_cur=[], n_lb=0))
    assert got["dest"] == [NO_PEER, NONE, NO_PEER, NO_PEER, NONE, NO_PEER] and got["lb_cur"] == []
    assert [r["frames"] for r in got["dst_results"]] == [0, 0, 0]
    # n_streams == 0: nothing is done, lb_cur is left alone
    ctx = _ctx(C, core)
    keep = torch.full((16,), -3, dtype=torch.int64, device=dev)
    cur = torch.full((4,), 0x7777, dtype=torch.int32, device=dev)
    a = C.ForwardZmtp(ctypes.sizeof(C.ForwardZmtp), 0)
    a.results, a.fwd, a.pair_off, a.dst_results, a.n_dst, a.max_frames = (C._ptr(keep), C._ptr(keep), C._ptr(keep),
                                                                            C._ptr(keep), 1, 6)
    gi = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    lb = C.ForwardLb(ctypes.sizeof(C.ForwardLb), PREPEND, None, None, 2, None, C._ptr(gi), 2, C._ptr(gi), C._ptr(cur),
                     C._ptr(keep))
    assert C._lib.zmqg_forward_zmtp_lb_multi(ctx._ctx, ctypes.byref(a), ctypes.byref(lb), C._stream_handle(None)) == 0
    torch.cuda.synchronize()
    assert bool((keep == -3).all()) and bool((cur == 0x7777).all())
    ctx.close()
