"""zmqg_forward_zmtp_router_multi: zmqg_forward_zmtp_multi for a proxy with a
ROUTER side, against tests/forward_router_model.py bit for bit.  Compared
everywhere: the receive side's outputs, fwd, pair_off, pair_status, dest_out,
dst_results, every byte of `out` (prefilled with 0xEE) and every session's
peer and send nonce.  The helpers are tests/test_gpu_forward.py's."""
import ctypes
import errno
import functools

import numpy as np
import pytest

from tests import forward_model as F
from tests import forward_router_model as FR
from tests import test_gpu_forward as TF
from tests import zmtp_send_model as M

MORE, CMD, LAST = F.MORE, F.COMMAND, 0
PAD, FILL = TF.PAD, TF.FILL
PREPEND, ROUTE = FR.PREPEND, FR.ROUTE
NONE, ADDRESS, UNKNOWN, MALFORMED = FR.NONE, FR.ADDRESS, FR.UNKNOWN, FR.MALFORMED
WINDOW = 256  # kFwdTopicWin: bytes of an address the route kernel stages (libzmq_amd/csrc/curve_fwd_route.hpp)
DEST_FILL = 0x5B5B5B5B  # what dest_out holds before the call

_rng_bytes, _case, _ctx, _t, _tamper = TF._rng_bytes, TF._case, TF._ctx, TF._t, TF._tamper


def _model(c, flags, src_ids=None, table=None, out_bytes=None, in_place=False):
    """The model's result for case c; out_bytes None: everything fits."""
    args = (c["precoms"], c["down"], c["arena"], c["offs"], c["lens"], c["sids"], c["peer"], -1, c["max_frames"],
            c["carry"], None if in_place else c["plain"], c["dst_sid"], c["routes"], c["send"], flags, src_ids, table)
    total = FR.model(*args, 2 ** 62, 0, encode=False)["enc"]["frame_off"][-1]
    cap = total if out_bytes is None else out_bytes
    m = FR.model(*args, cap, max(total, cap) + PAD)
    m["total"], m["cap"] = total, cap
    return m


def _forward_router(torch, C, c, flags, N, out_bytes, out_size, src_ids=None, table=None, in_place=False, ctx=None,
                    d_plain=None, want_dest=True, no_routes=False):
    """One zmqg_forward_zmtp_router_multi call on a fresh ctx (or `ctx`, which
    stays open).  table: forward_router_model's dict; its arrays may be longer
    than n_ids / bytes_len state.  no_routes: route_idx / route_dst NULL."""
    dev = torch.device("cuda", 0)
    own = ctx is None
    ctx = ctx or _ctx(C, c)
    S, D = len(c["offs"]), len(c["dst_sid"])
    b = TF._recv_buffers(torch, c, in_place, d_plain)
    ci = [0] + [int(x) for x in np.cumsum([len(x) for x in c["carry"]])]
    ri = [0] + [int(x) for x in np.cumsum([len(x) for x in c["routes"]])]
    assert C.CurveContext.forward_router_pair_base(flags, ri, ci, c["max_frames"])[-1] == N
    flat = [e for x in c["carry"] for e in x]
    d_out = torch.full((max(out_size, 1),), M.SENTINEL, dtype=torch.uint8, device=dev)
    d_poff = torch.full((N + 1,), -2, dtype=torch.int64, device=dev)
    d_pst = torch.full((max(N, 1),), -1, dtype=torch.int32, device=dev)
    d_dres = torch.full((max(D, 1), 4), -1, dtype=torch.int64, device=dev)
    d_fwd = torch.full((max(S, 1), 4), -1, dtype=torch.int64, device=dev)
    d_dest = torch.full((max(N, 1),), DEST_FILL, dtype=torch.int32, device=dev) if want_dest else None
    some = lambda a, dt, vt: _t(torch, a if len(a) else np.zeros(1, dt), dt, vt)  # (an empty array still has an address)
    kw = {}
    if src_ids is not None:
        kw.update(src_id_off=_t(torch, [o for o, _ in src_ids], np.uint64, np.int64),
                  src_id_len=_t(torch, [n for _, n in src_ids], np.uint32, np.int32))
    if table is not None:
        kw.update(id_off=some(table["off"], np.uint64, np.int64), id_len=some(table["len"], np.uint32, np.int32),
                  id_dst=some(table["dst"], np.uint32, np.int32),
                  id_bytes=some(np.frombuffer(bytes(table["raw"]), np.uint8).copy(), np.uint8, np.uint8),
                  n_ids=table["n_ids"], id_bytes_len=table["bytes_len"])
    ctx.forward_zmtp_router_multi(
        b["sid"], b["off"], b["len"], b["inp"], -1, c["max_frames"], b["foff"], b["flen"], b["poff"], b["plain"],
        b["fl"], b["st"], b["res"], _t(torch, c["dst_sid"], np.uint32, np.int32) if D else None,
        None if no_routes else ri, None if no_routes else [d for r in c["routes"] for d in r], d_out, d_poff, d_pst,
        d_dres, d_fwd, flags, dest_out=d_dest, carry_idx=ci if flat else None,
        carry_off=_t(torch, [e[0] for e in flat], np.uint64, np.int64) if flat else None,
        carry_len=_t(torch, [e[1] for e in flat], np.uint32, np.int32) if flat else None,
        carry_flags=_t(torch, [e[2] for e in flat], np.uint8, np.uint8) if flat else None, out_bytes=out_bytes, **kw)
    torch.cuda.synchronize()
    got = TF._recv_outputs(C, ctx, b, c)
    got.update(fwd=ctx.forward_results(d_fwd)[:S], pair_off=[int(x) for x in d_poff.cpu().numpy().view(np.uint64)],
               pair_status=[int(x) & 0xffffffff for x in d_pst.cpu().numpy()[:N]],
               dst_results=ctx.zmtp_send_results(d_dres)[:D], out=d_out.cpu().numpy()[:out_size],
               send=[ctx.get_nonce(s) for s in range(len(c["precoms"]))], d_out=d_out, d_plain=b["plain"],
               dest=[int(x) & 0xffffffff for x in d_dest.cpu().numpy()[:N]] if want_dest else None)
    if own:
        ctx.close()
    return got


def _compare(got, m, c):
    TF._compare(got, m, c)
    assert got["dest"] == m["dest"]
    # a pair that is not live: no stream, ZMQG_ERR_SESSION, UINT64_MAX
    for p, d in enumerate(m["dest"]):
        if d >= MALFORMED:
            assert got["pair_status"][p] == M.ERR_SESSION and got["pair_off"][p] == M.UINT64_MAX


def _run(torch, C, c, flags, src_ids=None, table=None, out_bytes=None, **kw):
    """The call against the model; returns (got, m)."""
    m = _model(c, flags, src_ids, table, out_bytes=out_bytes, in_place=kw.get("in_place", False))
    got = _forward_router(torch, C, c, flags, m["N"], m["cap"], m["total"] + PAD, src_ids, table, **kw)
    _compare(got, m, c)
    return got, m


def _park(c, ids, lead=1):
    """The ids behind the arena's span in `plain` (out of place), each at an
    odd offset; sets c["plain"] (keeping what it holds) and returns src_ids."""
    plain = TF._plain_init(c)
    buf, src_ids = bytearray(b"\xA5" * lead), []
    for i in ids:
        if (len(plain) + len(buf)) % 2 == 0:
            buf += b"\x5A"
        src_ids.append((len(plain) + len(buf), len(i)))
        buf += i
    c["plain"] = np.concatenate([plain, np.frombuffer(bytes(buf), np.uint8)])
    return src_ids


def _runs(got):
    return [(r["out_off"], r["out_bytes"]) for r in got["dst_results"]]


# 1 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("in_place", [False, True])
def test_flags_0_equals_the_parent_call(torch_cuda, C, in_place):
    """flags == 0: every output is zmqg_forward_zmtp_multi's on a second ctx
    with the same sessions, and dest_out is not written."""
    c, pm = TF._core(), TF._core_model(in_place)
    got = _forward_router(torch_cuda, C, c, 0, pm["N"], pm["cap"], pm["total"] + PAD, in_place=in_place)
    par = TF._forward(torch_cuda, C, c, pm["N"], pm["cap"], pm["total"] + PAD, in_place=in_place)
    TF._compare(got, pm, c)
    for k in ("results", "peer", "send", "fwd", "pair_off", "pair_status", "dst_results"):
        assert got[k] == par[k], k
    for k in TF.RECV_KEYS + ("out",):
        assert got[k].shape == par[k].shape and (got[k] == par[k]).all(), k
    assert got["dest"] == [DEST_FILL] * pm["N"]


# 2 ------------------------------------------------------------------------------------------------------------------

CORE_IDS = [b"\x00\x00\x00\x00\x07", b"client-B", b"\x00k"]


@functools.lru_cache(maxsize=None)
def _prepend_core():
    """3 sources on sessions 0-2, 3 destinations on sessions 3-5, max_frames 8.
    Routes s0 -> {d0, d1} (fan-out), s1 -> {d2, d2} (one destination twice),
    s2 -> {d1}."""
    rng = np.random.default_rng(6001)
    precoms = [_rng_bytes(rng, 32) for _ in range(6)]
    pay = lambda n: _rng_bytes(rng, n)
    # s0: a single part; a 3-part message with a command between its parts; an empty part; a held tail
    p0 = [(LAST, pay(40)), (MORE, pay(222)), (CMD, pay(9)), (MORE, pay(0)), (LAST, pay(223)), (LAST, b""),
          (MORE, pay(17))]
    # s1: a carried head (in plain) whose message these frames complete; then a single part
    p1 = [(MORE, pay(5)), (LAST, pay(100)), (LAST, pay(1))]
    # s2: a whole message, then a tampered tag inside the next one, valid frames behind it
    p2 = [(MORE, pay(3)), (LAST, pay(64)), (MORE, pay(30)), (LAST, pay(31)), (LAST, pay(8))]
    f2 = F.source_frames(precoms[2], p2)
    f2[3] = _tamper(f2[3])
    streams = [b"".join(F.source_frames(precoms[0], p0)), b"".join(F.source_frames(precoms[1], p1)), b"".join(f2)]
    c = _case(precoms, [0, 1, 2], streams, [[0, 1], [2, 2], [1]], [3, 4, 5], 8, send=[1, 1, 1, 7, 2 ** 32 - 2, 2 ** 40])
    n = len(c["arena"])
    carried = pay(77)
    c["plain"] = np.concatenate([np.full(n, FILL, np.uint8), np.frombuffer(b"\x11" + carried, np.uint8)])
    c["carry"][1] = [(n + 1, 77, MORE)]
    src_ids = _park(c, CORE_IDS)
    return c, src_ids, (p0, p1, p2, carried)


@pytest.mark.gpu
def test_prepend_core(torch_cuda, C):
    """Fan-out, a destination routed twice, a command between parts, a carried
    head completed by this call, a held tail and a failing frame; every run
    decoded by a client ctx is [id, parts ...] per message.  The destination
    routed twice gets every slot twice in slot order, as in the parent call:
    both copies of the id part, then both copies of the head."""
    c, src_ids, (p0, p1, p2, carried) = _prepend_core()
    m = _model(c, PREPEND, src_ids)
    f = m["fwd"]
    assert [x["frames"] for x in m["recv"]["results"]] == [7, 3, 5] and m["recv"]["status"][16 + 3] != 0
    assert (f[0]["held_first"], f[0]["forwarded"], f[0]["failed"]) == (6, 5, 0)
    assert (f[1]["seq"], f[1]["held_first"], f[1]["forwarded"]) == (4, 4, 4)
    assert (f[2]["held_first"], f[2]["forwarded"], f[2]["failed"]) == (2, 2, 1)
    assert m["N"] == 2 * (8 * 2 + 9 * 2 + 8 * 1) and m["base"] == [0, 32, 68, 84]
    got = _forward_router(torch_cuda, C, c, PREPEND, m["N"], m["cap"], m["total"] + PAD, src_ids)
    _compare(got, m, c)
    # without dest_out the same outputs
    again = _forward_router(torch_cuda, C, c, PREPEND, m["N"], m["cap"], m["total"] + PAD, src_ids, want_dest=False)
    assert (again["out"] == got["out"]).all() and again["pair_status"] == got["pair_status"]
    # every destination's run through a client ctx: [id, parts ...] per message
    msgs = TF._peer_decode(torch_cuda, C, c["precoms"], c["dst_sid"], _runs(got), got["d_out"], 24, [TF.PEER0] * 6)
    data = lambda parts: [(fl & MORE, p) for fl, p in parts if not fl & CMD]
    i0, i1, i2 = [(MORE, i) for i in CORE_IDS]
    s0 = [i0] + data(p0[:1]) + [i0] + data(p0[1:5]) + [i0] + data(p0[5:6])
    s2 = [i2] + data(p2[:2])
    assert msgs[0] == s0 and msgs[1] == s0 + s2
    # the id part sits immediately in front of every head; s1 routes d2 twice: every part twice, as in the
    # parent call, the two copies of the id part in front of the two copies of the head
    twice = lambda parts: [x for x in parts for _ in range(2)]
    assert msgs[2] == twice([i1, (MORE, carried)] + data(p1[:2])) + twice([i1] + data(p1[2:]))
    for t in (0, 1):
        heads = [k for k, (fl, _) in enumerate(msgs[t]) if k == 0 or not msgs[t][k - 1][0]]
        assert all(msgs[t][k] in (i0, i2) for k in heads) and len(heads) == (3 if t == 0 else 4)
    # dest_out: a live pair's destination, NONE elsewhere (held, command, failed, past seq, unused id slots)
    live = [d for d in got["dest"] if d != NONE]
    assert sorted(set(live)) == [0, 1, 2] and len(live) == (5 + 3) * 2 + (4 + 2) * 2 + (2 + 1)


# 3 ------------------------------------------------------------------------------------------------------------------

ID_LENS = [0, 1, 5, 255, 300]


@functools.lru_cache(maxsize=None)
def _ids_case(in_place):
    rng = np.random.default_rng(6002)
    precoms = [_rng_bytes(rng, 32) for _ in range(6)]
    ids = [_rng_bytes(rng, n) for n in ID_LENS]
    streams = [b"".join(F.source_frames(precoms[s], [(MORE, _rng_bytes(rng, 9 + s)), (LAST, _rng_bytes(rng, 60))]))
               for s in range(5)]
    if not in_place:
        c = _case(precoms, list(range(5)), streams, [[0]] * 5, [5], 3, send=[1] * 5 + [9])
        return c, _park(c, ids), ids
    # plain == in: the long ids in the gap in front of the first stream, the short ones between the streams
    c = _case(precoms, list(range(5)), streams, [[0]] * 5, [5], 3, send=[1] * 5 + [9], base_off=600)
    gap = lambda s: (c["offs"][s] + c["lens"][s]) | 1  # the first odd offset behind stream s
    src_ids = [(7, 0), (gap(0), 1), (gap(1), 5), (9, 255), (271, 300)]
    for (off, n), i in zip(src_ids, ids):
        assert off % 2 == 1 and all(off + n <= o or off >= o + ln for o, ln in zip(c["offs"], c["lens"]))
        c["arena"][off:off + n] = np.frombuffer(i, np.uint8)
    return c, src_ids, ids


@pytest.mark.gpu
@pytest.mark.parametrize("in_place", [False, True])
def test_prepend_ids(torch_cuda, C, in_place):
    """Ids of 0, 1, 5, 255 and 300 bytes at odd offsets; with plain == in they
    are parked in the gaps between the streams."""
    c, src_ids, ids = _ids_case(in_place)
    assert all(off % 2 == 1 for off, _ in src_ids)
    got, m = _run(torch_cuda, C, c, PREPEND, src_ids, in_place=in_place)
    assert [f["forwarded"] for f in m["fwd"]] == [2] * 5 and m["N"] == 2 * 3 * 5
    msgs = TF._peer_decode(torch_cuda, C, c["precoms"], c["dst_sid"], _runs(got), got["d_out"], 16, [TF.PEER0] * 6)[0]
    assert [p for fl, p in msgs[0::3]] == ids and all(fl == MORE for fl, _ in msgs[0::3]) and len(msgs) == 15


# 4 ------------------------------------------------------------------------------------------------------------------

ROUTE_PEERS = [(b"alpha", 0), (b"bravo", 1), (b"charlie", 0), (b"delta", 7), (b"echo", 2), (b"zulu", 3)]


@functools.lru_cache(maxsize=None)
def _route_core():
    """3 sources on sessions 0-2; destinations d0, d1, d3 on sessions 3-5 and
    d2 on a session the ctx has not (99).  "alpha" and "charlie" name d0,
    "delta" names destination 7 of 4."""
    rng = np.random.default_rng(6004)
    precoms = [_rng_bytes(rng, 32) for _ in range(6)]
    pay = lambda n: _rng_bytes(rng, n)
    msg = lambda addr, *lens: [(MORE, addr)] + [(MORE, pay(n)) for n in lens[:-1]] + [(LAST, pay(lens[-1]))]
    p0 = (msg(b"alpha", 40)                                   # the first table entry
          + [(MORE, b"charlie"), (MORE, pay(222)), (CMD, pay(3)), (LAST, pay(1))]  # a middle one, a command inside
          + msg(b"zulu", 0, 223)                              # the last one
          + msg(b"nobody", 12)                                # unknown
          + msg(b"alph", 13)                                  # a strict prefix of an id
          + msg(b"alphax", 14)                                # an id and one byte
          + msg(b"", 15)                                      # the empty address
          + [(LAST, b"bravo")]                                # a one-part message
          + msg(b"delta", 16)                                 # id_dst >= n_dst
          + msg(b"echo", 17))                                 # the destination without a session
    # s1: its address part is carried; then a message with a known address and an open tail
    p1 = [(LAST, pay(50)), (MORE, b"alpha"), (MORE, pay(20))]
    # s2: a whole message, then a failing frame inside the next one
    p2 = msg(b"zulu", 5) + msg(b"bravo", 6, 7)
    f2 = F.source_frames(precoms[2], p2)
    f2[3] = _tamper(f2[3])
    streams = [b"".join(F.source_frames(precoms[0], p0)), b"".join(F.source_frames(precoms[1], p1)), b"".join(f2)]
    c = _case(precoms, [0, 1, 2], streams, [[], [], []], [3, 4, 99, 5], 22, send=[1, 1, 1, 7, 2 ** 32 - 2, 2 ** 40])
    n = len(c["arena"])
    c["plain"] = np.concatenate([np.full(n, FILL, np.uint8), np.frombuffer(b"\x11bravo", np.uint8)])
    c["carry"][1] = [(n + 1, 5, MORE)]
    return c, p0


@pytest.mark.gpu
@pytest.mark.parametrize("with_empty", [False, True])
def test_route_core(torch_cuda, C, with_empty):
    c, p0 = _route_core()
    table = FR.table_of(ROUTE_PEERS + ([(b"", 1)] if with_empty else []))
    assert len(p0) == 22 and FR.entry(table, 0) == (b"" if with_empty else b"alpha")
    got, m = _run(torch_cuda, C, c, ROUTE, None, table, no_routes=True)
    assert m["N"] == 22 + 23 + 22 and m["base"] == [0, 22, 45, 67]
    d0 = got["dest"][:22]
    assert d0[:12] == [ADDRESS, 0, ADDRESS, 0, NONE, 0, ADDRESS, 3, 3, ADDRESS, UNKNOWN, ADDRESS]
    assert d0[12:] == [UNKNOWN, ADDRESS, UNKNOWN, ADDRESS, 1 if with_empty else UNKNOWN, MALFORMED, ADDRESS, UNKNOWN,
                       ADDRESS, 2]
    # "echo" names d2, whose session the ctx has not: the pair is live for dest_out, the encode reports the session
    p_echo = 21
    assert m["pairs"][p_echo][3] and got["dest"][p_echo] == 2 and got["pair_status"][p_echo] == M.ERR_SESSION
    assert got["dst_results"][2]["error"] == errno.EINVAL and got["dst_results"][2]["frames"] == 0
    # s1: the carried address "bravo" sends the first frame to d1; the open message is held whole
    assert got["dest"][22:45] == [ADDRESS, 1] + [NONE] * 21 and got["fwd"][1]["held_first"] == 2
    # s2: the message before the failing frame goes out, nothing behind it
    assert got["dest"][45:] == [ADDRESS, 3] + [NONE] * 20 and got["fwd"][2]["failed"] == 1
    assert [r["frames"] for r in got["dst_results"]] == [3, 2 if with_empty else 1, 0, 3]
    # route_idx / route_dst are not read: with arbitrary routes the same outputs
    again = _forward_router(torch_cuda, C, dict(c, routes=[[1, 2], [], [0]]), ROUTE, m["N"], m["cap"],
                            m["total"] + PAD, None, table)
    assert again["dest"] == got["dest"] and (again["out"] == got["out"]).all() and again["send"] == got["send"]


# 5 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_route_addresses_past_the_window(torch_cuda, C):
    """Ids of 256, 257 and 300 bytes, three of each length that differ only in
    the last byte: the deciding byte is the window's last one, the first one
    past it, and 44 bytes past it (read from global memory)."""
    rng = np.random.default_rng(6005)
    precoms = [_rng_bytes(rng, 32) for _ in range(5)]
    stem = _rng_bytes(rng, 299)
    ids = {stem[:n - 1] + bytes([last]): (n + last) % 3 for n in (256, 257, 300) for last in (0x10, 0x20, 0x30)}
    assert max(len(i) for i in ids) > WINDOW
    probes = [stem[:n - 1] + bytes([last]) for n in (256, 257, 300) for last in (0x20, 0x21, 0x10, 0x30)]
    parts = [x for a in probes for x in ((MORE, a), (LAST, _rng_bytes(rng, 4)))]
    half = len(parts) // 2
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in enumerate((parts[:half], parts[half:]))]
    c = _case(precoms, [0, 1], streams, [[], []], [2, 3, 4], half, send=[1] * 5)
    got, m = _run(torch_cuda, C, c, ROUTE, None, FR.table_of(ids.items()))
    want = [x for a in probes for x in (ADDRESS, ids.get(a, UNKNOWN))]
    assert got["dest"] == want and want.count(UNKNOWN) == 3


# 6 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n_ids", [0, 1, 2, 63, 64, 65, 1000])
def test_route_table_widths(torch_cuda, C, n_ids):
    """Ids in the reference's auto-generated form (a 0 byte, then BE32); the
    first, the last, a middle one and one that is absent."""
    rng = np.random.default_rng(6006)
    precoms = [_rng_bytes(rng, 32) for _ in range(4)]
    rid = lambda i: b"\x00" + int(3 + 7 * i).to_bytes(4, "big")
    ids = {rid(i): i % 3 for i in range(n_ids)}
    probes = [rid(0), rid(max(n_ids - 1, 0)), rid(n_ids // 2), rid(n_ids // 2)[:-1] + b"\x01", rid(n_ids)]
    parts = [x for a in probes for x in ((MORE, a), (LAST, _rng_bytes(rng, 33)))]
    c = _case(precoms, [0], [b"".join(F.source_frames(precoms[0], parts))], [[]], [1, 2, 3], 10, send=[1] * 4)
    got, m = _run(torch_cuda, C, c, ROUTE, None, FR.table_of(ids.items()))
    want = [x for a in probes for x in (ADDRESS, ids.get(a, UNKNOWN))]
    assert got["dest"] == want
    assert want.count(UNKNOWN) == (5 if n_ids == 0 else 2)


# 7 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_untrusted_table(torch_cuda, C):
    """Void entries (an offset past id_bytes_len, a length past it, off + len
    overflowing 64 bits), an unsorted table, duplicate ids, and arrays longer
    than n_ids / id_bytes_len whose bytes behind the stated extents hold ids
    that would match.  The model runs the header's loop: the outputs agree."""
    rng = np.random.default_rng(6007)
    precoms = [_rng_bytes(rng, 32) for _ in range(3)]
    stated = b"\x00" + b"aaa" + b"ccc" + b"ccc" + b"bbb" + b"eee" + b"yyy" + b"zz"
    raw = stated + b"z" + b"qqq"
    L = len(stated)
    # a void entry orders as the empty id, so a host that sorts puts them first: 0 (its offset is past
    # id_bytes_len) and 1 (off + len wraps); then "aaa", "ccc", "ccc" again, "bbb" out of order, "eee", and 7, whose
    # length runs one byte past id_bytes_len ("zzz" if read); entry 8, behind n_ids, is "yyy"
    off = [L + 1, 2 ** 64 - 1, 1, 4, 7, 10, 13, L - 2, 16]
    ln = [0, 2, 3, 3, 3, 3, 3, 3, 3]
    dst = [0, 1, 0, 1, 0, 1, 1, 0, 1]
    table = dict(off=off, len=ln, dst=dst, raw=raw, n_ids=8, bytes_len=L)
    assert [FR.entry(table, j) for j in range(8)] == [None, None, b"aaa", b"ccc", b"ccc", b"bbb", b"eee", None]
    assert raw[L - 2:L + 1] == b"zzz" and raw[16:19] == b"yyy"
    probes = [b"aaa", b"bbb", b"ccc", b"eee", b"zzz", b"yyy", b"", b"ddd"]
    parts = [x for a in probes for x in ((MORE, a), (LAST, _rng_bytes(rng, 10)))]
    c = _case(precoms, [0], [b"".join(F.source_frames(precoms[0], parts))], [[]], [1, 2], 16, send=[1] * 3)
    got, m = _run(torch_cuda, C, c, ROUTE, None, table)
    # "bbb" is lost to the order, the first "ccc" answers, nothing behind either extent is seen, and a void entry
    # does not equal the empty address
    assert got["dest"][1::2] == [0, UNKNOWN, 1, 1, UNKNOWN, UNKNOWN, UNKNOWN, UNKNOWN]


# 8 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("in_place", [False, True])
def test_route_and_prepend(torch_cuda, C, in_place):
    """A ROUTER to ROUTER proxy: every source's messages go whole to the
    destination whose id equals the source's id; a source whose id the table
    has not is dropped (UNKNOWN)."""
    rng = np.random.default_rng(6008)
    precoms = [_rng_bytes(rng, 32) for _ in range(5)]
    ids = [b"one", b"nobody", b"two"]
    parts = [[(MORE, _rng_bytes(rng, 30)), (CMD, b"x"), (LAST, _rng_bytes(rng, 1)), (LAST, _rng_bytes(rng, 200)),
              (MORE, b"held")] for _ in range(3)]
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in enumerate(parts)]
    c = _case(precoms, [0, 1, 2], streams, [[], [], []], [3, 4], 5, send=[1, 1, 1, 7, 9], base_off=64 if in_place else 0)
    if in_place:
        src_ids = [(1, 3), (5, 6), (13, 3)]
        c["arena"][1:16] = np.frombuffer(b"one\x00nobody\x00\x00two", np.uint8)
    else:
        src_ids = _park(c, ids)
    got, m = _run(torch_cuda, C, c, ROUTE | PREPEND, src_ids, FR.table_of([(b"one", 1), (b"two", 0)]),
                  in_place=in_place, no_routes=True)
    assert m["N"] == 15
    assert got["dest"] == [1, NONE, 1, 1, NONE] + [UNKNOWN, NONE, UNKNOWN, UNKNOWN, NONE] + [0, NONE, 0, 0, NONE]
    msgs = TF._peer_decode(torch_cuda, C, c["precoms"], c["dst_sid"], _runs(got), got["d_out"], 8, [TF.PEER0] * 5)
    whole = lambda p: [(fl & MORE, d) for fl, d in p[:4] if not fl & CMD]
    assert msgs == [whole(parts[2]), whole(parts[0])]


# 9 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("flags", [PREPEND, ROUTE])
def test_fit(torch_cuda, C, flags):
    """out_bytes cuts the destination's run in the middle of a message: after
    an id part (PREPEND), after a first payload part (ROUTE).  The fitting
    frames are a prefix, the rest ZMQG_ERR_BOUND with no nonce taken, the
    destination ENOBUFS, nothing at or past out_bytes."""
    rng = np.random.default_rng(6009)
    precoms = [_rng_bytes(rng, 32) for _ in range(3)]
    body = [(MORE, _rng_bytes(rng, 100)), (LAST, _rng_bytes(rng, 50))]
    parts = [(LAST, _rng_bytes(rng, 10))] + body if flags == PREPEND else \
        [(MORE, b"w"), (LAST, _rng_bytes(rng, 10)), (MORE, b"w")] + body
    c = _case(precoms, [0], [b"".join(F.source_frames(precoms[0], parts))], [[0]], [1], 6, send=[1, 2 ** 32 - 2, 5])
    src_ids = _park(c, [b"\x00\x00\x00\x00\x09"]) if flags == PREPEND else None
    table = FR.table_of([(b"w", 0)]) if flags == ROUTE else None
    full = _model(c, flags, src_ids, table)
    live = [p for p, pr in enumerate(full["pairs"]) if pr[3]]
    assert len(live) == (5 if flags == PREPEND else 3)
    # PREPEND: [id, a] [id, b1 | b2]: the cut falls after the second id part.  ROUTE: [a] [b1 | b2]: after b1.
    first_out = live[3] if flags == PREPEND else live[2]
    cap = full["enc"]["frame_off"][first_out] + 7
    got, m = _run(torch_cuda, C, c, flags, src_ids, table, out_bytes=cap)
    fit = 3 if flags == PREPEND else 2
    R = got["dst_results"][0]
    assert (R["frames"], R["error"]) == (fit, errno.ENOBUFS)
    assert [got["pair_status"][p] for p in live] == [0] * fit + [C.ERR_BOUND] * (len(live) - fit)
    assert got["send"] == [1, 2 ** 32 - 2 + fit, 5]
    assert got["pair_off"] == full["enc"]["frame_off"] and got["dest"] == full["dest"]
    assert (got["out"][cap:] == M.SENTINEL).all()


# 10 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_request_reply_loop(torch_cuda, C):
    """Two calls on one ctx: a client's request goes through PREPEND to a
    worker, which sees [id, parts]; its reply [id, payload], sealed as that
    peer seals, comes back through ROUTE; the client decodes exactly the
    payload parts.  The nonces continue across the calls."""
    torch = torch_cuda
    rng = np.random.default_rng(6010)
    precoms = [_rng_bytes(rng, 32) for _ in range(2)]  # session 0: the client, 1: the worker
    cid = b"\x00\x00\x00\x10\x01"
    request = [(MORE, b""), (LAST, _rng_bytes(rng, 120))]
    reply = [(MORE, b""), (MORE, _rng_bytes(rng, 64)), (LAST, _rng_bytes(rng, 3))]
    c1 = _case(precoms, [0], [b"".join(F.source_frames(precoms[0], request))], [[0]], [1], 3, send=[40, 50])
    L1 = len(c1["arena"])
    fr = F.source_frames(precoms[1], [(MORE, cid)] + reply)
    c2 = _case(precoms, [1], [b"".join(fr)], [[]], [0], 5, send=[0, 0], base_off=L1)
    L2 = len(c2["arena"])
    plain = np.full(L2 + 8, FILL, np.uint8)
    plain[L2 + 1:L2 + 6] = np.frombuffer(cid, np.uint8)
    c1["plain"] = plain.copy()
    src_ids = [(L2 + 1, 5)]
    m1 = _model(c1, PREPEND, src_ids)
    c2.update(send=m1["enc"]["send"], peer=m1["recv"]["peer"], plain=plain.copy())
    table = FR.table_of([(cid, 0)])
    m2 = _model(c2, ROUTE, None, table)
    ctx = _ctx(C, c1)
    d_plain = torch.from_numpy(plain.copy()).to(torch.device("cuda", 0))
    g1 = _forward_router(torch, C, c1, PREPEND, m1["N"], m1["cap"], m1["total"] + PAD, src_ids, ctx=ctx,
                         d_plain=d_plain)
    _compare(g1, m1, c1)
    g2 = _forward_router(torch, C, c2, ROUTE, m2["N"], m2["cap"], m2["total"] + PAD, None, table, ctx=ctx,
                         d_plain=d_plain, no_routes=True)
    ctx.close()
    _compare(g2, m2, c2)
    seen = TF._peer_decode(torch, C, precoms, [1], _runs(g1), g1["d_out"], 8, [TF.PEER0] * 2)[0]
    assert seen == [(MORE, cid)] + request
    back = TF._peer_decode(torch, C, precoms, [0], _runs(g2), g2["d_out"], 8, [TF.PEER0] * 2)[0]
    assert back == reply
    assert g2["dest"] == [ADDRESS, 0, 0, 0, NONE]
    # session 0 received 2 frames and sent 3, session 1 sent 3 and received 4
    assert g2["send"] == [40 + 3, 50 + 3] and g1["send"] == [40, 53]
    assert g2["peer"] == [g1["peer"][0], m2["recv"]["peer"][1]] and g1["peer"][0] > TF.PEER0 < g2["peer"][1]


# 11 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_einval(torch_cuda, C):
    """Every -EINVAL case of the header, the parent call's included, with nothing queued."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    core = TF._core()
    ctx = _ctx(C, core)
    big = C.CurveContext(0, 8193)
    z32 = torch.zeros(64, dtype=torch.int32, device=dev)
    z64 = torch.zeros(64, dtype=torch.int64, device=dev)
    buf = torch.full((256,), M.SENTINEL, dtype=torch.uint8, device=dev)
    res = torch.full((16, 4), -1, dtype=torch.int64, device=dev)
    dout = torch.full((64,), DEST_FILL, dtype=torch.int32, device=dev)
    ri = np.array([0, 1, 2], np.uint32)
    rd = np.array([0, 1], np.uint32)
    ci = np.array([0, 1, 1], np.uint32)
    keepalive = []
    RT_KEYS = ("rt_size", "flags", "src_id_off", "src_id_len", "n_ids", "id_off", "id_len", "id_dst", "id_bytes",
               "id_bytes_len", "dest_out")

    def call(flags, c=ctx._ctx, null_args=False, null_router=False, **kw):
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
        rt = C.ForwardRouter(ctypes.sizeof(C.ForwardRouter), flags, C._ptr(z64), C._ptr(z32), 2, C._ptr(z64),
                             C._ptr(z32), C._ptr(z32), C._ptr(buf), 16, C._ptr(dout))
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                keepalive.append(v)
                v = v.ctypes.data
            if k in RT_KEYS:
                setattr(rt, "size" if k == "rt_size" else k, v)
            else:
                setattr(a, k, v)
        return C._lib.zmqg_forward_zmtp_router_multi(c, None if null_args else ctypes.byref(a),
                                                     None if null_router else ctypes.byref(rt),
                                                     C._stream_handle(None))

    u32 = lambda *x: np.array(x, np.uint32)
    E = -errno.EINVAL
    BOTH = PREPEND | ROUTE
    # the router struct's cases
    for fl in (0, PREPEND, ROUTE, BOTH):
        assert call(fl, null_router=True) == E
        assert call(fl, rt_size=ctypes.sizeof(C.ForwardRouter) - 8) == E and call(fl, rt_size=0) == E
    assert call(4) == E and call(PREPEND | 4) == E and call(2 ** 31) == E
    for fl in (PREPEND, BOTH):
        assert call(fl, src_id_off=None) == E and call(fl, src_id_len=None) == E
    for fl in (ROUTE, BOTH):
        assert call(fl, n_ids=2 ** 31) == E
        assert call(fl, id_off=None) == E and call(fl, id_len=None) == E and call(fl, id_dst=None) == E
        assert call(fl, id_bytes=None) == E
        assert call(fl, n_dst=0) == E  # frames and no streams
    # the parent call's, under every flag combination
    for fl in (0, PREPEND, ROUTE, BOTH):
        assert call(fl, c=None) == E and call(fl, null_args=True) == E
        assert call(fl, size=ctypes.sizeof(C.ForwardZmtp) - 8) == E and call(fl, reserved=1) == E
        assert call(fl, results=None) == E and call(fl, max_frames=2 ** 31) == E and call(fl, n_streams=2 ** 31) == E
        assert call(fl, n_streams=2 ** 16, max_frames=2 ** 15) == E
        for k in ("stream_sid", "stream_off", "stream_len", "inp", "frame_in_off", "frame_len", "plain_off", "plain",
                  "flags_out", "status_out"):
            assert call(fl, **{k: None}) == E, k
        assert call(fl, n_dst=8193) == E and call(fl, c=big._ctx) == E
        assert call(fl, dst_sid=None) == E and call(fl, dst_results=None) == E and call(fl, pair_off=None) == E
        assert call(fl, out=None) == E and call(fl, fwd=None) == E
        assert call(fl, carry_idx=u32(0, 2, 1)) == E and call(fl, carry_idx=u32(1, 1, 1)) == E
        assert call(fl, carry_off=None) == E and call(fl, carry_len=None) == E and call(fl, carry_flags=None) == E
    # the route_idx / route_dst cases: skipped under ROUTE alone
    for fl in (0, PREPEND):
        assert call(fl, route_idx=None) == E and call(fl, route_idx=u32(1, 1, 2)) == E
        assert call(fl, route_idx=u32(0, 2, 1)) == E
        assert call(fl, route_dst=u32(0, 2)) == E and call(fl, route_dst=None) == E
        assert call(fl, n_streams=1, max_frames=2 ** 30, route_idx=u32(0, 2), carry_idx=None) == E
        assert call(fl, n_streams=1, max_frames=2 ** 31 - 1, route_idx=u32(0, 2 ** 32 - 1), carry_idx=None) == E
    # N as the router pair space counts it: PREPEND alone doubles the slots; ROUTE has one route slot a stream
    assert call(PREPEND, n_streams=1, max_frames=2 ** 30, route_idx=u32(0, 1), carry_idx=None) == E
    assert call(ROUTE, n_streams=2, max_frames=2 ** 30, carry_idx=None) == E
    torch.cuda.synchronize()
    assert bool((res == -1).all()) and bool((buf == M.SENTINEL).all()) and bool((z64 == 0).all())
    assert bool((dout == DEST_FILL).all()) and bool((z32 == 0).all())
    # what is no error (with outputs of their own): the arguments the cases above start from, under every flag; a
    # null table with nothing in it, a null dest_out; null routes under ROUTE
    o64 = [torch.zeros(64, dtype=torch.int64, device=dev) for _ in range(3)]
    o32 = [torch.zeros(64, dtype=torch.int32, device=dev) for _ in range(3)]
    o8 = [torch.zeros(256, dtype=torch.uint8, device=dev) for _ in range(3)]
    own = dict(frame_in_off=C._ptr(o64[0]), plain_off=C._ptr(o64[1]), pair_off=C._ptr(o64[2]),
               frame_len=C._ptr(o32[0]), status_out=C._ptr(o32[1]), pair_status=C._ptr(o32[2]), plain=C._ptr(o8[0]),
               flags_out=C._ptr(o8[1]), out=C._ptr(o8[2]), results=C._ptr(o64[0][32:]),
               dst_results=C._ptr(o64[1][32:]))
    for fl in (0, PREPEND, ROUTE, BOTH):
        assert call(fl, **own) == 0
    assert call(ROUTE, route_idx=None, route_dst=None, **own) == 0
    assert call(BOTH, route_idx=u32(7, 1, 0), route_dst=u32(9, 9), **own) == 0
    assert call(ROUTE, n_ids=0, id_off=None, id_len=None, id_dst=None, id_bytes=None, id_bytes_len=0, dest_out=None,
                **own) == 0
    assert call(0, src_id_off=None, src_id_len=None, n_ids=2 ** 31, id_off=None, **own) == 0  # flags 0: nothing is read
    torch.cuda.synchronize()
    assert ctx.forward_results(res[:2]) == [dict(seq=1, held_first=0, forwarded=0, failed=0),
                                            dict(seq=0, held_first=0, forwarded=0, failed=0)]
    # N = (1 + 3) + 3 pairs, twice as many under PREPEND alone, none live; nothing behind them is written
    assert bool((dout[:14] == -1).all()) and bool((dout[14:] == DEST_FILL).all())
    ctx.close()
    big.close()


# 12 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_edges(torch_cuda, C):
    """N == 0 and n_dst == 0: as the parent call states."""
    torch = torch_cuda
    core = TF._core()
    ids = [(1, 2)] * 4
    # N == 0 under PREPEND (no routes at all): the receive side and fwd are done, pair_off[0] = 0, dst_results as
    # for n == 0, dest_out untouched
    c = dict(core, routes=[[], [], [], []])
    got, m = _run(torch, C, c, PREPEND, ids)
    assert m["N"] == 0 and got["pair_off"] == [0] and got["dest"] == []
    assert got["dst_results"] == [dict(frames=0, out_off=0, out_bytes=0, error=0)] * 3
    assert got["fwd"][0]["forwarded"] == 3 and (got["out"] == M.SENTINEL).all()
    # n_dst == 0, N == 0
    c = dict(core, routes=[[], [], [], []], dst_sid=[])
    got, m = _run(torch, C, c, PREPEND, ids)
    assert m["N"] == 0 and got["pair_off"] == [0] and got["fwd"][0]["forwarded"] == 3
    # N == 0 under ROUTE: max_frames == 0 and no carries (with or without destinations)
    for dst_sid in ([], core["dst_sid"]):
        c = dict(core, routes=[[], [], [], []], dst_sid=dst_sid, max_frames=0)
        got, m = _run(torch, C, c, ROUTE, None, FR.table_of([(b"a", 0)]), no_routes=True)
        assert m["N"] == 0 and got["pair_off"] == [0]
        assert got["results"] == [dict(frames=0, consumed=0, out_bytes=0, error=0)] * 4
    # max_frames == 0 with carries under ROUTE: the carried address is looked up, the carried parts flushed
    rng = np.random.default_rng(5)
    plain = rng.integers(0, 256, 600, dtype=np.uint8)
    plain[3:6] = (65, 66, 67)
    c = _case(core["precoms"], [0, 1], [b"\x00" * 4, b"\x00" * 4], [[], []], [4, 5], 0, core["send"],
              carry=[[(3, 3, MORE), (301, 0, CMD), (400, 1, MORE), (401, 9, LAST), (500, 9, MORE)], [(250, 40, LAST)]],
              plain=plain)
    got, m = _run(torch, C, c, ROUTE, None, FR.table_of([(b"ABC", 1)]), no_routes=True)
    assert m["N"] == 5 + 1 and got["dest"] == [ADDRESS, NONE, 1, 1, NONE, MALFORMED]
    assert (got["plain"] == plain).all() and got["dst_results"][1]["frames"] == 2
    # n_streams == 0: nothing is done
    ctx = _ctx(C, core)
    dev = torch.device("cuda", 0)
    keep = torch.full((16,), -3, dtype=torch.int64, device=dev)
    a = C.ForwardZmtp(ctypes.sizeof(C.ForwardZmtp), 0)
    a.results, a.fwd, a.pair_off, a.dst_results, a.n_dst, a.max_frames = (C._ptr(keep), C._ptr(keep), C._ptr(keep),
                                                                            C._ptr(keep), 1, 6)
    rt = C.ForwardRouter(ctypes.sizeof(C.ForwardRouter), PREPEND | ROUTE, None, None, 0, None, None, None, None, 0,
                         C._ptr(keep))
    assert C._lib.zmqg_forward_zmtp_router_multi(ctx._ctx, ctypes.byref(a), ctypes.byref(rt),
                                                 C._stream_handle(None)) == 0
    torch.cuda.synchronize()
    assert bool((keep == -3).all())
    ctx.close()
