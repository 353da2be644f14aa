"""zmqg_forward_zmtp_multi: many connections' receive buffers decoded, the whole
messages picked on the device and re-encoded for their destinations in one
call, against tests/forward_model.py bit for bit.  Compared everywhere: the
receive side's outputs (also against zmqg_decode_zmtp_multi itself, run on a
second ctx with the same sessions), fwd, pair_off, pair_status, dst_results,
every byte of `out` (prefilled with 0xEE: what no fitting frame covers keeps
it) and every session's peer and send nonce."""
import ctypes
import errno
import functools

import numpy as np
import pytest

from oracle import zmtp_oracle as Z
from tests import forward_model as F
from tests import zmtp_send_model as M

MORE, CMD, LAST = F.MORE, F.COMMAND, 0
PEER0 = 2      # every session's peer nonce before the first call
PAD = 64       # bytes of `out` behind its capacity
FILL = 0x77    # what `plain` holds where nothing was decoded


def _rng_bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _case(precoms, sids, streams, routes, dst_sid, max_frames, send, carry=None, plain=None, peer=None, base_off=0):
    """One call's inputs.  base_off: bytes in front of the arena (a later
    call's receive buffers lie behind an earlier call's in `plain`)."""
    arena, offs = F.arena_of(streams)
    if base_off:
        arena = np.concatenate([np.full(base_off, 0x5A, np.uint8), arena])
        offs = [o + base_off for o in offs]
    return dict(precoms=precoms, down=[False] * len(precoms), sids=sids, arena=arena, offs=offs,
                lens=[len(s) for s in streams], routes=routes, dst_sid=dst_sid, max_frames=max_frames,
                send=list(send), peer=list(peer) if peer else [PEER0] * len(precoms),
                carry=carry or [[] for _ in streams], plain=plain)


def _model(c, out_bytes=None, in_place=False):
    """The model's result for case c; out_bytes None: everything fits."""
    args = (c["precoms"], c["down"], c["arena"], c["offs"], c["lens"], c["sids"], c["peer"], -1, c["max_frames"],
            c["carry"], None if in_place else c["plain"], c["dst_sid"], c["routes"], c["send"])
    total = F.model(*args, 2 ** 62, 0, encode=False)["enc"]["frame_off"][-1]
    cap = total if out_bytes is None else out_bytes
    m = F.model(*args, cap, max(total, cap) + PAD)
    m["total"], m["cap"] = total, cap
    return m


def _ctx(C, c, n_sessions=None):
    ctx = C.CurveContext(0, n_sessions or len(c["precoms"]))
    for s, p in enumerate(c["precoms"]):
        ctx.session_set(s, p, C.SERVER_PREFIX, C.CLIENT_PREFIX, c["down"][s], c["peer"][s])
        ctx.set_nonce(s, c["send"][s])
    return ctx


def _t(torch, a, dt, vt):
    return torch.from_numpy(np.ascontiguousarray(a, dt).view(vt)).to(torch.device("cuda", 0))


def _plain_init(c):
    """`plain` before the call: FILL over the arena's span, or the case's own bytes (its carried payloads)."""
    return np.full(len(c["arena"]), FILL, np.uint8) if c["plain"] is None else c["plain"].copy()


def _recv_buffers(torch, c, in_place, d_plain=None):
    dev = torch.device("cuda", 0)
    S, slots = len(c["offs"]), max(len(c["offs"]) * c["max_frames"], 1)
    d_in = torch.from_numpy(c["arena"].copy()).to(dev)
    if d_plain is None:
        d_plain = d_in if in_place else torch.from_numpy(_plain_init(c)).to(dev)
    return dict(sid=_t(torch, c["sids"], np.uint32, np.int32), off=_t(torch, c["offs"], np.uint64, np.int64),
                len=_t(torch, c["lens"], np.uint32, np.int32), inp=d_in, plain=d_plain,
                foff=torch.full((slots,), -1, dtype=torch.int64, device=dev),
                flen=torch.full((slots,), -1, dtype=torch.int32, device=dev),
                poff=torch.full((slots,), -1, dtype=torch.int64, device=dev),
                fl=torch.full((slots,), 0xEE, dtype=torch.uint8, device=dev),
                st=torch.full((slots,), -1, dtype=torch.int32, device=dev),
                res=torch.full((max(S, 1), 4), -1, dtype=torch.int64, device=dev))


def _recv_outputs(C, ctx, b, c):
    slots = len(c["offs"]) * c["max_frames"]
    return dict(results=ctx.zmtp_results(b["res"])[:len(c["offs"])], f_off=b["foff"].cpu().numpy().view(np.uint64)[:slots],
                f_len=b["flen"].cpu().numpy().view(np.uint32)[:slots],
                plain_off=b["poff"].cpu().numpy().view(np.uint64)[:slots], flags=b["fl"].cpu().numpy()[:slots],
                status=(b["st"].cpu().numpy().astype(np.int64) & 0xffffffff)[:slots], plain=b["plain"].cpu().numpy(),
                peer=[ctx.get_peer_nonce(s) for s in range(len(c["precoms"]))])


def _forward(torch, C, c, N, out_bytes, out_size, in_place=False, ctx=None, d_plain=None):
    """One zmqg_forward_zmtp_multi call on a fresh ctx (or `ctx`, which stays open)."""
    dev = torch.device("cuda", 0)
    own = ctx is None
    ctx = ctx or _ctx(C, c)
    S, D = len(c["offs"]), len(c["dst_sid"])
    b = _recv_buffers(torch, c, in_place, d_plain)
    ci = [0] + [int(x) for x in np.cumsum([len(x) for x in c["carry"]])]
    ri = [0] + [int(x) for x in np.cumsum([len(x) for x in c["routes"]])]
    assert C.CurveContext.forward_pair_base(ri, ci, c["max_frames"])[-1] == N
    flat = [e for x in c["carry"] for e in x]
    d_out = torch.full((max(out_size, 1),), M.SENTINEL, dtype=torch.uint8, device=dev)
    d_poff = torch.full((N + 1,), -2, dtype=torch.int64, device=dev)
    d_pst = torch.full((max(N, 1),), -1, dtype=torch.int32, device=dev)
    d_dres = torch.full((max(D, 1), 4), -1, dtype=torch.int64, device=dev)
    d_fwd = torch.full((max(S, 1), 4), -1, dtype=torch.int64, device=dev)
    ctx.forward_zmtp_multi(b["sid"], b["off"], b["len"], b["inp"], -1, c["max_frames"], b["foff"], b["flen"], b["poff"],
                           b["plain"], b["fl"], b["st"], b["res"], _t(torch, c["dst_sid"], np.uint32, np.int32), ri,
                           [d for r in c["routes"] for d in r], d_out, d_poff, d_pst, d_dres, d_fwd,
                           carry_idx=ci if flat else None,
                           carry_off=_t(torch, [e[0] for e in flat], np.uint64, np.int64) if flat else None,
                           carry_len=_t(torch, [e[1] for e in flat], np.uint32, np.int32) if flat else None,
                           carry_flags=_t(torch, [e[2] for e in flat], np.uint8, np.uint8) if flat else None,
                           out_bytes=out_bytes)
    torch.cuda.synchronize()
    got = _recv_outputs(C, ctx, b, c)
    got.update(fwd=ctx.forward_results(d_fwd)[:S], pair_off=[int(x) for x in d_poff.cpu().numpy().view(np.uint64)],
               pair_status=[int(x) & 0xffffffff for x in d_pst.cpu().numpy()[:N]],
               dst_results=ctx.zmtp_send_results(d_dres)[:D], out=d_out.cpu().numpy()[:out_size],
               send=[ctx.get_nonce(s) for s in range(len(c["precoms"]))], d_out=d_out, d_plain=b["plain"])
    if own:
        ctx.close()
    return got


def _decode_only(torch, C, c, in_place=False):
    """zmqg_decode_zmtp_multi on a ctx of its own with the same sessions and arguments."""
    ctx = _ctx(C, c)
    b = _recv_buffers(torch, c, in_place)
    ctx.decode_zmtp_multi(b["sid"], b["off"], b["len"], b["inp"], -1, c["max_frames"], b["foff"], b["flen"], b["poff"],
                          b["plain"], b["fl"], b["st"], b["res"])
    torch.cuda.synchronize()
    got = _recv_outputs(C, ctx, b, c)
    got["ctx"], got["b"] = ctx, b
    return got


RECV_KEYS = ("f_off", "f_len", "plain_off", "flags", "status", "plain")


def _same_receive_side(got, dec):
    """Bit-equal to what zmqg_decode_zmtp_multi writes: every slot of every array, all of `plain`, the peer nonces."""
    assert got["results"] == dec["results"] and got["peer"] == dec["peer"]
    for k in RECV_KEYS:
        assert got[k].shape == dec[k].shape and (got[k] == dec[k]).all(), k


def _compare(got, m, c):
    r = m["recv"]
    assert got["results"] == r["results"] and got["peer"] == r["peer"]
    assert (got["f_off"] == r["f_off"]).all() and (got["f_len"] == r["f_len"]).all()
    assert (got["plain_off"] == r["f_off"]).all()
    assert (got["status"] == r["status"]).all() and (got["flags"] == r["flags"]).all()
    for s, res in enumerate(r["results"]):  # the returned frames' payloads, at their bodies' offsets
        for k in range(s * c["max_frames"], s * c["max_frames"] + res["frames"]):
            a, ln = int(r["f_off"][k]), max(int(r["f_len"][k]) - 33, 0)
            assert (got["plain"][a:a + ln] == r["out"][a:a + ln]).all()
    assert got["fwd"] == [{k: f[k] for k in ("seq", "held_first", "forwarded", "failed")} for f in m["fwd"]]
    e = m["enc"]
    assert got["pair_off"] == e["frame_off"]
    assert got["pair_status"] == e["status"]
    assert got["dst_results"] == e["results"]
    bad = np.nonzero(got["out"] != e["out"])[0]
    assert bad.size == 0, (bad[:8].tolist(), got["out"][bad[:8]].tolist(), e["out"][bad[:8]].tolist())
    assert (got["out"][m["cap"]:] == M.SENTINEL).all()
    assert got["send"] == e["send"]


def _tamper(frame):
    b = bytearray(frame)
    b[-1] ^= 1
    return bytes(b)


@functools.lru_cache(maxsize=None)
def _core():
    """4 source streams on sessions 0-3, 3 destinations on sessions 4-6,
    max_frames 6; routes s0 -> {d0, d1}, s1 -> {d1}, s2 -> {}, s3 -> {d2, d2}."""
    rng = np.random.default_rng(4242)
    precoms = [_rng_bytes(rng, 32) for _ in range(7)]
    pay = lambda n: _rng_bytes(rng, n)
    # s0: five frames (fewer than max_frames); a COMMAND between the two parts of its first message; ends on an open part
    s0 = F.source_frames(precoms[0], [(MORE, pay(222)), (CMD, pay(10)), (LAST, pay(223)), (LAST, pay(0)),
                                      (MORE, pay(1))])
    # s1: a tampered tag in the middle, valid frames behind it, an incomplete frame at the end
    f1 = F.source_frames(precoms[1], [(LAST, pay(5000)), (MORE, pay(1)), (LAST, pay(222)), (LAST, pay(0)),
                                      (LAST, pay(223)), (LAST, pay(300))])
    f1[2] = _tamper(f1[2])
    f1[5] = f1[5][:-7]
    # s2: routed nowhere
    s2 = F.source_frames(precoms[2], [(LAST, pay(223)), (LAST, pay(1))])
    # s3: frame 0 again as frame 2 (a replayed nonce); seven frames, one more than max_frames
    f3 = F.source_frames(precoms[3], [(LAST, pay(1)), (MORE, pay(222)), (LAST, pay(5000)), (LAST, pay(0)),
                                      (LAST, pay(223)), (LAST, pay(1))])
    f3.insert(2, f3[0])
    streams = [b"".join(x) for x in (s0, f1, s2, f3)]
    return _case(precoms, [0, 1, 2, 3], streams, [[0, 1], [1], [], [2, 2]], [4, 5, 6], 6,
                 send=[1, 1, 1, 1, 11, 2 ** 32 - 2, 2 ** 40])


@functools.lru_cache(maxsize=None)
def _core_model(in_place=False):
    return _model(_core(), in_place=in_place)


def _check_core_shape(m):
    """The core case holds what it is meant to hold."""
    r, f = m["recv"], m["fwd"]
    assert [x["frames"] for x in r["results"]] == [5, 5, 2, 6]
    assert r["status"][6 + 2] != 0 and (r["status"][6 + 3:6 + 5] == 0).all()     # s1: the tampered frame, valid ones behind
    assert r["status"][18 + 2] != 0 and (r["status"][18 + 3:18 + 6] == 0).all()  # s3: the replay
    assert r["flags"][1] & CMD
    assert f[0] == dict(seq=5, held_first=4, forwarded=3, failed=0, live=[True, False, True, True, False])
    assert (f[1]["held_first"], f[1]["forwarded"], f[1]["failed"]) == (1, 1, 1)  # [last, more, FAIL, ...]
    assert (f[2]["held_first"], f[2]["forwarded"]) == (2, 2)
    assert (f[3]["held_first"], f[3]["forwarded"], f[3]["failed"]) == (1, 1, 1)
    assert m["N"] == 6 * 2 + 6 + 0 + 6 * 2 and m["base"] == [0, 12, 18, 18, 30]
    assert [x["frames"] for x in m["enc"]["results"]] == [3, 4, 2]               # d2: two copies of s3's message


@pytest.mark.gpu
@pytest.mark.parametrize("in_place", [False, True])
def test_core_matches_the_model_and_decode_zmtp_multi(torch_cuda, C, in_place):
    """Payloads of 0, 1, 222 / 223 and 5,000 bytes at odd stream offsets; every
    output against the model and the receive side against the decode call."""
    c, m = _core(), _core_model(in_place)
    _check_core_shape(m)
    got = _forward(torch_cuda, C, c, m["N"], m["cap"], m["total"] + PAD, in_place=in_place)
    _compare(got, m, c)
    dec = _decode_only(torch_cuda, C, c, in_place)
    dec["ctx"].close()
    _same_receive_side(got, dec)
    if not in_place:  # nothing but the returned frames' payload regions is written
        region = np.zeros(len(c["arena"]), bool)
        for k in range(len(c["offs"]) * c["max_frames"]):
            region[int(got["f_off"][k]):int(got["f_off"][k]) + max(int(got["f_len"][k]) - 33, 0)] = True
        assert (got["plain"][~region] == FILL).all()


def _live_frames(C, dec, c):
    """The encode descriptors of the two-call path, built on the host from the decode's outputs."""
    fs, fl, off, ln = [], [], [], []
    for s in range(len(c["offs"])):
        k0 = s * c["max_frames"]
        q = [(int(dec["flags"][k]), bool(dec["status"][k] != 0)) for k in range(k0, k0 + dec["results"][s]["frames"])]
        live = F.rule(q)["live"]
        for j, on in enumerate(live):
            for d in c["routes"][s] if on else []:
                fs.append(d), fl.append(q[j][0] & MORE), off.append(int(dec["plain_off"][k0 + j]))
                ln.append(int(dec["f_len"][k0 + j]) - 33)
    return fs, fl, off, ln


@pytest.mark.gpu
def test_equals_the_two_call_path(torch_cuda, C):
    """zmqg_decode_zmtp_multi, the descriptors built on the host from what it
    returned, zmqg_encode_zmtp_multi: the same `out`, the same nonces."""
    torch = torch_cuda
    c, m = _core(), _core_model()
    got = _forward(torch, C, c, m["N"], m["cap"], m["total"] + PAD)
    dec = _decode_only(torch, C, c)
    ctx, b = dec["ctx"], dec["b"]
    fs, fl, off, ln = _live_frames(C, dec, c)
    n, dev = len(fs), torch.device("cuda", 0)
    d_out = torch.full((m["total"] + PAD,), M.SENTINEL, dtype=torch.uint8, device=dev)
    d_foff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_res = torch.zeros((3, 4), dtype=torch.int64, device=dev)
    ctx.encode_zmtp_multi(_t(torch, c["dst_sid"], np.uint32, np.int32), _t(torch, fs, np.uint32, np.int32), None,
                          _t(torch, fl, np.uint8, np.uint8), _t(torch, off, np.uint64, np.int64),
                          _t(torch, ln, np.uint32, np.int32), b["plain"], d_out, d_foff, None, d_res,
                          out_bytes=m["cap"])
    torch.cuda.synchronize()
    assert n == sum(p[3] for p in m["pairs"]) > 0
    assert (d_out.cpu().numpy() == got["out"]).all()
    assert ctx.zmtp_send_results(d_res) == got["dst_results"]
    assert [ctx.get_nonce(s) for s in range(7)] == got["send"] and [ctx.get_peer_nonce(s) for s in range(7)] == got["peer"]
    ctx.close()


def _peer_decode(torch, C, precoms, dst_sid, runs, d_out, max_frames, peer_nonce):
    """A peer ctx (a client: the prefixes swapped) decodes every destination's
    run out[off .. +len); returns per destination [(msg_t flags, payload)]."""
    dev = torch.device("cuda", 0)
    D, slots = len(runs), len(runs) * max_frames
    peer = C.CurveContext(0, len(precoms))
    for s, p in enumerate(precoms):
        peer.session_set(s, p, C.CLIENT_PREFIX, C.SERVER_PREFIX, False, peer_nonce[s])
    foff = torch.zeros(slots, dtype=torch.int64, device=dev)
    flen = torch.zeros(slots, dtype=torch.int32, device=dev)
    poff = torch.zeros(slots, dtype=torch.int64, device=dev)
    pay = torch.zeros(int(d_out.numel()), dtype=torch.uint8, device=dev)
    fl = torch.zeros(slots, dtype=torch.uint8, device=dev)
    st = torch.full((slots,), -1, dtype=torch.int32, device=dev)
    res = torch.full((D, 4), -1, dtype=torch.int64, device=dev)
    peer.decode_zmtp_multi(_t(torch, dst_sid, np.uint32, np.int32), _t(torch, [r[0] for r in runs], np.uint64, np.int64),
                           _t(torch, [r[1] for r in runs], np.uint32, np.int32), d_out, -1, max_frames, foff, flen, poff,
                           pay, fl, st, res)
    torch.cuda.synchronize()
    back = peer.zmtp_results(res)
    peer.close()
    pay, poff, flen, fl, st = pay.cpu().numpy(), poff.cpu().numpy(), flen.cpu().numpy(), fl.cpu().numpy(), st.cpu().numpy()
    msgs = []
    for d in range(D):
        assert back[d]["error"] == 0 and back[d]["consumed"] == runs[d][1]
        ks = range(d * max_frames, d * max_frames + back[d]["frames"])
        assert all(st[k] == 0 for k in ks)
        msgs.append([(int(fl[k]), pay[int(poff[k]):int(poff[k]) + int(flen[k]) - 33].tobytes()) for k in ks])
    return msgs


def _expected(m, D):
    """Per destination, the forwarded parts in pair order: (MORE bit, payload)."""
    want = [[] for _ in range(D)]
    for p, (_, _, _, live) in enumerate(m["pairs"]):
        if live:
            want[m["frame_stream"][p]].append((m["flags"][p], m["payloads"][p]))
    return want


@pytest.mark.gpu
def test_round_trip_through_a_peer(torch_cuda, C):
    """Each destination's run, dst_results[d].out_off / out_bytes, decoded by a
    peer ctx: the payloads, MORE bits and order are the forwarded messages."""
    c, m = _core(), _core_model()
    got = _forward(torch_cuda, C, c, m["N"], m["cap"], m["total"] + PAD)
    runs = [(r["out_off"], r["out_bytes"]) for r in got["dst_results"]]
    msgs = _peer_decode(torch_cuda, C, c["precoms"], c["dst_sid"], runs, got["d_out"], 8, [PEER0] * 7)
    want = _expected(m, 3)
    assert msgs == want
    assert [len(w) for w in want] == [3, 4, 2] and want[2][0] == want[2][1]  # s3's message twice on d2
    assert all(w[-1][0] == 0 for w in want)                                  # every run ends on a whole message


@functools.lru_cache(maxsize=None)
def _two_calls(a_fails):
    """Sources A and B (sessions 0, 1) both route to D (session 2).  Call 1: A
    ends on a part with MORE, B holds complete messages.  Call 2: A's carry
    and its closing part (tampered with when a_fails), and more of B."""
    rng = np.random.default_rng(777)
    precoms = [_rng_bytes(rng, 32) for _ in range(3)]
    pa = [_rng_bytes(rng, n) for n in (40, 223, 1)]
    pb = [_rng_bytes(rng, n) for n in (5, 300, 0, 64)]
    fa = F.source_frames(precoms[0], [(LAST, pa[0]), (MORE, pa[1]), (LAST, pa[2])])
    fb = F.source_frames(precoms[1], [(LAST, pb[0]), (MORE, pb[1]), (LAST, pb[2]), (LAST, pb[3])])
    if a_fails:
        fa[2] = _tamper(fa[2])
    c1 = _case(precoms, [0, 1], [b"".join(fa[:2]), b"".join(fb[:3])], [[0], [0]], [2], 4, send=[1, 1, 9])
    m1 = _model(c1)
    # the host's bookkeeping between the calls: A's held part becomes its carry
    f = m1["fwd"][0]
    assert (f["seq"], f["held_first"], f["failed"]) == (2, 1, 0) and m1["fwd"][1]["held_first"] == 3
    k = 0 * 4 + 1
    held = (int(m1["recv"]["f_off"][k]), int(m1["recv"]["f_len"][k]) - 33, int(m1["recv"]["flags"][k]))
    assert held[1:] == (223, MORE)
    L1 = len(c1["arena"])
    c2 = _case(precoms, [0, 1], [fa[2], fb[3]], [[0], [0]], [2], 4, send=m1["enc"]["send"], peer=m1["recv"]["peer"],
               carry=[[held], []], base_off=L1)
    plain2 = np.full(len(c2["arena"]), FILL, np.uint8)
    plain2[held[0]:held[0] + held[1]] = m1["recv"]["out"][held[0]:held[0] + held[1]]
    c2["plain"] = plain2
    return c1, m1, c2, _model(c2), pa, pb


@pytest.mark.gpu
@pytest.mark.parametrize("a_fails", [False, True])
def test_carry_and_fan_in(torch_cuda, C, a_fails):
    """D's two runs, concatenated, parse into whole messages that never mix A's
    parts with B's; held_first / seq of call 1 name the carried part.  When A
    fails in call 2, nothing of its held message reaches D."""
    torch = torch_cuda
    c1, m1, c2, m2, pa, pb = _two_calls(a_fails)
    ctx = _ctx(C, c1)
    d_plain = torch.full((len(c2["arena"]),), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
    g1 = _forward(torch, C, c1, m1["N"], m1["cap"], m1["total"] + PAD, ctx=ctx, d_plain=d_plain[:len(c1["arena"])])
    _compare(g1, m1, c1)
    assert (g1["fwd"][0]["seq"], g1["fwd"][0]["held_first"]) == (2, 1)
    g2 = _forward(torch, C, c2, m2["N"], m2["cap"], m2["total"] + PAD, ctx=ctx, d_plain=d_plain)
    ctx.close()
    _compare(g2, m2, c2)
    assert m2["N"] == (1 + 4) + 4 and g2["fwd"][0]["failed"] == int(a_fails)
    # D's runs, one behind the other, through a peer
    r1, r2 = g1["dst_results"][0], g2["dst_results"][0]
    both = torch.cat([g1["d_out"][r1["out_off"]:r1["out_off"] + r1["out_bytes"]],
                      g2["d_out"][r2["out_off"]:r2["out_off"] + r2["out_bytes"]]])
    msgs = _peer_decode(torch, C, c1["precoms"], [2], [(0, r1["out_bytes"] + r2["out_bytes"])], both, 12, [PEER0] * 3)[0]
    tail = [] if a_fails else [(MORE, pa[1]), (LAST, pa[2])]
    assert msgs == [(LAST, pa[0]), (LAST, pb[0]), (MORE, pb[1]), (LAST, pb[2])] + tail + [(LAST, pb[3])]
    if a_fails:
        assert g2["fwd"][0] == dict(seq=2, held_first=0, forwarded=0, failed=1)
        assert pa[1] not in [p for _, p in msgs]


@pytest.mark.gpu
def test_fit(torch_cuda, C):
    """out_bytes cuts the second destination's run in the middle: the fitting
    frames are a prefix, the destination reports ENOBUFS, its send counter
    advances by the fitting frames alone, nothing at or past out_bytes."""
    c, full = _core(), _core_model()
    r1 = full["enc"]["results"][1]
    cap = r1["out_off"] + r1["out_bytes"] // 2
    m = _model(c, out_bytes=cap)
    got = _forward(torch_cuda, C, c, m["N"], cap, full["total"] + PAD)
    _compare(got, m, c)
    R = got["dst_results"]
    assert [r["error"] for r in R] == [0, errno.ENOBUFS, errno.ENOBUFS]
    assert 0 < R[1]["frames"] < r1["frames"] and R[2]["frames"] == 0
    mine = [got["pair_status"][p] for p in range(m["N"]) if m["frame_stream"][p] == 1]
    assert mine == [0] * R[1]["frames"] + [C.ERR_BOUND] * (len(mine) - R[1]["frames"])
    assert got["send"][4:] == [c["send"][4] + R[0]["frames"], c["send"][5] + R[1]["frames"], c["send"][6]]
    assert (got["out"][cap:] == M.SENTINEL).all()
    assert got["pair_off"] == full["enc"]["frame_off"]  # a pair that does not fit keeps its offset


@pytest.mark.gpu
def test_shared_sessions_follow_slot_and_pair_order(torch_cuda, C):
    """Two sources on one session: the later stream sees the earlier one's
    nonces.  Two destinations on one session: the nonces go in pair order."""
    rng = np.random.default_rng(99)
    precoms = [_rng_bytes(rng, 32) for _ in range(2)]
    parts = [(LAST, _rng_bytes(rng, 30)), (MORE, _rng_bytes(rng, 1)), (LAST, _rng_bytes(rng, 222)),
             (LAST, _rng_bytes(rng, 223)), (LAST, _rng_bytes(rng, 7))]
    fr = F.source_frames(precoms[0], parts)
    # stream 1 holds the connection's frames 3 and 0: frame 0's nonce is behind stream 0's by then
    c = _case(precoms, [0, 0], [b"".join(fr[:3]), fr[3] + fr[0]], [[0, 1], [1, 0]], [1, 1], 4, send=[1, 2 ** 32 - 3])
    m = _model(c)
    assert [x["frames"] for x in m["recv"]["results"]] == [3, 2] and m["recv"]["status"][4 + 1] != 0
    assert m["enc"]["send"][1] == 2 ** 32 - 3 + 8 and m["fwd"][1]["failed"] == 1
    got = _forward(torch_cuda, C, c, m["N"], m["cap"], m["total"] + PAD)
    _compare(got, m, c)
    # the nonces on the wire rise in pair order across the two destinations
    nonces = []
    for p in range(m["N"]):
        if m["pairs"][p][3]:
            a, Fp = got["pair_off"][p], m["enc"]["F"][p]
            body = got["out"][a + (9 if Fp > 257 else 2):][:16].tobytes()
            assert body[:8] == Z.MESSAGE
            nonces.append(int.from_bytes(body[8:], "big"))
    assert nonces == list(range(2 ** 32 - 3, 2 ** 32 - 3 + 8))


@functools.lru_cache(maxsize=None)
def _long():
    """Nine source streams (three workgroups of the per-stream scan) of up to
    141 small frames at max_frames 140 (three 64-element steps of a wave), the
    deciding elements on both sides of a step's edge; 1,405 pairs (six
    workgroups of the per-pair kernel)."""
    rng = np.random.default_rng(31337)
    precoms = [_rng_bytes(rng, 32) for _ in range(11)]
    pay = lambda: _rng_bytes(rng, int(rng.integers(0, 9)))
    only = lambda n, last: [(LAST if i in last else MORE, pay()) for i in range(n)]
    parts = [only(135, set(range(135))),                      # 0: single-part messages
             only(130, {63}),                                 # 1: E in the last lane of the first step
             only(130, {64}),                                 # 2: E in the first lane of the second step
             [(int(rng.choice([0, 1, 1, 2, 3])), pay()) for _ in range(100)],  # 3: fails at 70 behind a carry of 3
             only(100, set(range(100))),                      # 4: fails at frame 64
             only(100, set(range(100))),                      # 5: fails at frame 63; no routes
             [],                                              # 6: nothing received, a carried message flushed
             only(141, {139}),                                # 7: one frame more than max_frames; E in the third step
             [(CMD, pay()) for _ in range(70)]]               # 8: commands only
    frames = [F.source_frames(precoms[s], p) for s, p in enumerate(parts)]
    for s, i in ((3, 70), (4, 64), (5, 63)):
        frames[s][i] = _tamper(frames[s][i])
    c = _case(precoms, list(range(9)), [b"".join(f) for f in frames], [[0], [1, 0], [0], [1], [0, 1], [], [1], [0], [1]],
              [9, 10], 140, send=[1] * 9 + [5, 2 ** 32 - 100])
    n = len(c["arena"])
    c["plain"] = np.concatenate([np.full(n, FILL, np.uint8), rng.integers(0, 256, 64, dtype=np.uint8)])
    c["carry"][3] = [(n + 1, 7, MORE), (n + 9, 3, CMD), (n + 13, 0, MORE)]
    c["carry"][6] = [(n + 20, 30, MORE), (n + 50, 1, LAST)]
    return c


@pytest.mark.gpu
def test_long_streams(torch_cuda, C):
    c = _long()
    m = _model(c)
    f = m["fwd"]
    assert [x["seq"] for x in f] == [135, 130, 130, 103, 100, 100, 2, 140, 70] and m["N"] == 1405
    assert [x["held_first"] for x in f[:3]] == [135, 64, 65] and f[3]["failed"] == 1 and f[3]["held_first"] <= 73
    assert (f[4]["forwarded"], f[5]["forwarded"], f[6]["forwarded"], f[7]["held_first"], f[8]["forwarded"]) == (
        64, 63, 2, 140, 0)
    got = _forward(torch_cuda, C, c, m["N"], m["cap"], m["total"] + PAD)
    _compare(got, m, c)


@pytest.mark.gpu
def test_edges(torch_cuda, C):
    """n_streams == 0; N == 0; max_frames == 0 with a carry; a destination on a
    session the ctx does not have."""
    torch = torch_cuda
    core = _core()
    # N == 0 (no routes at all): the receive side and fwd are done, pair_off[0] = 0, dst_results as for n == 0
    c = dict(core, routes=[[], [], [], []])
    m = _model(c)
    assert m["N"] == 0
    got = _forward(torch, C, c, 0, m["cap"], m["total"] + PAD)
    _compare(got, m, c)
    assert got["pair_off"] == [0] and got["dst_results"] == [dict(frames=0, out_off=0, out_bytes=0, error=0)] * 3
    assert got["fwd"][0]["forwarded"] == 3 and (got["out"] == M.SENTINEL).all()
    # a destination whose session the ctx does not have: EINVAL in its result, ZMQG_ERR_SESSION on its pairs
    c = dict(core, dst_sid=[4, 7, 6])
    m = _model(c)
    got = _forward(torch, C, c, m["N"], m["cap"], m["total"] + PAD)
    _compare(got, m, c)
    assert got["dst_results"][1] == dict(frames=0, out_off=got["dst_results"][2]["out_off"], out_bytes=0,
                                         error=errno.EINVAL)
    assert all(got["pair_status"][p] == C.ERR_SESSION and got["pair_off"][p] == M.UINT64_MAX
               for p in range(m["N"]) if m["pairs"][p][3] and m["frame_stream"][p] == 1)
    assert got["send"][5] == core["send"][5]
    # max_frames == 0 with a carry: the carry alone is flushed
    rng = np.random.default_rng(5)
    plain = rng.integers(0, 256, 600, dtype=np.uint8)
    c = _case(core["precoms"], [0, 1], [b"\x00" * 4, b"\x00" * 4], [[0], [1, 0]], [4, 5], 0, core["send"],
              carry=[[(3, 223, MORE), (301, 0, CMD), (400, 1, LAST), (500, 9, MORE)], [(250, 40, LAST)]], plain=plain)
    m = _model(c)
    assert m["N"] == 4 + 2 and [f["forwarded"] for f in m["fwd"]] == [2, 1]
    got = _forward(torch, C, c, m["N"], m["cap"], m["total"] + PAD)
    _compare(got, m, c)
    assert got["results"] == [dict(frames=0, consumed=0, out_bytes=0, error=0)] * 2
    assert got["fwd"][0] == dict(seq=4, held_first=3, forwarded=2, failed=0)
    assert (got["plain"] == plain).all()
    # n_streams == 0: nothing is done
    ctx = _ctx(C, core)
    dev = torch.device("cuda", 0)
    keep = torch.full((16,), -3, dtype=torch.int64, device=dev)
    a = C.ForwardZmtp(ctypes.sizeof(C.ForwardZmtp), 0)
    a.results, a.fwd, a.pair_off, a.dst_results, a.n_dst, a.max_frames = (C._ptr(keep), C._ptr(keep), C._ptr(keep),
                                                                            C._ptr(keep), 1, 6)
    assert C._lib.zmqg_forward_zmtp_multi(ctx._ctx, ctypes.byref(a), C._stream_handle(None)) == 0
    torch.cuda.synchronize()
    assert bool((keep == -3).all())
    ctx.close()


@pytest.mark.gpu
def test_einval(torch_cuda, C):
    """Every -EINVAL case of the header, with nothing queued."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    core = _core()
    ctx = _ctx(C, core)
    big = C.CurveContext(0, 8193)
    z32 = torch.zeros(64, dtype=torch.int32, device=dev)
    z64 = torch.zeros(64, dtype=torch.int64, device=dev)
    buf = torch.full((256,), M.SENTINEL, dtype=torch.uint8, device=dev)
    res = torch.full((16, 4), -1, dtype=torch.int64, device=dev)
    ri = np.array([0, 1, 2], np.uint32)
    rd = np.array([0, 1], np.uint32)
    ci = np.array([0, 1, 1], np.uint32)

    def call(c=ctx._ctx, null_args=False, **kw):
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
        return C._lib.zmqg_forward_zmtp_multi(c, None if null_args else ctypes.byref(a), C._stream_handle(None))

    keepalive = []
    u32 = lambda *x: np.array(x, np.uint32)
    E = -errno.EINVAL
    assert call(c=None) == E and call(null_args=True) == E
    assert call(size=ctypes.sizeof(C.ForwardZmtp) - 8) == E and call(reserved=1) == E
    # the two underlying calls' cases
    assert call(results=None) == E and call(max_frames=2 ** 31) == E and call(n_streams=2 ** 31) == E
    assert call(n_streams=2 ** 16, max_frames=2 ** 15) == E
    for k in ("stream_sid", "stream_off", "stream_len", "inp", "frame_in_off", "frame_len", "plain_off", "plain",
              "flags_out", "status_out"):
        assert call(**{k: None}) == E, k
    assert call(n_dst=8193) == E and call(c=big._ctx) == E
    assert call(dst_sid=None) == E and call(dst_results=None) == E and call(pair_off=None) == E
    assert call(out=None) == E and call(fwd=None) == E
    # the routes and the carry
    assert call(route_idx=None) == E and call(route_idx=u32(1, 1, 2)) == E and call(route_idx=u32(0, 2, 1)) == E
    assert call(route_dst=u32(0, 2)) == E and call(route_dst=None) == E
    assert call(carry_idx=u32(0, 2, 1)) == E and call(carry_idx=u32(1, 1, 1)) == E
    assert call(carry_off=None) == E and call(carry_len=None) == E and call(carry_flags=None) == E
    # N = (c + max_frames) * d summed: one pair too many, and a product beyond 64 bits' reach of the check
    assert call(n_streams=1, max_frames=2 ** 30, route_idx=u32(0, 2), carry_idx=None) == E
    assert call(n_streams=1, max_frames=2 ** 31 - 1, route_idx=u32(0, 2 ** 32 - 1), carry_idx=None) == E
    torch.cuda.synchronize()
    assert bool((res == -1).all()) and bool((buf == M.SENTINEL).all()) and bool((z64 == 0).all())
    # the arguments the cases above start from are valid (here with outputs of their own)
    o64 = [torch.zeros(64, dtype=torch.int64, device=dev) for _ in range(3)]
    o32 = [torch.zeros(64, dtype=torch.int32, device=dev) for _ in range(3)]
    o8 = [torch.zeros(256, dtype=torch.uint8, device=dev) for _ in range(3)]
    assert call(frame_in_off=C._ptr(o64[0]), plain_off=C._ptr(o64[1]), pair_off=C._ptr(o64[2]),
                frame_len=C._ptr(o32[0]), status_out=C._ptr(o32[1]), pair_status=C._ptr(o32[2]),
                plain=C._ptr(o8[0]), flags_out=C._ptr(o8[1]), out=C._ptr(o8[2]), results=C._ptr(o64[0][32:]),
                dst_results=C._ptr(o64[1][32:])) == 0
    torch.cuda.synchronize()
    assert ctx.forward_results(res[:2]) == [dict(seq=1, held_first=0, forwarded=0, failed=0),
                                            dict(seq=0, held_first=0, forwarded=0, failed=0)]
    ctx.close()
    big.close()
