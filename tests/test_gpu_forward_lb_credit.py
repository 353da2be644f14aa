"""zmqg_forward_lb_credit_multi: the framed load-balancer call under
per-destination high-water marks, against tests/forward_lb_credit_model.py bit
for bit.  Compared everywhere: what tests/test_gpu_forward_credit.py compares
(the receive side's outputs, fwd, pair_off, pair_status, dst_results, every byte
of a sentinel-filled `out`, `plain`, every session's peer and send nonce,
dst_taken, dst_dropped and dst_credit after the call) plus dest_out and lb_cur;
a guard word sits behind each credit array and each table array.  The helpers
are tests/test_gpu_forward.py's and its siblings'.  Payloads are 1 to 300
bytes."""
import ctypes
import errno
import functools
import os
import re

import numpy as np
import pytest

from tests import forward_lb_credit_model as LC
from tests import forward_lb_model as FL
from tests import forward_model as F
from tests import test_gpu_forward as TF
from tests import test_gpu_forward_framed as TG
from tests import test_gpu_forward_router as TFR
from tests import zmtp_send_model as M

MORE, CMD, LAST = F.MORE, F.COMMAND, 0
PAD, FILL, PEER0 = TF.PAD, TF.FILL, TF.PEER0
ZMTP, WS, WSM = LC.ZMTP, LC.WS_PLAIN, LC.WS_MASKED
LB = TG.LB
UNL = LC.UNLIMITED
PREPEND, NO_GROUP, NONE, NO_PEER = FL.PREPEND, FL.NO_GROUP, FL.NONE, FL.NO_PEER
OUT_FILL = 0x5B5B5B5B   # dst_taken / dst_dropped before the call
GUARD = 0x11111111      # behind dst_credit, grp_idx, lb_dst and lb_cur

_rng_bytes, _case, _ctx, _t = TF._rng_bytes, TF._case, TF._ctx, TF._t
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(c, recv, send, credit, kw, out_bytes=None, out_size=PAD, mask=None, consume=False):
    return LC.model(recv, send, credit, c["precoms"], c["down"], c["arena"], c["offs"], c["lens"], c["sids"],
                    c["peer"], -1, c["max_frames"], c["carry"], TF._plain_init(c), c["dst_sid"], c["send"], out_bytes,
                    out_size, mask=mask, consume=consume, **kw)


def _dev_table(torch, table):
    return {k: _t(torch, list(np.asarray(table[k], np.uint32)) + [GUARD], np.uint32, np.int32)
            for k in ("grp_idx", "lb_dst", "lb_cur")}


def _call(torch, C, c, recv, send, N, credit, out_bytes, out_size, kw, consume=False, ctx=None, d_plain=None,
          mask=None, d_credit=None, d_table=None):
    """One zmqg_forward_lb_credit_multi call on a fresh ctx (or `ctx`, which
    stays open); d_credit / d_table: the device arrays of an earlier call, used
    as they stand."""
    dev = torch.device("cuda", 0)
    own = ctx is None
    ctx = ctx or _ctx(C, c)
    S, D = len(c["offs"]), len(c["dst_sid"])
    table = kw["table"]
    G, n_idx, n_all = len(table["lb_cur"]), len(table["grp_idx"]), len(table["lb_dst"])
    assert TG._pair_count(C, c, LB, kw) == N
    b = TF._recv_buffers(torch, c, False, d_plain)
    wres = torch.full((max(S, 1), 6), TG.RES_FILL, dtype=torch.int64, device=dev)
    ci = [0] + [int(x) for x in np.cumsum([len(x) for x in c["carry"]])]
    flat = [e for x in c["carry"] for e in x]
    d_out = torch.full((max(out_size, 1),), M.SENTINEL, dtype=torch.uint8, device=dev)
    d_poff = torch.full((N + 1,), -2, dtype=torch.int64, device=dev)
    d_pst = torch.full((max(N, 1),), -1, dtype=torch.int32, device=dev)
    d_dres = torch.full((max(D, 1), 4), -1, dtype=torch.int64, device=dev)
    d_fwd = torch.full((max(S, 1), 4), -1, dtype=torch.int64, device=dev)
    d_dest = torch.full((N + 1,), TG.PLAN_FILL * 0x01010101, dtype=torch.int32, device=dev)
    d_mask = None if mask is None else _t(torch, mask if len(mask) else [0], np.uint32, np.int32)
    if d_credit is None:
        d_credit = _t(torch, list(credit) + [GUARD], np.uint32, np.int32)
    d_taken = _t(torch, [OUT_FILL] * (D + 1), np.uint32, np.int32)
    d_dropped = _t(torch, [OUT_FILL] * (D + 1), np.uint32, np.int32)
    d_table = d_table or _dev_table(torch, table)
    ids = {}
    if kw.get("src_ids") is not None:
        ids = dict(src_id_off=_t(torch, [o for o, _ in kw["src_ids"]], np.uint64, np.int64),
                   src_id_len=_t(torch, [n for _, n in kw["src_ids"]], np.uint32, np.int32))
    ctx.forward_lb_credit_multi(
        recv, send, d_credit, d_taken, d_dropped, b["sid"], b["off"], b["len"], b["inp"], -1, c["max_frames"],
        b["foff"], b["flen"], b["poff"], b["plain"], b["fl"], b["st"], b["res"],
        _t(torch, c["dst_sid"], np.uint32, np.int32) if D else None, d_out, d_poff, d_pst, d_dres, d_fwd,
        consume=consume, ws_results=wres, mask=d_mask, carry_idx=ci if flat else None,
        carry_off=_t(torch, [e[0] for e in flat], np.uint64, np.int64) if flat else None,
        carry_len=_t(torch, [e[1] for e in flat], np.uint32, np.int32) if flat else None,
        carry_flags=_t(torch, [e[2] for e in flat], np.uint8, np.uint8) if flat else None, out_bytes=out_bytes,
        flags=kw["flags"], stream_group=kw["stream_group"], grp_idx=d_table["grp_idx"][:n_idx],
        lb_dst=d_table["lb_dst"][:n_all], lb_cur=d_table["lb_cur"][:G], n_groups=G, n_lb=table["n_lb"],
        dest_out=d_dest, **ids)
    torch.cuda.synchronize()
    got = TF._recv_outputs(C, ctx, b, c)
    if recv == ZMTP:
        assert bool((wres == TG.RES_FILL).all())
    else:
        assert bool((b["res"] == -1).all())
        got["results"] = ctx.ws_results(wres)[:S]
    u32 = lambda t: [int(x) for x in t.cpu().numpy().view(np.uint32)]
    assert u32(d_taken)[D] == OUT_FILL and u32(d_dropped)[D] == OUT_FILL and u32(d_credit)[D] == GUARD
    tab = {k: u32(v) for k, v in d_table.items()}
    assert tab["grp_idx"] == [int(x) for x in table["grp_idx"]] + [GUARD]  # the call writes neither
    assert tab["lb_dst"] == [int(x) for x in table["lb_dst"]] + [GUARD] and tab["lb_cur"][G] == GUARD
    dest = u32(d_dest)
    assert dest[N] == TG.PLAN_FILL * 0x01010101
    got.update(fwd=ctx.forward_results(d_fwd)[:S], pair_off=[int(x) for x in d_poff.cpu().numpy().view(np.uint64)],
               pair_status=[int(x) & 0xffffffff for x in d_pst.cpu().numpy()[:N]],
               dst_results=ctx.zmtp_send_results(d_dres)[:D], out=d_out.cpu().numpy()[:out_size],
               send=[ctx.get_nonce(s) for s in range(len(c["precoms"]))], d_out=d_out, d_plain=b["plain"],
               inp=b["inp"].cpu().numpy(), taken=u32(d_taken)[:D], dropped=u32(d_dropped)[:D],
               credit=u32(d_credit)[:D], d_credit=d_credit, dest=dest[:N], lb_cur=tab["lb_cur"][:G], d_table=d_table)
    if own:
        ctx.close()
    return got


def _compare(got, m, c):
    print("taken", got["taken"], m["taken"], "dropped", got["dropped"], m["dropped"], "credit", got["credit"],
          m["credit_after"], "lb_cur", got["lb_cur"], m["lb_cur"])
    assert got["dest"] == m["dest"]
    assert got["lb_cur"] == m["lb_cur"]
    assert (got["taken"], got["dropped"], got["credit"]) == (m["taken"], m["dropped"], m["credit_after"])
    TF._compare(got, m, c)
    # a pair that is not live: no stream, UINT64_MAX; ZMQG_ERR_HWM exactly at a refused message's pairs
    for p in range(m["N"]):
        if m["frame_stream"][p] == F.NO_STREAM:
            assert got["pair_status"][p] == (LC.ERR_HWM if m["hwm"][p] else M.ERR_SESSION)
            assert got["pair_off"][p] == M.UINT64_MAX
            assert got["dest"][p] >= NO_PEER and (got["dest"][p] == NO_PEER or not m["hwm"][p])
        else:
            assert got["pair_status"][p] != LC.ERR_HWM


def _run(torch, C, c, credit, kw, recv=ZMTP, send=ZMTP, **opt):
    m = _model(c, recv, send, credit, kw, **opt)
    got = _call(torch, C, c, recv, send, m["N"], credit, m["cap"], m["size"], kw, **opt)
    _compare(got, m, c)
    return m, got


def _table(groups, cur, pad=0):
    idx, dst = [pad], [0x7fffffff] * pad
    for g in groups:
        dst += list(g)
        idx.append(len(dst))
    return dict(grp_idx=idx, lb_dst=dst, lb_cur=list(cur), n_lb=len(dst))


def _simple(seed, parts, n_dst, dst_sessions=None, max_frames=None):
    """Streams on sessions 0 .. S - 1; destination t on session S + t % dst_sessions."""
    rng = np.random.default_rng(seed)
    S = len(parts)
    ns = dst_sessions or n_dst
    precoms = [_rng_bytes(rng, 32) for _ in range(S + ns)]
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in enumerate(parts)]
    mf = max_frames if max_frames is not None else max(len(p) for p in parts) + 1
    return _case(precoms, list(range(S)), streams, [[] for _ in range(S)], [S + t % ns for t in range(n_dst)], mf,
                 send=[1 + 3 * i for i in range(S + ns)])


def _heads(m, s=None):
    """dest of every message's first element slot, in pair order (of stream s, or of all)."""
    return [m["dest"][p] for p, (ps, q, _, _, is_id) in enumerate(m["pairs"])
            if not is_id and (s is None or ps == s) and q < len(m["head"][ps]) and m["head"][ps][q] == q]


# 1 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, PREPEND])
def test_unlimited_is_the_framed_lb_call(torch_cuda, C, flags):
    """Every credit unlimited: every output is zmqg_forward_framed_multi's with
    ZMQG_FWD_LB, run on a second ctx with the same sessions; lb_cur too."""
    precoms, parts = TG._modes_parts()
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in enumerate(parts)]
    c = _case(precoms, [0, 1, 2], streams, TG.MODES_ROUTES, [3, 4, 5], 4, TG.MODES_SEND)
    kw = TG._mode_kw(LB, TFR._park(c, TG.IDS), lb_flags=flags)
    m, got = _run(torch_cuda, C, c, [UNL] * 3, kw, consume=True)
    assert sum(got["taken"]) > 0 and got["dropped"] == [0, 0, 0] and got["credit"] == [UNL] * 3
    fm = TG._model(c, LB, ZMTP, ZMTP, **kw)
    framed = TG._framed(torch_cuda, C, c, LB, ZMTP, ZMTP, fm["N"], fm["cap"], fm["size"], **kw)
    for k in ("results", "peer", "send", "fwd", "pair_off", "pair_status", "dst_results", "dest", "lb_cur"):
        assert got[k] == framed[k], k
    for k in TF.RECV_KEYS + ("out",):
        assert got[k].shape == framed[k].shape and (got[k] == framed[k]).all(), k


# 2 ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _swap_case():
    """One stream: messages of 1, 2 and 3 parts, a command inside a message, a held tail; 4 destinations."""
    rng = np.random.default_rng(9201)
    pay = lambda n: _rng_bytes(rng, n)
    parts = [[(LAST, pay(7)), (MORE, pay(300)), (LAST, pay(2)), (MORE, pay(1)), (CMD, pay(4)), (MORE, pay(33)),
              (LAST, pay(40)), (LAST, pay(9)), (LAST, pay(5)), (MORE, pay(6)), (LAST, pay(11)), (LAST, pay(1)),
              (MORE, pay(3))]]
    return _simple(9201, parts, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("ring,cur0,full,picks,cur", [([0, 1, 2, 3], 1, 1, [3, 2, 0, 3, 2, 0, 3], 2),
                                                       ([0, 1, 2], 2, 2, [0, 1, 0, 1, 0, 1, 0], 1)])
def test_the_swap_is_visible(torch_cuda, C, ring, cur0, full, picks, cur):
    """A full entry under the cursor: the last active entry takes its place (a
    stable skip would give 2, 3, 0); with nothing to swap the cursor resets."""
    c = _swap_case()
    credit = [UNL] * 4
    credit[full] = 0
    kw = dict(flags=0, src_ids=None, stream_group=[0], table=_table([ring], [cur0], pad=1))
    m, got = _run(torch_cuda, C, c, credit, kw)
    assert _heads(m) == picks and got["lb_cur"] == [cur] and got["taken"][full] == 0 and sum(got["taken"]) == 7
    assert m["fwd"][0]["held_first"] == 12 and got["dest"][12] == NONE and got["dest"][4] == NONE  # held; a command


# 3 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_credits_run_out_and_the_host_refills(torch_cuda, C):
    """Credits [1, 2, 1], eight messages: four are admitted, four refused with
    ZMQG_ERR_HWM / NO_PEER and no nonce.  The host raises dst_credit on the
    device and offers the refused messages again as carries, on the same ctx,
    with the credits and lb_cur the first call left."""
    torch = torch_cuda
    rng = np.random.default_rng(9301)
    pay = lambda n: _rng_bytes(rng, n)
    parts = [[(LAST, pay(10)), (MORE, pay(20)), (LAST, pay(30)), (LAST, pay(1)), (LAST, pay(300))],
             [(LAST, pay(5)), (LAST, pay(6)), (MORE, pay(7)), (LAST, pay(8)), (LAST, pay(9))]]
    c1 = _simple(9301, parts, 3, max_frames=6)
    kw = dict(flags=0, src_ids=None, stream_group=[0, 0], table=_table([[0, 1, 2]], [0]))
    m1 = _model(c1, ZMTP, ZMTP, [1, 2, 1], kw, consume=True)
    assert m1["picks"] == [[0, 1, 2, 1] + [LC.REFUSED] * 4] and m1["lb_cur"] == [0]
    ctx = _ctx(C, c1)
    L1 = len(c1["arena"])
    d_plain = torch.full((2 * L1 + 4096,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
    g1 = _call(torch, C, c1, ZMTP, ZMTP, m1["N"], [1, 2, 1], m1["cap"], m1["size"], kw, consume=True, ctx=ctx,
               d_plain=d_plain[:L1])
    _compare(g1, m1, c1)
    assert g1["taken"] == [1, 2, 1] and g1["dropped"] == [0, 0, 0] and g1["credit"] == [0, 0, 0]
    refused = [p for p in range(m1["N"]) if m1["hwm"][p]]
    assert len(refused) == 5 and all(g1["dest"][p] == NO_PEER for p in refused)  # four messages, one of two parts
    assert g1["send"] == [c1["send"][s] for s in range(2)] + [c1["send"][2] + 1, c1["send"][3] + 3, c1["send"][4] + 1]
    # the host's bookkeeping: the refused messages become carries, in order; two more credits for destination 2,
    # one for destination 0; lb_cur stays where the device left it
    carry = [[], []]
    for p in refused:
        s, q = m1["pairs"][p][:2]
        k = s * 6 + q
        carry[s].append((int(m1["recv"]["f_off"][k]), int(m1["recv"]["f_len"][k]) - 33,
                         int(m1["recv"]["flags"][k]) & MORE))
    g1["d_credit"][:3] += torch.tensor([1, 0, 2], dtype=torch.int32, device=g1["d_credit"].device)
    new = [[(LAST, pay(4))], [(LAST, pay(3))]]
    nonce0 = [p - PEER0 + 3 for p in m1["recv"]["peer"][:2]]
    streams = [b"".join(F.source_frames(c1["precoms"][s], new[s], nonce0[s])) for s in range(2)]
    c2 = _case(c1["precoms"], [0, 1], streams, [[], []], c1["dst_sid"], 2, send=m1["enc"]["send"],
               peer=m1["recv"]["peer"], carry=carry, base_off=L1)
    plain2 = np.full(len(c2["arena"]), FILL, np.uint8)
    plain2[:L1] = g1["plain"][:L1]
    c2["plain"] = plain2
    kw2 = dict(kw, table=dict(kw["table"], lb_cur=g1["lb_cur"]))
    m2 = _model(c2, ZMTP, ZMTP, [1, 0, 2], kw2, consume=True)
    g2 = _call(torch, C, c2, ZMTP, ZMTP, m2["N"], None, m2["cap"], m2["size"], kw2, consume=True, ctx=ctx,
               d_plain=d_plain[:len(c2["arena"])], d_credit=g1["d_credit"], d_table=g1["d_table"])
    ctx.close()
    _compare(g2, m2, c2)
    # entry 0 takes one, entry 1 is found full, entry 2 takes two; the other three of the six are refused again
    assert m2["picks"] == [[0, 2, 2] + [LC.REFUSED] * 3]
    assert g2["taken"] == [1, 0, 2] and g2["credit"] == [0, 0, 0] and g2["lb_cur"] == [0]


@pytest.mark.gpu
def test_every_credit_zero(torch_cuda, C):
    """Nothing is sent: every forwarded pair is ZMQG_ERR_HWM, `out` stays as it was, no nonce moves."""
    c = dict(_swap_case())  # (_park gives the copy a `plain` of its own)
    kw = dict(flags=PREPEND, src_ids=TFR._park(c, [b"src0"]), stream_group=[0], table=_table([[2, 0, 1]], [1]))
    m, got = _run(torch_cuda, C, c, [0, 0, 0, 5], kw, consume=True)
    assert got["taken"] == [0] * 4 and got["credit"] == [0, 0, 0, 5] and got["lb_cur"] == [0]
    assert sum(m["hwm"]) == 11 + 7 and (got["out"] == M.SENTINEL).all() and got["send"] == c["send"]
    assert got["pair_off"][-1] == 0


# 4 ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _wide_case():
    """Three streams of 130 one-part messages each in one group; 257 destinations on three sessions."""
    rng = np.random.default_rng(9401)
    parts = [[(LAST, _rng_bytes(rng, int(rng.integers(1, 9)))) for _ in range(130)] for _ in range(3)]
    return _simple(9401, parts, 257, dst_sessions=3, max_frames=130)


STEP_EDGES = {
    # the entry found full first is at position 63 (the last lane of the first wave), reached on its second visit
    "lane63": (65, 0, {63: 1, 10: 3}),
    # the last position, then two full entries side by side at the cursor: deactivations with no message between
    "last_then_two_at_once": (65, 2, {64: 0, 0: 0, 1: 0}),
    # 257 entries: the last position (the first lane's second step), then position 64 on its second visit
    "last_of_257": (257, 0, {256: 0, 64: 1}),
    "lane63_of_257": (257, 200, {63: 0}),
    "second_wave_lane0": (257, 0, {64: 0, 65: 0, 130: 0}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STEP_EDGES))
def test_step_edges(torch_cuda, C, name):
    A, cur0, finite = STEP_EDGES[name]
    c = _wide_case()
    credit = [UNL] * 257
    ring = [(7 * j) % A for j in range(A)]  # (a permutation: 7 divides neither 65 nor 257)
    for j, w in finite.items():
        credit[ring[j]] = w
    kw = dict(flags=0, src_ids=None, stream_group=[0, 0, 0], table=_table([ring], [cur0 + 5 * A], pad=3))
    m, got = _run(torch_cuda, C, c, credit, kw, consume=True)
    assert m["N"] == 390 and sum(got["taken"]) == 390 and not any(m["hwm"])
    for j, w in finite.items():
        assert got["taken"][ring[j]] == w and got["credit"][ring[j]] == 0, j
    if name == "last_then_two_at_once":  # 62 messages, then entries 64, 0 and 1 go one after the other
        assert m["picks"][0][60:65] == [62, 63, 63, 62, 2]
    if name == "lane63":  # position 63 takes message 63 and is found full by message 128; 64 has taken its place
        assert m["picks"][0][63] == 63 and m["picks"][0][126:130] == [61, 62, 64, 0]


def _kernel_const(name):
    text = open(os.path.join(ROOT, "libzmq_amd", "csrc", "curve_fwd_lb_credit.hpp")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))


@pytest.mark.gpu
@pytest.mark.parametrize("over", [0, 1])
def test_ring_at_and_above_the_lds_capacity(torch_cuda, C, over):
    """The largest ring the group kernel keeps in LDS, and one entry more, which
    works in the ctx's scratch: the first hundred messages go to entries that
    name no destination, then two full entries side by side are swapped for
    entries from the ring's end, and one entry runs out on its only visit."""
    A = _kernel_const("kFwdLbcRing") + over
    assert A in (512, 513)
    c = _wide_case()
    ring = [(7 * j) % 257 if j < 257 else 1000 + j for j in range(A)]
    credit = [UNL] * 257
    for j, w in {5: 0, 6: 0, 200: 1}.items():
        credit[ring[j]] = w
    kw = dict(flags=0, src_ids=None, stream_group=[0, 0, 0], table=_table([ring], [A - 100], pad=2))
    m, got = _run(torch_cuda, C, c, credit, kw, consume=True)
    assert m["picks"][0][98:108] == [A - 2, A - 1, 0, 1, 2, 3, 4, A - 1, A - 2, 7]
    # positions 0-4 and 7-256 name destinations; the cursor rests on position 290
    assert sum(got["taken"]) == 5 + 250 and got["credit"][ring[200]] == 0 and got["lb_cur"] == [290]


@functools.lru_cache(maxsize=None)
def _many_streams(S):
    """S streams of one one-part message each, three destinations."""
    rng = np.random.default_rng(9450 + S)
    parts = [[(LAST, _rng_bytes(rng, int(rng.integers(1, 5))))] for _ in range(S)]
    return _simple(9450 + S, parts, 3, max_frames=1)


@pytest.mark.gpu
@pytest.mark.parametrize("over", [0, 1])
def test_streams_at_and_above_the_lds_capacity(torch_cuda, C, over):
    """A group of as many streams as the group kernel searches in LDS, and one
    more, whose counts it searches in memory; two entries run out on the way."""
    S = _kernel_const("kFwdLbcStreams") + over
    assert S in (1024, 1025)
    c = _many_streams(S)
    kw = dict(flags=0, src_ids=None, stream_group=[0] * S, table=_table([[0, 1, 2]], [2]))
    m, got = _run(torch_cuda, C, c, [1, UNL, 300], kw, consume=True)
    assert got["taken"] == [1, S - 301, 300] and got["credit"] == [0, UNL, 0]
    assert m["picks"][0][:4] == [2, 0, 1, 2] and m["picks"][0][-2:] == [1, 1]


# 5 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_table_edges(torch_cuda, C):
    """Two groups with messages in one call, a stream without a group, a range
    that is empty, one that falls, one clamped to n_lb, cursors past A; an
    entry naming no destination takes its turn and is never deactivated; one
    destination named by two entries is sent more than its credit: dst_dropped
    counts the excess and the write-back saturates at 0."""
    rng = np.random.default_rng(9501)
    one = lambda: (LAST, _rng_bytes(rng, int(rng.integers(1, 301))))
    parts = [[one() for _ in range(4)], [one() for _ in range(3)], [(MORE, b"a"), (LAST, b"b"), one()], [one()],
             [one()], [one()]]
    c = _simple(9501, parts, 4)
    # g0 = [0, 3): {0, 9 (none), 1}; g1 = [3, 3): empty; g2 = [3, 9) clamped to [3, 5): {2, 2}; g3 = [5, 4): falls
    table = dict(grp_idx=[0, 3, 3, 9, 4], lb_dst=[0, 9, 1, 2, 2, 3], lb_cur=[7, 5, 0xffffffff, 6], n_lb=5)
    kw = dict(flags=0, src_ids=None, stream_group=[0, 2, 0, NO_GROUP, 1, 3], table=table)
    m, got = _run(torch_cuda, C, c, [1, 2, 1, UNL], kw, consume=True)
    # g0 from cursor 7 mod 3 = 1: 9, 1, 0, 9, 1, then 0 and 1 are full one after the other: 9 again, the only
    # entry left, on which the cursor rests; entry 1 (9) is never deactivated
    assert m["picks"][0] == [1, 2, 0, 1, 2, 1] and got["lb_cur"] == [1, 0, 0, 0]
    assert _heads(m, 0) == [NO_PEER, 1, 0, NO_PEER] and _heads(m, 2) == [1, NO_PEER]
    # g2: both entries carry destination 2's credit of 1; the third message finds the ring empty
    assert m["picks"][2] == [1, 0, LC.REFUSED] and _heads(m, 1) == [2, 2, NO_PEER]
    assert got["taken"] == [1, 2, 1, 0] and got["dropped"] == [0, 0, 1, 0] and got["credit"] == [0, 0, 0, UNL]
    hw = [p for p in range(m["N"]) if m["hwm"][p]]
    assert [m["pairs"][p][0] for p in hw] == [1]
    # without a group, an empty range, a falling range: ZMQG_ERR_SESSION, as in the LB call
    for s in (3, 4, 5):
        assert _heads(m, s) == [NO_PEER] and got["pair_status"][m["base"][s]] == M.ERR_SESSION


# 6 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_websocket_on_both_sides(torch_cuda, C):
    """Masked WebSocket receive and send with PREPEND: the mask entries of the
    refused message's pairs are poisoned on the device and must not show."""
    rng = np.random.default_rng(9601)
    precoms = [_rng_bytes(rng, 32) for _ in range(4)]
    pay = lambda n: _rng_bytes(rng, n)
    f0 = TG._ws_stream(rng, precoms[0], [(LAST, pay(10)), (MORE, pay(130)), (LAST, pay(3)), (LAST, pay(5))], True)
    f1 = TG._ws_stream(rng, precoms[1], [(LAST, pay(20)), (LAST, pay(21))], True)
    c = _case(precoms, [0, 1], [b"".join(f0), b"".join(f1)], [[], []], [2, 3], 4, [1, 1, 5, 2 ** 32 - 3])
    kw = dict(flags=PREPEND, src_ids=TFR._park(c, [b"A", b"peerB"]), stream_group=[0, 0],
              table=_table([[1, 0]], [0]))
    N = 16
    mask = TG._mask_of(N)
    m = _model(c, WSM, WSM, [2, 1], kw, mask=mask)
    assert m["N"] == N and m["picks"] == [[0, 1, 1, LC.REFUSED, LC.REFUSED]] and sum(m["hwm"]) == 4
    poisoned = [0xdeadbeef if m["hwm"][p] else k for p, k in enumerate(mask)]
    got = _call(torch_cuda, C, c, WSM, WSM, N, [2, 1], m["cap"], m["size"], kw, mask=poisoned)
    _compare(got, m, c)
    assert got["taken"] == [2, 1] and got["dropped"] == [0, 0] and got["lb_cur"] == [0]


# 7 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_fit_with_credits(torch_cuda, C):
    """out_bytes short by one frame of destination 3's run: its last admitted
    pair is ZMQG_ERR_BOUND, dst_taken still counts the message, ENOBUFS."""
    c = _swap_case()
    credit = [1, 0, UNL, 2]
    kw = dict(flags=0, src_ids=None, stream_group=[0], table=_table([[0, 1, 2, 3]], [0]))
    full = _model(c, ZMTP, ZMTP, credit, kw)
    mine = [p for p in range(full["N"]) if full["frame_stream"][p] == 3]
    cap = full["enc"]["frame_off"][mine[-1]] + 1
    size = full["total"] + PAD
    m = _model(c, ZMTP, ZMTP, credit, kw, out_bytes=cap, out_size=size)
    got = _call(torch_cuda, C, c, ZMTP, ZMTP, m["N"], credit, cap, size, kw)
    _compare(got, m, c)
    assert got["pair_status"][mine[-1]] == C.ERR_BOUND and got["pair_status"][mine[0]] == 0
    assert got["taken"] == [1, 0, 4, 2] and got["dropped"] == [0] * 4 and got["credit"] == credit
    assert got["dst_results"][3]["error"] == errno.ENOBUFS and got["dst_results"][3]["frames"] == len(mine) - 1


@pytest.mark.gpu
def test_no_pairs(torch_cuda, C):
    """max_frames 0 and no carry: N == 0.  dst_taken and dst_dropped are zero-filled, dst_credit is not
    written, lb_cur is clamped."""
    c = _simple(9701, [[(LAST, b"x")], [(LAST, b"y")]], 3, max_frames=0)
    kw = dict(flags=0, src_ids=None, stream_group=[0, NO_GROUP], table=_table([[0, 1, 2], []], [8, 3]))
    m, got = _run(torch_cuda, C, c, [0, 5, UNL], kw, consume=True)
    assert m["N"] == 0 and got["taken"] == [0, 0, 0] and got["dropped"] == [0, 0, 0] and got["credit"] == [0, 5, UNL]
    assert got["pair_off"] == [0] and got["lb_cur"] == [2, 0]


# 8 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_einval(torch_cuda, C):
    """The -EINVAL cases with a live ctx: nothing is queued, every output keeps what it held."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    ctx = C.CurveContext(0, 4)
    z32 = torch.zeros(64, dtype=torch.int32, device=dev)
    z64 = torch.zeros(64, dtype=torch.int64, device=dev)
    buf = torch.full((256,), M.SENTINEL, dtype=torch.uint8, device=dev)
    res = torch.full((16, 6), -1, dtype=torch.int64, device=dev)
    cred = torch.full((8,), 3, dtype=torch.int32, device=dev)
    cnt = torch.full((8,), 0x5B, dtype=torch.int32, device=dev)
    cur = torch.full((4,), 9, dtype=torch.int32, device=dev)
    sg = np.array([0, 0], np.uint32)

    def call(c=ctx._ctx, null_credit=False, mode=LB, plan=True, pk=None, fr=None, cr=None, **kw):
        a = C.ForwardZmtp(ctypes.sizeof(C.ForwardZmtp), 0)
        a.n_streams, a.max_frames, a.max_msg_size, a.n_dst, a.out_bytes = 2, 3, -1, 2, 256
        for k in ("stream_sid", "stream_len", "frame_len", "status_out", "dst_sid", "pair_status"):
            setattr(a, k, C._ptr(z32))
        for k in ("stream_off", "frame_in_off", "plain_off", "pair_off"):
            setattr(a, k, C._ptr(z64))
        for k in ("inp", "plain", "flags_out", "out"):
            setattr(a, k, C._ptr(buf))
        for k in ("results", "dst_results", "fwd"):
            setattr(a, k, C._ptr(res))
        for k, v in kw.items():
            setattr(a, k, v)
        p = C.ForwardLb(ctypes.sizeof(C.ForwardLb), 0, None, None, 1, sg.ctypes.data, C._ptr(z32), 1, C._ptr(z32),
                        C._ptr(cur), None)
        for k, v in (pk or {}).items():
            setattr(p, k, v)
        f = C.ForwardFraming(ctypes.sizeof(C.ForwardFraming), 0, C.FRAMING_ZMTP, C.FRAMING_ZMTP, mode, 0,
                             ctypes.addressof(p) if plan else None, C._ptr(res), C._ptr(z32))
        for k, v in (fr or {}).items():
            setattr(f, k, v)
        k3 = C.ForwardCredit(ctypes.sizeof(C.ForwardCredit), 0, C._ptr(cred), C._ptr(cnt), C._ptr(cnt))
        for k, v in (cr or {}).items():
            setattr(k3, k, v)
        return C._lib.zmqg_forward_lb_credit_multi(c, ctypes.byref(a), ctypes.byref(f),
                                                   None if null_credit else ctypes.byref(k3), C._stream_handle(None))

    E = -errno.EINVAL
    assert call(c=None) == E and call(null_credit=True) == E
    assert call(cr=dict(size=24)) == E and call(cr=dict(flags=2)) == E
    for k in ("dst_credit", "dst_taken", "dst_dropped"):
        assert call(cr={k: None}) == E, k
    for mode in (TG.STATIC, TG.SUB, TG.ROUTER, 4):
        assert call(mode=mode) == E, mode
    # the framed LB call's own
    assert call(plan=False) == E and call(fr=dict(send=3)) == E and call(fr=dict(reserved2=1)) == E
    assert call(pk=dict(size=72)) == E and call(pk=dict(flags=2)) == E and call(pk=dict(flags=PREPEND)) == E
    assert call(pk=dict(stream_group=None)) == E and call(pk=dict(lb_cur=None)) == E and call(pk=dict(lb_dst=None)) == E
    assert call(pk=dict(n_groups=0)) == E and call(pk=dict(n_lb=2 ** 31)) == E  # (a group index out of range)
    assert call(results=None) == E and call(pair_off=None) == E and call(out=None) == E and call(n_dst=0) == E
    torch.cuda.synchronize()
    assert bool((cred == 3).all()) and bool((cnt == 0x5B).all()) and bool((cur == 9).all())
    assert bool((buf == M.SENTINEL).all()) and bool((res == -1).all()) and bool((z32 == 0).all())
    ctx.close()
