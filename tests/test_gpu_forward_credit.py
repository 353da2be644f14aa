"""zmqg_forward_credit_multi: the framed forward call with a high-water mark
per destination, against tests/forward_credit_model.py bit for bit.  Compared
everywhere: what tests/test_gpu_forward_framed.py compares (the receive side's
outputs, fwd, pair_off, pair_status, dst_results, match_out / dest_out, every
byte of a sentinel-filled `out`, `plain`, every session's peer and send nonce)
and dst_taken, dst_dropped and dst_credit after the call.  The helpers are
tests/test_gpu_forward.py's and its siblings'."""
import errno
import functools
import os
import re

import numpy as np
import pytest

from tests import forward_credit_model as FC
from tests import forward_model as F
from tests import forward_router_model as FR
from tests import test_gpu_forward as TF
from tests import test_gpu_forward_framed as TG
from tests import test_gpu_forward_router as TFR
from tests import ws_model as W
from tests import zmtp_send_model as M

MORE, CMD, LAST = F.MORE, F.COMMAND, 0
PAD, PEER0 = TF.PAD, TF.PEER0
ZMTP, WS, WSM = FC.ZMTP, FC.WS_PLAIN, FC.WS_MASKED
STATIC, SUB, ROUTER = FC.STATIC, FC.SUB, FC.ROUTER
UNL = FC.UNLIMITED
OUT_FILL = 0x5B5B5B5B   # dst_taken / dst_dropped before the call

_rng_bytes, _case, _ctx, _t = TF._rng_bytes, TF._case, TF._ctx, TF._t
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile():
    """Pairs per count tile, from the kernels' header."""
    text = open(os.path.join(ROOT, "libzmq_amd", "csrc", "curve_fwd_credit.hpp")).read()
    return int(re.search(r"constexpr uint32_t kFwdCreditTile = (\d+);", text).group(1))


def _model(c, mode, recv, send, credit, out_bytes=None, out_size=PAD, mask=None, consume=False, **kw):
    return FC.model(mode, recv, send, credit, c["precoms"], c["down"], c["arena"], c["offs"], c["lens"], c["sids"],
                    c["peer"], -1, c["max_frames"], c["carry"], TF._plain_init(c), c["dst_sid"], c["send"], out_bytes,
                    out_size, routes=c["routes"], mask=mask, consume=consume, **kw)


def _credit(torch, C, c, mode, recv, send, N, credit, out_bytes, out_size, consume=False, ctx=None, d_plain=None,
            mask=None, d_credit=None, **kw):
    """One zmqg_forward_credit_multi call on a fresh ctx (or `ctx`, which stays
    open); d_credit: the device credits of an earlier call, used as they stand."""
    dev = torch.device("cuda", 0)
    own = ctx is None
    ctx = ctx or _ctx(C, c)
    S, D = len(c["offs"]), len(c["dst_sid"])
    assert TG._pair_count(C, c, mode, kw) == N
    b = TF._recv_buffers(torch, c, False, d_plain)
    wres = torch.full((max(S, 1), 6), TG.RES_FILL, dtype=torch.int64, device=dev)
    ci = [0] + [int(x) for x in np.cumsum([len(x) for x in c["carry"]])]
    ri = [0] + [int(x) for x in np.cumsum([len(x) for x in c["routes"]])]
    flat = [e for x in c["carry"] for e in x]
    d_out = torch.full((max(out_size, 1),), M.SENTINEL, dtype=torch.uint8, device=dev)
    d_poff = torch.full((N + 1,), -2, dtype=torch.int64, device=dev)
    d_pst = torch.full((max(N, 1),), -1, dtype=torch.int32, device=dev)
    d_dres = torch.full((max(D, 1), 4), -1, dtype=torch.int64, device=dev)
    d_fwd = torch.full((max(S, 1), 4), -1, dtype=torch.int64, device=dev)
    d_mask = None if mask is None else _t(torch, mask if len(mask) else [0], np.uint32, np.int32)
    if d_credit is None:
        d_credit = _t(torch, list(credit) + [0x11111111], np.uint32, np.int32)  # (a guard word behind each array)
    d_taken = _t(torch, [OUT_FILL] * (D + 1), np.uint32, np.int32)
    d_dropped = _t(torch, [OUT_FILL] * (D + 1), np.uint32, np.int32)
    plan, read_plan = TG._plan_tensors(torch, C, mode, N, kw) if mode != STATIC else ({}, dict)
    ctx.forward_credit_multi(
        recv, send, mode, d_credit, d_taken, d_dropped, b["sid"], b["off"], b["len"], b["inp"], -1, c["max_frames"],
        b["foff"], b["flen"], b["poff"], b["plain"], b["fl"], b["st"], b["res"],
        _t(torch, c["dst_sid"], np.uint32, np.int32) if D else None, ri, [d for r in c["routes"] for d in r], d_out,
        d_poff, d_pst, d_dres, d_fwd, consume=consume, ws_results=wres, mask=d_mask, carry_idx=ci if flat else None,
        carry_off=_t(torch, [e[0] for e in flat], np.uint64, np.int64) if flat else None,
        carry_len=_t(torch, [e[1] for e in flat], np.uint32, np.int32) if flat else None,
        carry_flags=_t(torch, [e[2] for e in flat], np.uint8, np.uint8) if flat else None, out_bytes=out_bytes, **plan)
    torch.cuda.synchronize()
    got = TF._recv_outputs(C, ctx, b, c)
    if recv == ZMTP:
        assert bool((wres == TG.RES_FILL).all())
    else:
        assert bool((b["res"] == -1).all())
        got["results"] = ctx.ws_results(wres)[:S]
    u32 = lambda t: [int(x) for x in t.cpu().numpy().view(np.uint32)]
    assert u32(d_taken)[D] == OUT_FILL and u32(d_dropped)[D] == OUT_FILL and u32(d_credit)[D] == 0x11111111
    got.update(fwd=ctx.forward_results(d_fwd)[:S], pair_off=[int(x) for x in d_poff.cpu().numpy().view(np.uint64)],
               pair_status=[int(x) & 0xffffffff for x in d_pst.cpu().numpy()[:N]],
               dst_results=ctx.zmtp_send_results(d_dres)[:D], out=d_out.cpu().numpy()[:out_size],
               send=[ctx.get_nonce(s) for s in range(len(c["precoms"]))], d_out=d_out, d_plain=b["plain"],
               inp=b["inp"].cpu().numpy(), taken=u32(d_taken)[:D], dropped=u32(d_dropped)[:D],
               credit=u32(d_credit)[:D], d_credit=d_credit)
    got.update(read_plan())
    if own:
        ctx.close()
    return got


def _compare(got, m, c, mode=STATIC):
    print("taken", got["taken"], m["taken"], "dropped", got["dropped"], m["dropped"], "credit", got["credit"],
          m["credit_after"])
    TF._compare(got, m, c)
    for k in TG.PLAN_OUT[mode]:
        assert got[k] == m[k], k
    assert (got["taken"], got["dropped"], got["credit"]) == (m["taken"], m["dropped"], m["credit_after"])
    # a pair that is not live: no stream, UINT64_MAX; ZMQG_ERR_HWM exactly where the pass cleared it
    for p in range(m["N"]):
        if m["frame_stream"][p] == F.NO_STREAM:
            assert got["pair_status"][p] == (FC.ERR_HWM if m["hwm"][p] else M.ERR_SESSION)
            assert got["pair_off"][p] == M.UINT64_MAX
        else:
            assert got["pair_status"][p] != FC.ERR_HWM


def _run(torch, C, c, mode, credit, recv=ZMTP, send=ZMTP, **kw):
    m = _model(c, mode, recv, send, credit, **kw)
    got = _credit(torch, C, c, mode, recv, send, m["N"], credit, m["cap"], m["size"], **kw)
    _compare(got, m, c, mode)
    return m, got


def _zmtp_case(precoms, parts, routes, dst_sid, max_frames, send, **over):
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in enumerate(parts)]
    return _case(precoms, list(range(len(parts))), streams, routes, dst_sid, max_frames, send, **over)


# 1 ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _values_case():
    """3 sources on sessions 0-2, 3 destinations on sessions 3-5, every source
    routed to every destination: messages of 1, 2 and 3 parts, a command, a
    held tail.  Every destination has 6 deliveries."""
    rng = np.random.default_rng(9101)
    precoms = [_rng_bytes(rng, 32) for _ in range(6)]
    pay = lambda n: _rng_bytes(rng, n)
    parts = [[(LAST, pay(7)), (MORE, pay(300)), (LAST, pay(2))],
             [(MORE, pay(1)), (CMD, pay(4)), (MORE, pay(0)), (LAST, pay(40)), (LAST, pay(9)), (MORE, pay(3))],
             [(MORE, pay(5)), (LAST, pay(6)), (LAST, pay(11))]]
    return _zmtp_case(precoms, parts, [[0, 1, 2], [2, 0, 1], [1, 2, 0]], [3, 4, 5], 6,
                      [1, 1, 1, 7, 2 ** 32 - 2, 2 ** 40])


@pytest.mark.gpu
@pytest.mark.parametrize("credit", [[0, 1, 2], [2, UNL, 0], [UNL, 3, UNL], [6, 7, 5]])
def test_credit_values(torch_cuda, C, credit):
    """Credits of 0, 1, 2 and unlimited; [UNL, 3, UNL] cuts destination 1 in the
    middle of its deliveries while the others stay complete; 6 and 7 admit all."""
    c = _values_case()
    m, got = _run(torch_cuda, C, c, STATIC, credit)
    D = [6, 6, 6]
    assert got["taken"] == [min(d, x) for d, x in zip(D, credit)]
    assert got["dropped"] == [d - k for d, k in zip(D, got["taken"])] and got["credit"] == credit
    if credit == [UNL, 3, UNL]:
        mine = [p for p in range(m["N"]) if m["pairs"][p][3] and c["routes"][m["pairs"][p][0]][m["pairs"][p][2]] == 1]
        assert [m["hwm"][p] for p in mine] == [False] * 6 + [True] * 4  # s0 whole, s1's first message; then nothing
        assert got["dst_results"][1]["frames"] == 6 and got["dst_results"][0]["frames"] == 10


# 2, 3 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_duplicate_route(torch_cuda, C):
    """A stream naming destination 0 twice, credit 1: exactly one copy goes out, whole."""
    rng = np.random.default_rng(9102)
    precoms = [_rng_bytes(rng, 32) for _ in range(3)]
    parts = [[(MORE, _rng_bytes(rng, 10)), (LAST, _rng_bytes(rng, 20))]]
    c = _zmtp_case(precoms, parts, [[0, 0, 1]], [1, 2], 3, [1, 5, 9])
    m, got = _run(torch_cuda, C, c, STATIC, [1, 1])
    assert got["taken"] == [1, 1] and got["dropped"] == [1, 0]
    assert [m["hwm"][p] for p in range(6)] == [False, True, False, False, True, False]
    assert got["dst_results"][0]["frames"] == 2 and got["send"][1] == 5 + 2
    msgs = TF._peer_decode(torch_cuda, C, precoms, [1], [(got["dst_results"][0]["out_off"],
                                                         got["dst_results"][0]["out_bytes"])], got["d_out"], 4,
                           [PEER0] * 3)[0]
    assert msgs == [(MORE, parts[0][0][1]), (LAST, parts[0][1][1])]


@pytest.mark.gpu
@pytest.mark.parametrize("credit,taken,dropped", [([0, 1], [0, 1], [2, 1]), ([1, UNL], [1, 2], [1, 0])])
def test_carried_head(torch_cuda, C, credit, taken, dropped):
    """A head carried from an earlier call with its last part in this call, then
    a second message: the carried message is one delivery per destination,
    admitted or dropped whole."""
    rng = np.random.default_rng(9103)
    precoms = [_rng_bytes(rng, 32) for _ in range(3)]
    head, last, second = _rng_bytes(rng, 13), _rng_bytes(rng, 8), _rng_bytes(rng, 5)
    streams = [b"".join(F.source_frames(precoms[0], [(LAST, last), (LAST, second)]))]
    arena, _ = F.arena_of(streams)
    plain = np.concatenate([np.full(len(arena), TF.FILL, np.uint8), np.frombuffer(head, np.uint8)])
    c = _case(precoms, [0], streams, [[0, 1]], [1, 2], 2, [1, 3, 4], carry=[[(len(arena), len(head), MORE)]],
              plain=plain)
    m, got = _run(torch_cuda, C, c, STATIC, credit)
    assert m["N"] == 6 and got["taken"] == taken and got["dropped"] == dropped
    # the carried head and the part that closes it share their fate
    assert m["hwm"][0] == m["hwm"][2] and m["hwm"][1] == m["hwm"][3]


# 4 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_sub(torch_cuda, C):
    """A message matched by destinations 0 and 2 of three, destination 0 at
    credit 0: match_out still says matched, its pairs report ZMQG_ERR_HWM, and
    destination 2's run is byte for byte the framed call's."""
    rng = np.random.default_rng(9104)
    precoms = [_rng_bytes(rng, 32) for _ in range(4)]
    parts = [[(MORE, b"news/a"), (LAST, _rng_bytes(rng, 50)), (LAST, b"other")]]
    c = _zmtp_case(precoms, parts, [[0, 1, 2]], [1, 2, 3], 4, [1, 5, 6, 7])
    kw = dict(subs=[[b"news"], [b"sport"], [b"ne", b"zz"]])
    m, got = _run(torch_cuda, C, c, SUB, [0, UNL, 1], **kw)
    assert got["match"][:6] == [1, 0, 1, 1, 0, 1] and got["taken"] == [0, 0, 1] and got["dropped"] == [1, 0, 0]
    assert [got["pair_status"][p] for p in (0, 3)] == [FC.ERR_HWM] * 2
    assert [got["pair_status"][p] for p in (2, 5)] == [0, 0]
    fm = TG._model(c, SUB, ZMTP, ZMTP, **kw)
    framed = TG._framed(torch_cuda, C, c, SUB, ZMTP, ZMTP, fm["N"], fm["cap"], fm["size"], **kw)
    a, b = got["dst_results"][2], framed["dst_results"][2]
    assert (a["frames"], a["out_bytes"]) == (b["frames"], b["out_bytes"]) == (2, a["out_bytes"]) and a["out_bytes"] > 0
    assert (got["out"][a["out_off"]:a["out_off"] + a["out_bytes"]] ==
            framed["out"][b["out_off"]:b["out_off"] + b["out_bytes"]]).all()
    assert got["send"][3] == framed["send"][3] and got["send"][1] == 5 and framed["send"][1] == 7


# 5 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("flags", [FR.ROUTE, FR.ROUTE | FR.PREPEND])
def test_router(torch_cuda, C, flags):
    """Peer B (destination 1) at credit 1 is addressed twice: the first message
    is sent, the second dropped whole, dest_out still names it.  The consumed
    address takes no credit of its own; an unknown and a malformed message take
    none either."""
    rng = np.random.default_rng(9105)
    precoms = [_rng_bytes(rng, 32) for _ in range(5)]
    pay = lambda n: _rng_bytes(rng, n)
    if flags & FR.PREPEND:  # the address is the source's own id: streams 0 and 1 are "peerB", stream 2 is unknown
        parts = [[(MORE, pay(9)), (LAST, pay(20))], [(LAST, pay(30))], [(LAST, pay(4))]]
        ids = [b"peerB", b"peerB", b"nobody"]
    else:
        parts = [[(MORE, b"peerB"), (MORE, pay(9)), (LAST, pay(20)), (LAST, b"peerB")],   # whole, then malformed
                 [(MORE, b"nobody"), (LAST, pay(3)), (MORE, b"peerB"), (LAST, pay(30))],  # unknown, then whole
                 [(MORE, b"peerA"), (LAST, pay(4))]]
        ids = [b"x", b"y", b"z"]
    c = _zmtp_case(precoms, parts, [[0], [0], [0]], [3, 4], 4, [1, 1, 1, 5, 9])
    kw = dict(flags=flags, src_ids=TFR._park(c, ids), table=FR.table_of([(b"peerA", 0), (b"peerB", 1)]))
    m, got = _run(torch_cuda, C, c, ROUTER, [UNL, 1], **kw)
    assert got["taken"] == ([0, 1] if flags & FR.PREPEND else [1, 1])
    assert got["dropped"] == [0, 1]
    cleared = [p for p in range(m["N"]) if m["hwm"][p]]
    assert cleared == ([4] if flags & FR.PREPEND else [7]) and all(got["dest"][p] == 1 for p in cleared)
    assert got["dst_results"][1]["frames"] == 2 and got["send"][4] == 9 + 2
    if not flags & FR.PREPEND:
        assert got["dest"][:8] == [FR.ADDRESS, 1, 1, FR.MALFORMED, FR.ADDRESS, FR.UNKNOWN, FR.ADDRESS, 1]


@pytest.mark.gpu
def test_prepend_alone(torch_cuda, C):
    """The m = 2 pair space: a delivery starts at its id slot, and a refused one loses the id part with the rest."""
    rng = np.random.default_rng(9106)
    precoms = [_rng_bytes(rng, 32) for _ in range(3)]
    parts = [[(LAST, _rng_bytes(rng, 6)), (MORE, _rng_bytes(rng, 7)), (LAST, _rng_bytes(rng, 8))]]
    c = _zmtp_case(precoms, parts, [[1, 0]], [1, 2], 3, [1, 5, 9])
    kw = dict(flags=FR.PREPEND, src_ids=TFR._park(c, [b"src0"]), table=None)
    m, got = _run(torch_cuda, C, c, ROUTER, [1, 2], **kw)
    assert m["N"] == 12 and got["taken"] == [1, 2] and got["dropped"] == [1, 0]
    assert [p for p in range(12) if m["hwm"][p]] == [5, 7, 11]  # the id slot, the head and the last part for t = 0


# 6 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_invalid_session(torch_cuda, C):
    """Destination 0 has no session and credit 1: it takes the credit, its
    admitted pairs are ZMQG_ERR_SESSION as before, the refused ones ZMQG_ERR_HWM."""
    rng = np.random.default_rng(9107)
    precoms = [_rng_bytes(rng, 32) for _ in range(2)]
    parts = [[(LAST, _rng_bytes(rng, 6)), (LAST, _rng_bytes(rng, 7))]]
    c = _zmtp_case(precoms, parts, [[0, 1]], [77, 1], 2, [1, 5])
    m, got = _run(torch_cuda, C, c, STATIC, [1, UNL])
    assert got["taken"] == [1, 2] and got["dropped"] == [1, 0]
    assert got["pair_status"] == [M.ERR_SESSION, 0, FC.ERR_HWM, 0]
    assert got["dst_results"][0]["error"] == errno.EINVAL and got["dst_results"][1]["frames"] == 2


# 7 ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _seam_case(n_streams):
    """Streams of 65 elements and four routes each, 260 pairs a stream: one-part
    messages but for a two-part message at elements 63 - i and 64 - i of stream
    i.  Its first part's pairs end at pair 256 (i + 1), so with a tile of 256
    pairs the message straddles the edge of tiles i and i + 1."""
    rng = np.random.default_rng(9108 + n_streams)
    precoms = [_rng_bytes(rng, 32) for _ in range(n_streams + 3)]
    one = lambda: (LAST, _rng_bytes(rng, int(rng.integers(0, 6))))
    parts = [[one() for _ in range(63 - i)] + [(MORE, _rng_bytes(rng, 3)), (LAST, _rng_bytes(rng, 4))] +
             [one() for _ in range(i)] for i in range(n_streams)]
    routes = [[0, 1, 2, 0]] * n_streams
    return _zmtp_case(precoms, parts, routes, [n_streams + t for t in range(3)], 65, [1] * (n_streams + 3))


@pytest.mark.gpu
@pytest.mark.parametrize("n_streams", [1, 2])
def test_tile_seams(torch_cuda, C, n_streams):
    """N just above one count tile (260 pairs) and above two (520).  The last
    stream's two-part message has its first part at the end of one tile and its
    last part at the start of the next.  That delivery's rank counts the deliveries of every earlier tile; the
    credit falls on it from both sides: destination 1 has exactly its rank (it
    is the first one refused), destination 2 one more (it is the last one
    admitted), destination 0, named twice, is cut between its two copies."""
    T = _tile()
    c = _seam_case(n_streams)
    N = n_streams * 65 * 4
    i = n_streams - 1
    first = i * 260 + (63 - i) * 4       # the seam message's first pair
    assert T == 256 and N > n_streams * T and N < (n_streams + 1) * T
    assert first // T == n_streams - 1 and (first + 4) // T == n_streams and (first + 4) % T == 0
    rank = i * 64 + 63 - i               # deliveries of destination 1 (or 2) before the seam message
    credit = [2 * rank + 1, rank, rank + 1]
    m, got = _run(torch_cuda, C, c, STATIC, credit)
    assert m["N"] == N
    D = 64 * n_streams
    assert got["taken"] == credit and got["dropped"] == [2 * D - credit[0], D - rank, D - rank - 1]
    assert [m["hwm"][first + k] for k in range(8)] == [False, True, False, True] * 2
    assert got["dst_results"][2]["frames"] == 65 * i + (63 - i) + 2
    assert got["dst_results"][1]["frames"] == 65 * i + 63 - i


# 8 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_fit_with_credits(torch_cuda, C):
    """out_bytes short by one frame: destination 2's last admitted pair does
    not fit and is ZMQG_ERR_BOUND; dst_taken still counts its delivery."""
    c = _values_case()
    credit = [UNL, 0, 4]
    full = _model(c, STATIC, ZMTP, ZMTP, credit)
    mine = [p for p in range(full["N"]) if full["frame_stream"][p] == 2]
    cap = full["enc"]["frame_off"][mine[-1]] + 1
    size = full["total"] + PAD
    m = _model(c, STATIC, ZMTP, ZMTP, credit, out_bytes=cap, out_size=size)
    got = _credit(torch_cuda, C, c, STATIC, ZMTP, ZMTP, m["N"], credit, cap, size)
    _compare(got, m, c)
    assert got["pair_status"][mine[-1]] == C.ERR_BOUND and got["pair_status"][mine[-2]] == 0
    assert got["taken"] == [6, 0, 4] and got["dropped"] == [0, 6, 2]
    assert got["dst_results"][2]["error"] == errno.ENOBUFS and got["dst_results"][2]["frames"] == len(mine) - 1
    assert got["send"][5] == c["send"][5] + len(mine) - 1


# 9 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_websocket_on_both_sides(torch_cuda, C):
    """Masked WebSocket on both sides: a ping ends stream 1's parse between two
    messages; the masks stay indexed by pair p, cleared pairs between live ones."""
    rng = np.random.default_rng(9109)
    precoms = [_rng_bytes(rng, 32) for _ in range(4)]
    pay = lambda n: _rng_bytes(rng, n)
    f0 = TG._ws_stream(rng, precoms[0], [(LAST, pay(10)), (MORE, pay(130)), (LAST, pay(3)), (LAST, pay(5))], True)
    f1 = TG._ws_stream(rng, precoms[1], [(LAST, pay(20)), (LAST, pay(21))], True)
    ping = W.frame(b"PING", 0x0badf00d, opcode=W.OP_PING)
    streams = [b"".join(f0), f1[0] + ping + f1[1]]
    c = _case(precoms, [0, 1], streams, [[0, 1], [1, 0]], [2, 3], 4, [1, 1, 5, 2 ** 32 - 3])
    N = 16
    mask = TG._mask_of(N)
    m, got = _run(torch_cuda, C, c, STATIC, [2, 1], recv=WSM, send=WSM, mask=mask)
    assert [r["frames"] for r in got["results"]] == [4, 1] and got["results"][1]["ctl_opcode"] == W.OP_PING
    assert got["taken"] == [2, 1] and got["dropped"] == [2, 3]
    live = [p for p in range(N) if m["frame_stream"][p] != F.NO_STREAM]
    assert live == [0, 1, 2, 4] and sum(m["hwm"]) == 6
    for p in live:  # the key on the wire is the pair's own
        hdr = m["enc"]["hdr"][p] - 1 - 4
        a = got["pair_off"][p] + hdr
        assert got["out"][a:a + 4].tobytes() == W.key_bytes(mask[p])


# 10 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_consume_over_two_calls(torch_cuda, C):
    """One ctx, two calls on the same device credits: the second call sees what
    the first left, unlimited stays unlimited; without the flag dst_credit is
    bit-identical after the call."""
    torch = torch_cuda
    c1 = _values_case()
    credit = [8, UNL, 3]
    m1 = _model(c1, STATIC, ZMTP, ZMTP, credit, consume=True)
    ctx = _ctx(C, c1)
    g1 = _credit(torch, C, c1, STATIC, ZMTP, ZMTP, m1["N"], credit, m1["cap"], m1["size"], consume=True, ctx=ctx)
    _compare(g1, m1, c1)
    assert g1["credit"] == [2, UNL, 0] and g1["taken"] == [6, 6, 3]
    # the same streams again, sealed with the nonces that follow
    c2 = dict(c1, peer=m1["recv"]["peer"], send=m1["enc"]["send"])
    rng = np.random.default_rng(9110)
    parts = [[(LAST, _rng_bytes(rng, 5)), (LAST, _rng_bytes(rng, 6)), (LAST, _rng_bytes(rng, 7))]] * 3
    nonce0 = [p - PEER0 + 3 for p in m1["recv"]["peer"][:3]]
    streams = [b"".join(F.source_frames(c1["precoms"][s], parts[s], nonce0[s])) for s in range(3)]
    arena, offs = F.arena_of(streams)
    c2.update(arena=arena, offs=offs, lens=[len(s) for s in streams])
    m2 = _model(c2, STATIC, ZMTP, ZMTP, g1["credit"], consume=True)
    assert [f["forwarded"] for f in m2["fwd"]] == [3, 3, 3]
    g2 = _credit(torch, C, c2, STATIC, ZMTP, ZMTP, m2["N"], None, m2["cap"], m2["size"], consume=True, ctx=ctx,
                 d_credit=g1["d_credit"])
    _compare(g2, m2, c2)
    assert g2["taken"] == [2, 9, 0] and g2["dropped"] == [7, 0, 9] and g2["credit"] == [0, UNL, 0]
    ctx.close()
    # without the flag
    m3 = _model(c1, STATIC, ZMTP, ZMTP, credit)
    g3 = _credit(torch, C, c1, STATIC, ZMTP, ZMTP, m3["N"], credit, m3["cap"], m3["size"])
    _compare(g3, m3, c1)
    assert g3["credit"] == credit and g3["taken"] == g1["taken"]


# 11 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", [STATIC, SUB, ROUTER])
def test_unlimited_is_the_framed_call(torch_cuda, C, mode):
    """Every credit unlimited: every output is zmqg_forward_framed_multi's, run
    on a second ctx with the same sessions, and nothing is dropped."""
    precoms, parts = TG._modes_parts()
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in enumerate(parts)]
    c = _case(precoms, [0, 1, 2], streams, TG.MODES_ROUTES, [3, 4, 5], 4, TG.MODES_SEND)
    kw = TG._mode_kw(mode, TFR._park(c, TG.IDS))
    m, got = _run(torch_cuda, C, c, mode, [UNL] * 3, consume=True, **kw)
    assert sum(got["taken"]) > 0 and got["dropped"] == [0, 0, 0] and got["credit"] == [UNL] * 3
    fm = TG._model(c, mode, ZMTP, ZMTP, **kw)
    framed = TG._framed(torch_cuda, C, c, mode, ZMTP, ZMTP, fm["N"], fm["cap"], fm["size"], **kw)
    for k in ("results", "peer", "send", "fwd", "pair_off", "pair_status", "dst_results") + TG.PLAN_OUT[mode]:
        assert got[k] == framed[k], k
    for k in TF.RECV_KEYS + ("out",):
        assert got[k].shape == framed[k].shape and (got[k] == framed[k]).all(), k


# 12 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_no_pairs(torch_cuda, C):
    """N == 0 with destinations: dst_taken and dst_dropped are zero-filled, dst_credit is not written."""
    precoms, parts = TG._modes_parts()
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in enumerate(parts)]
    c = _case(precoms, [0, 1, 2], streams, [[], [], []], [3, 4, 5], 4, TG.MODES_SEND)
    m, got = _run(torch_cuda, C, c, STATIC, [0, 5, UNL], consume=True)
    assert m["N"] == 0 and got["taken"] == [0, 0, 0] and got["dropped"] == [0, 0, 0] and got["credit"] == [0, 5, UNL]
    assert got["pair_off"] == [0]


# 13 -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _wide_case():
    """One stream of two one-part messages at max_frames 33 with 4,096 routes
    among 8,192 destinations (three sessions behind them): 135,168 pairs.  Route
    slots k and k + 256 of every block of 512 name one destination."""
    rng = np.random.default_rng(9113)
    precoms = [_rng_bytes(rng, 32) for _ in range(4)]
    parts = [[(LAST, _rng_bytes(rng, 3)), (LAST, _rng_bytes(rng, 2))]]
    routes = [[2 * ((k // 512) * 256 + k % 256) for k in range(4096)]]
    return _zmtp_case(precoms, parts, routes, [1 + t % 3 for t in range(8192)], 33, [1, 5, 6, 7])


@pytest.mark.gpu
def test_tiles_of_two_rounds(torch_cuda, C):
    """Where 256-pair tiles would make a table of more than 4 Mi counts the tile
    doubles, and a tile is walked in two rounds of 256 pairs: a destination's
    two copies of a message lie in one tile, a round apart, and its credit of
    1, 2 or 3 falls between them, or between the messages."""
    c = _wide_case()
    T, N, D = _tile(), 33 * 4096, 8192
    assert (N + T - 1) // T * D > 4 << 20 and (N + 2 * T - 1) // (2 * T) * D <= 4 << 20
    credit = [1 + t % 3 for t in range(D)]
    m, got = _run(torch_cuda, C, c, STATIC, credit)
    named = sorted(set(c["routes"][0]))
    assert m["N"] == N and len(named) == 2048
    assert all(got["taken"][t] == credit[t] and got["dropped"][t] == 4 - credit[t] for t in named)
    assert sum(got["taken"]) == sum(credit[t] for t in named)
    assert sum(got["dropped"]) == sum(4 - credit[t] for t in named)
    # destinations 0, 4 and 2 with credits 1, 2 and 3: the verdict on (message 0, message 1) in each of their two slots
    want = {0: [False, True], 256: [True, True], 2: [False, True], 258: [False, True], 1: [False, False],
            257: [False, True]}
    for k, w in want.items():
        assert [m["hwm"][q * 4096 + k] for q in (0, 1)] == w, k
