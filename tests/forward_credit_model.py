"""Pure-Python model of zmqg_forward_credit_multi's contract
(include/zmqg_curve.h) -- test infrastructure, not a test.  It is a post-pass
over tests/forward_framed_model.py's plan: the deliveries are read off the
plan's pairs as the header states them (position p0, destination, pair order),
the i-th delivery of a destination is admitted iff i < credit, the live pairs of
a refused delivery are cleared, and the existing send models run over what is
left.  A cleared pair reports ERR_HWM where the send model says ERR_SESSION."""
import numpy as np

from oracle import oracle as O
from tests import forward_framed_model as FM
from tests import forward_model as F
from tests import forward_router_model as FR
from tests import forward_sub_model as FS
from tests import ws_send_model as WS
from tests import zmtp_send_model as M

ZMTP, WS_PLAIN, WS_MASKED = FM.ZMTP, FM.WS_PLAIN, FM.WS_MASKED
STATIC, SUB, ROUTER, LB = FM.STATIC, FM.SUB, FM.ROUTER, FM.LB
UNLIMITED = 0xFFFFFFFF   # ZMQG_CREDIT_UNLIMITED
ERR_HWM = 0x7A000003     # ZMQG_ERR_HWM
NO_STREAM = F.NO_STREAM


def pair_space(mode, kw):
    """(m, one_route) of the mode's pair space: m = 2 with id slots (ROUTER_PREPEND alone), d' = 1 with ROUTE."""
    fl = kw.get("flags", 0) if mode == ROUTER else 0
    return (2 if fl & FR.PREPEND and not fl & FR.ROUTE else 1), bool(fl & FR.ROUTE)


def seq_flags(recv, carry, max_frames):
    """Q(s)'s msg_t flags per stream: the carried parts, then the returned frames."""
    return [[int(e[2]) for e in carry[s]] +
            [int(recv["flags"][s * max_frames + j]) for j in range(r["frames"])]
            for s, r in enumerate(recv["results"])]


def deliveries(m, mode, kw, carry, routes, max_frames):
    """{p0: (destination, [live pairs])} of a plan: every live pair belongs to
    the delivery at base(s) + slot0 * d'(s) + k, slot0 the first slot of its
    element's message."""
    mm, one_route = pair_space(mode, kw)
    fl = seq_flags(m["recv"], carry, max_frames)
    head = [FS.heads(fl[s], m["fwd"][s]["held_first"]) for s in range(len(fl))]
    out = {}
    for p, pr in enumerate(m["pairs"]):
        s, q, k, live = pr[:4]
        if not live:
            continue
        d = 1 if one_route else len(routes[s])
        p0 = m["base"][s] + mm * head[s][q] * d + k
        t = m["frame_stream"][p]
        assert p0 <= p and out.setdefault(p0, (t, []))[0] == t  # one destination per delivery
        out[p0][1].append(p)
    return out


def admit(m, mode, kw, carry, routes, max_frames, credit, consume):
    """The pass: dict(frame_stream, flags, lens, payloads, hwm, taken, dropped,
    credit_after) for the plan m and credit[t] per destination."""
    n_dst = len(credit)
    fs, fl, ln, pay = list(m["frame_stream"]), list(m["flags"]), list(m["lens"]), list(m["payloads"])
    hwm, seen = [False] * m["N"], [0] * n_dst
    taken, dropped = [0] * n_dst, [0] * n_dst
    dl = deliveries(m, mode, kw, carry, routes, max_frames)
    for p0 in sorted(dl):
        t, mine = dl[p0]
        i, seen[t] = seen[t], seen[t] + 1
        if credit[t] == UNLIMITED or i < credit[t]:
            taken[t] += 1
            continue
        dropped[t] += 1
        for p in mine:
            fs[p], fl[p], ln[p], pay[p], hwm[p] = NO_STREAM, 0, 0, b"", True
    after = [c if c == UNLIMITED or not consume else c - k for c, k in zip(credit, taken)]
    return dict(frame_stream=fs, flags=fl, lens=ln, payloads=pay, hwm=hwm, taken=taken, dropped=dropped,
                credit_after=after)


def model(mode, recv_fr, send_fr, credit, precoms, downgrade, arena, offs, lens, sids, peer, max_msg, max_frames, carry,
          plain, dst_sid, send, out_bytes, out_size, routes=None, mask=None, consume=False, encode=True, **kw):
    """The whole call: forward_framed_model.model's arguments with credit[t]
    in front.  Returns its dict with the pairs' frames after the pass, enc the
    send model's over them (status ERR_HWM at a cleared pair), and hwm, taken,
    dropped, credit_after."""
    assert mode != LB
    m = FM.model(mode, recv_fr, send_fr, precoms, downgrade, arena, offs, lens, sids, peer, max_msg, max_frames, carry,
                 plain, dst_sid, send, None, 0, routes=routes, mask=mask, encode=False, **kw)
    a = admit(m, mode, kw, carry, routes, max_frames, [int(x) for x in credit], consume)
    N = m["N"]
    args = (precoms, downgrade, dst_sid, a["frame_stream"], None, a["flags"], a["lens"], a["payloads"])
    pre = dict(send=send, enc_prefix=O.SERVER_PREFIX, dec_prefix=O.CLIENT_PREFIX)
    if send_fr == ZMTP:
        enc_of = lambda cap, size, enc: M.model(*args, cap, size, encode=enc, **pre)
    else:
        keys = [int(x) for x in mask] if send_fr == WS_MASKED else None
        assert keys is None or len(keys) == N
        enc_of = lambda cap, size, enc: WS.model(*args, keys, cap, size, encode=enc, **pre)
    total = enc_of(2 ** 62, 0, False)["frame_off"][-1] if len(dst_sid) else 0
    cap = total if out_bytes is None else out_bytes
    size = out_size if out_bytes is not None else total + out_size
    if len(dst_sid):
        enc = enc_of(cap, size, encode)
        enc["status"] = [ERR_HWM if h else s for s, h in zip(enc["status"], a["hwm"])]
    else:
        enc = dict(out=np.full(size, M.SENTINEL, np.uint8), frame_off=[0], status=[], results=[],
                   send=[int(x) for x in send])
    out = dict(m)
    out.update(a)
    out.update(enc=enc, total=total, cap=cap, size=size)
    return out
