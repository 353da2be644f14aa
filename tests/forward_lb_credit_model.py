"""Pure-Python model of zmqg_forward_lb_credit_multi's contract
(include/zmqg_curve.h) -- test infrastructure, not a test.  The plan is
tests/forward_lb_model.py's, through tests/forward_framed_model.py for the
framings, without its encode; the choice is made again with the header's loop,
taken literally, message by message; the pairs, dest, a hwm list, taken /
dropped / credit_after and lb_cur are rebuilt from it, and
forward_framed_model's send side runs over what is left.

The payload of a slot does not depend on where its message goes, so it is taken
from a second run of the plan over a table whose every entry names destination
0: there every slot that can ever be live is live."""
import numpy as np

from oracle import oracle as O
from tests import forward_framed_model as FM
from tests import forward_lb_model as FL
from tests import forward_model as F
from tests import ws_send_model as WS
from tests import zmtp_send_model as M

ZMTP, WS_PLAIN, WS_MASKED = FM.ZMTP, FM.WS_PLAIN, FM.WS_MASKED
UNLIMITED = 0xFFFFFFFF   # ZMQG_CREDIT_UNLIMITED
ERR_HWM = 0x7A000003     # ZMQG_ERR_HWM
NO_STREAM = F.NO_STREAM
NO_GROUP, NONE, NO_PEER = FL.NO_GROUP, FL.NONE, FL.NO_PEER
REFUSED = "refused"


def choose(ring, credit, cur, n_msgs):
    """The header's loop over one group: ring = the destinations R[0 .. A0),
    credit[t] per destination, cur = cur0.  Returns (picks, lb_cur): per
    message the original ring position that took it, or REFUSED, and the
    original position of the entry the cursor points at (0 when A ended at 0)."""
    n_dst = len(credit)
    orig = list(range(len(ring)))
    w = [credit[t] if t < n_dst else UNLIMITED for t in ring]
    A, picks = len(ring), []
    for _ in range(n_msgs):
        took = REFUSED
        while A > 0:
            if w[cur] == UNLIMITED or w[cur] > 0:
                took = orig[cur]
                if w[cur] != UNLIMITED:
                    w[cur] -= 1
                cur += 1
                if cur >= A:
                    cur = 0
                break
            A -= 1
            if cur < A:
                orig[cur], orig[A] = orig[A], orig[cur]
                w[cur], w[A] = w[A], w[cur]
            else:
                cur = 0
        picks.append(took)
    return picks, (orig[cur] if A else 0)


def model(recv_fr, send_fr, credit, precoms, downgrade, arena, offs, lens, sids, peer, max_msg, max_frames, carry, plain,
          dst_sid, send, out_bytes, out_size, flags=0, src_ids=None, stream_group=None, table=None, mask=None,
          consume=False, encode=True):
    """The whole call: forward_framed_model.model's arguments for the LB mode
    with credit[t] in front.  Returns its dict with the pairs' frames under the
    credits, dest, lb_cur, picks[g] (per message of group g the original ring
    position, or REFUSED), enc the send model's over them (status ERR_HWM at a
    refused message's pairs), and hwm, sent (X), taken, dropped, credit_after."""
    credit = [int(x) for x in credit]
    n_dst, S, G = len(dst_sid), len(offs), len(table["lb_cur"])
    assert len(credit) == n_dst
    run = lambda t: FM.model(FM.LB, recv_fr, send_fr, precoms, downgrade, arena, offs, lens, sids, peer, max_msg,
                             max_frames, carry, plain, dst_sid, send, None, 0, mask=mask, encode=False, flags=flags,
                             src_ids=src_ids, stream_group=stream_group, table=t)
    m = run(table)
    probe = run(dict(table, lb_dst=[0] * len(table["lb_dst"])))
    assert probe["pairs"] == [pr[:3] + (d == 0 and n_dst > 0, pr[4]) for pr, d in zip(m["pairs"], probe["dest"])]
    # the choice, group by group: the messages by rising stream, then rising head
    msgs = [[] for _ in range(G)]
    for s in range(S):
        g = int(stream_group[s])
        if g != NO_GROUP:
            msgs[g] += [(s, h) for h in sorted(set(x for x in m["head"][s] if x is not None))]
    chosen, picks, lb_cur, sent = {}, [], [], [0] * n_dst
    for g in range(G):
        lo, A0 = FL.group_range(table, g)
        ring = [int(x) for x in table["lb_dst"][lo:lo + A0]]
        pk, cur = choose(ring, credit, FL.cur0(table, g), len(msgs[g]) if A0 else 0)
        picks.append(pk)
        lb_cur.append(cur)
        for (s, h), j in zip(msgs[g], pk):
            chosen[s, h] = REFUSED if j == REFUSED else ring[j]
            if j != REFUSED and ring[j] < n_dst:
                sent[ring[j]] += 1
    fs, fl, ln, pay, dest, hwm, pairs = [], [], [], [], [], [], []
    for p, (s, q, k, _, is_id) in enumerate(m["pairs"]):
        t = NONE
        if probe["dest"][p] == 0:  # a slot of a message in a group with a ring
            t = chosen[s, m["head"][s][q]]
        elif m["dest"][p] != NONE:  # forwarded, without a group or with an empty range
            assert m["dest"][p] == NO_PEER
            t = NO_PEER
        refused = t == REFUSED
        live = not refused and t < n_dst
        pairs.append((s, q, k, live, is_id))
        hwm.append(refused)
        dest.append(t if live else NONE if t == NONE else NO_PEER)
        fs.append(t if live else NO_STREAM)
        fl.append(probe["flags"][p] if live else 0)
        ln.append(probe["lens"][p] if live else 0)
        pay.append(probe["payloads"][p] if live else b"")
    taken = [x if c == UNLIMITED else min(x, c) for x, c in zip(sent, credit)]
    dropped = [x - k for x, k in zip(sent, taken)]
    after = [c if c == UNLIMITED or not consume else c - k for c, k in zip(credit, taken)]
    N = m["N"]
    args = (precoms, downgrade, dst_sid, fs, None, fl, ln, pay)
    pre = dict(send=send, enc_prefix=O.SERVER_PREFIX, dec_prefix=O.CLIENT_PREFIX)
    if send_fr == ZMTP:
        enc_of = lambda cap, size, enc: M.model(*args, cap, size, encode=enc, **pre)
    else:
        keys = [int(x) for x in mask] if send_fr == WS_MASKED else None
        assert keys is None or len(keys) == N
        enc_of = lambda cap, size, enc: WS.model(*args, keys, cap, size, encode=enc, **pre)
    total = enc_of(2 ** 62, 0, False)["frame_off"][-1] if n_dst else 0
    cap = total if out_bytes is None else out_bytes
    size = out_size if out_bytes is not None else total + out_size
    if n_dst:
        enc = enc_of(cap, size, encode)
        enc["status"] = [ERR_HWM if h else s for s, h in zip(enc["status"], hwm)]
    else:
        enc = dict(out=np.full(size, M.SENTINEL, np.uint8), frame_off=[0], status=[], results=[],
                   send=[int(x) for x in send])
    out = dict(m)
    out.update(pairs=pairs, frame_stream=fs, flags=fl, lens=ln, payloads=pay, dest=dest, hwm=hwm, picks=picks,
               lb_cur=lb_cur, sent=sent, taken=taken, dropped=dropped, credit_after=after, enc=enc, total=total,
               cap=cap, size=size)
    return out
