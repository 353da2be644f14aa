"""Pure-Python model of zmqg_forward_zmtp_lb_multi's contract
(include/zmqg_curve.h) -- test infrastructure, not a test.  The receive side and
the rule of what is forwarded are tests/forward_model.py's (receive, rule);
heads are tests/forward_sub_model.py's; the choice is the header's arithmetic,
written as it is stated there, over a table the model trusts no more than the
device does; the send side is tests/zmtp_send_model.py's model over the pairs."""
from tests import forward_model as F
from tests import forward_sub_model as FS
from tests import zmtp_send_model as M

MORE, COMMAND = F.MORE, F.COMMAND
NO_STREAM = F.NO_STREAM
PREPEND = 1  # ZMQG_LB_PREPEND
NO_GROUP, NONE, NO_PEER = 0xffffffff, 0xffffffff, 0xfffffffd  # ZMQG_LB_*


def group_range(table, g):
    """(lo, A) of group g: grp_idx entries above n_lb clamped to it, a falling pair an empty range."""
    n_lb = table["n_lb"]
    lo, hi = min(int(table["grp_idx"][g]), n_lb), min(int(table["grp_idx"][g + 1]), n_lb)
    return lo, max(hi - lo, 0)


def cur0(table, g):
    A = group_range(table, g)[1]
    return int(table["lb_cur"][g]) % A if A else 0


def pair_base(flags, carry_counts, max_frames):
    """base(s), n_streams + 1 entries (the last is N): stream s owns m * (c(s) + max_frames) pairs."""
    m = 2 if flags & PREPEND else 1
    base = [0]
    for c in carry_counts:
        base.append(base[-1] + m * (c + max_frames))
    return base


def model(precoms, downgrade, arena, offs, lens, sids, peer, max_msg, max_frames, carry, plain, dst_sid, send, flags,
          src_ids, stream_group, table, out_bytes, out_size, enc_prefix=F.O.SERVER_PREFIX,
          dec_prefix=F.O.CLIENT_PREFIX, encode=True):
    """forward_model.model's arguments without routes, plus flags, src_ids[s] =
    (offset into plain, length) (PREPEND), stream_group[s] and table =
    dict(grp_idx, lb_dst, lb_cur, n_lb), n_groups = len(lb_cur), the arrays
    possibly longer than n_lb states.  Returns forward_model.model's dict plus
    dest (dest_out), head[s][q], msgs[g] (M(g)), picks[g] (the ring position of
    every message of the group, in order) and lb_cur, the cursors after the
    call; pairs[p] = (stream, element, 0, live, is id slot)."""
    S, n_dst, G = len(offs), len(dst_sid), len(table["lb_cur"])
    prepend = bool(flags & PREPEND)
    recv = F.receive(arena, offs, lens, sids, precoms, peer, max_msg, max_frames, dec_prefix)
    src = arena if plain is None else plain
    fwd, elems = [], []
    for s in range(S):
        q = [(int(fl), False, int(off), int(ln)) for off, ln, fl in carry[s]]
        for j in range(recv["results"][s]["frames"]):
            k = s * max_frames + j
            q.append((int(recv["flags"][k]), recv["status"][k] != 0, int(recv["f_off"][k]),
                      int(recv["f_len"][k]) - 33))
        fwd.append(F.rule([(e[0], e[1]) for e in q]))
        elems.append(q)
    base = pair_base(flags, [len(c) for c in carry], max_frames)
    N = base[-1]

    def payload(s, q):  # a returned frame's payload is what the receive side decoded; a carried part's is in plain
        _, _, off, ln = elems[s][q]
        return (src if q < len(carry[s]) else recv["out"])[off:off + ln].tobytes()

    def src_id(s):
        off, ln = src_ids[s]
        return src[off:off + ln].tobytes()

    head = [FS.heads([e[0] for e in elems[s]], fwd[s]["held_first"]) for s in range(S)]
    # the choice: the i-th message of a group, streams rising, elements rising
    count = [0] * G
    start = [cur0(table, g) for g in range(G)]
    picks = [[] for _ in range(G)]
    chosen = {}  # (s, head) -> the entry's value, or None without a group or with A = 0
    for s in range(S):
        g = int(stream_group[s])
        for h in sorted(set(x for x in head[s] if x is not None)):
            if g == NO_GROUP:
                chosen[s, h] = None
                continue
            lo, A = group_range(table, g)
            if A == 0:
                chosen[s, h] = None
            else:
                pos = (start[g] + count[g]) % A
                picks[g].append(pos)
                chosen[s, h] = int(table["lb_dst"][lo + pos])
            count[g] += 1
    lb_cur = []
    for g in range(G):
        A = group_range(table, g)[1]
        lb_cur.append((start[g] + count[g]) % A if A else 0)

    frame_stream, fl_p, lens_p, payloads, pairs, dest = [], [], [], [], [], []

    def emit(s, q, is_id, d, fl, data):
        live = d < NO_PEER
        pairs.append((s, q, 0, live, is_id))
        dest.append(d)
        frame_stream.append(d if live else NO_STREAM), fl_p.append(fl & MORE if live else 0)
        lens_p.append(len(data) if live else 0), payloads.append(data if live else b"")

    for s in range(S):
        for q in range(len(carry[s]) + max_frames):
            forwarded = q < fwd[s]["seq"] and fwd[s]["live"][q]
            d = NONE
            if forwarded:
                t = chosen[s, head[s][q]]
                d = t if t is not None and t < n_dst else NO_PEER
            if prepend:
                is_head = forwarded and head[s][q] == q
                emit(s, q, True, d if is_head else NONE, MORE, src_id(s) if is_head else b"")
            emit(s, q, False, d, elems[s][q][0] if forwarded else 0, payload(s, q) if forwarded else b"")
    assert len(pairs) == N
    enc = M.model(precoms, downgrade, dst_sid, frame_stream, None, fl_p, lens_p, payloads, out_bytes, out_size,
                  send=send, enc_prefix=enc_prefix, dec_prefix=dec_prefix, encode=encode)
    return dict(recv=recv, fwd=fwd, base=base, N=N, pairs=pairs, enc=enc, frame_stream=frame_stream, flags=fl_p,
                lens=lens_p, payloads=payloads, dest=dest, head=head, msgs=count, picks=picks, lb_cur=lb_cur)
