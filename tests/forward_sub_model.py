"""Pure-Python model of zmqg_forward_zmtp_sub_multi's contract
(include/zmqg_curve.h) -- test infrastructure, not a test.  The receive side,
the rule of what is forwarded and the pair layout are tests/forward_model.py's
(receive, rule, pair_base); heads and topics are stated element by element;
the match is a plain topic.startswith(prefix) over the destination's list; the
send side is tests/zmtp_send_model.py's model over the pairs."""
from tests import forward_model as F
from tests import zmtp_send_model as M

MORE, COMMAND = F.MORE, F.COMMAND
NO_STREAM = F.NO_STREAM


def heads(flags, held_first):
    """flags: Q(s)'s msg_t flags in order.  Returns, per element, the index of
    its message's head, or None for a command or an element at or behind
    held_first: the data elements are the non-command elements below
    held_first; the first one is a head, and so is every one whose
    predecessor among them has MORE clear."""
    out, head, prev_more = [None] * len(flags), None, False
    for q in range(min(held_first, len(flags))):
        if flags[q] & COMMAND:
            continue
        if head is None or not prev_more:
            head = q
        out[q] = head
        prev_more = bool(flags[q] & MORE)
    return out


def matches(prefixes, topic, invert=False):
    """One destination's verdict on a topic: some prefix of its list starts the topic."""
    return any(topic.startswith(p) for p in prefixes) != bool(invert)


def table_view(sub_idx, sub_off, sub_len, sub_bytes, n_dst, n_subs=None, sub_bytes_len=None):
    """What the call makes of a table it cannot trust, as lists of bytes by
    destination: sub_idx entries clamped to n_subs, a falling pair an empty
    range, a subscription that runs past sub_bytes_len dropped (it never
    matches)."""
    n_subs = len(sub_off) if n_subs is None else n_subs
    sub_bytes_len = len(sub_bytes) if sub_bytes_len is None else sub_bytes_len
    raw = bytes(bytearray(sub_bytes))
    out = []
    for t in range(n_dst):
        lo, hi = min(int(sub_idx[t]), n_subs), min(int(sub_idx[t + 1]), n_subs)
        out.append([raw[int(sub_off[j]):int(sub_off[j]) + int(sub_len[j])] for j in range(lo, max(lo, hi))
                    if int(sub_off[j]) + int(sub_len[j]) <= sub_bytes_len])
    return out


def model(precoms, downgrade, arena, offs, lens, sids, peer, max_msg, max_frames, carry, plain, dst_sid, routes,
          send, subs, out_bytes, out_size, invert=False, enc_prefix=F.O.SERVER_PREFIX, dec_prefix=F.O.CLIENT_PREFIX,
          encode=True):
    """forward_model.model's arguments plus subs[t] = destination t's prefixes
    (bytes).  Returns the same dict, `pairs` and the encode over the live
    pairs of this call, plus match[p] (match_out), topics[s][q] (the topic of
    every head) and head[s][q]."""
    S = len(offs)
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
    base = F.pair_base([len(c) for c in carry], [len(r) for r in routes], max_frames)
    N = base[-1]

    def payload(s, q):  # a returned frame's payload is what the receive side decoded; a carried part's is in plain
        _, _, off, ln = elems[s][q]
        return (src if q < len(carry[s]) else recv["out"])[off:off + ln].tobytes()

    head = [heads([e[0] for e in elems[s]], fwd[s]["held_first"]) for s in range(S)]
    topics = [{h: payload(s, h) for h in set(head[s]) if h is not None} for s in range(S)]
    frame_stream, flags, lens_p, payloads, pairs, match = [], [], [], [], [], []
    for s in range(S):
        for q in range(len(carry[s]) + max_frames):
            forwarded = q < fwd[s]["seq"] and fwd[s]["live"][q]
            for k, dst in enumerate(routes[s]):
                live = forwarded and matches(subs[dst], topics[s][head[s][q]], invert)
                pairs.append((s, q, k, live))
                match.append(int(live))
                if live:
                    frame_stream.append(dst), flags.append(elems[s][q][0] & MORE), lens_p.append(elems[s][q][3])
                    payloads.append(payload(s, q))
                else:
                    frame_stream.append(NO_STREAM), flags.append(0), lens_p.append(0), payloads.append(b"")
    assert len(pairs) == N
    enc = M.model(precoms, downgrade, dst_sid, frame_stream, None, flags, lens_p, payloads, out_bytes, out_size,
                  send=send, enc_prefix=enc_prefix, dec_prefix=dec_prefix, encode=encode)
    return dict(recv=recv, fwd=fwd, base=base, N=N, pairs=pairs, enc=enc, frame_stream=frame_stream, flags=flags,
                lens=lens_p, payloads=payloads, match=match, topics=topics, head=head)
