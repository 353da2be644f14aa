"""Pure-Python model of zmqg_forward_zmtp_router_multi's contract
(include/zmqg_curve.h) -- test infrastructure, not a test.  The receive side,
the rule of what is forwarded and the parent pair layout are
tests/forward_model.py's (receive, rule, pair_base); heads are
tests/forward_sub_model.py's; the lookup is the header's loop, written as it
is stated there, over a table the model trusts no more than the device does;
the send side is tests/zmtp_send_model.py's model over the pairs."""
from tests import forward_model as F
from tests import forward_sub_model as FS
from tests import zmtp_send_model as M

MORE, COMMAND = F.MORE, F.COMMAND
NO_STREAM = F.NO_STREAM
PREPEND, ROUTE = 1, 2  # ZMQG_ROUTER_*
NONE, ADDRESS, UNKNOWN, MALFORMED = 0xffffffff, 0xfffffffe, 0xfffffffd, 0xfffffffc  # ZMQG_ROUTE_*


def less(a, b):
    """blob_t::operator< (src/blob.hpp:92): memcmp over the shorter length
    gives < 0, or gives 0 and a is shorter."""
    n = min(len(a), len(b))
    for x, y in zip(a[:n], b[:n]):
        if x != y:
            return x < y
    return len(a) < len(b)


def entry(table, j):
    """Entry j's bytes, or None for a void entry (it orders as the empty id and equals nothing)."""
    off, ln, L = int(table["off"][j]), int(table["len"][j]), table["bytes_len"]
    if off > L or ln > L - off:
        return None
    return bytes(bytearray(table["raw"][off:off + ln]))


def lookup(table, address, n_dst):
    """table: dict(off, len, dst, raw, n_ids, bytes_len), the arrays possibly
    longer than n_ids / bytes_len state.  The destination the address names, or
    None."""
    lo, hi, n = 0, table["n_ids"], table["n_ids"]
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if less(entry(table, mid) or b"", address):
            lo = mid + 1
        else:
            hi = mid
    if lo < n and entry(table, lo) == address and int(table["dst"][lo]) < n_dst:
        return int(table["dst"][lo])
    return None


def table_of(ids_with_dst):
    """A sorted table with distinct ids from (id, destination) pairs, packed back to back."""
    rows = sorted((bytes(i), int(d)) for i, d in ids_with_dst)
    off, raw = [], bytearray()
    for i, _ in rows:
        off.append(len(raw))
        raw += i
    return dict(off=off, len=[len(i) for i, _ in rows], dst=[d for _, d in rows], raw=bytes(raw), n_ids=len(rows),
                bytes_len=len(raw))


def pair_base(flags, carry_counts, route_counts, max_frames):
    """base(s), n_streams + 1 entries (the last is N): stream s owns m * (c(s) +
    max_frames) * d'(s) pairs."""
    m = 2 if flags & PREPEND and not flags & ROUTE else 1
    base = [0]
    for c, d in zip(carry_counts, route_counts):
        base.append(base[-1] + m * (c + max_frames) * (1 if flags & ROUTE else d))
    return base


def model(precoms, downgrade, arena, offs, lens, sids, peer, max_msg, max_frames, carry, plain, dst_sid, routes,
          send, flags, src_ids, table, out_bytes, out_size, enc_prefix=F.O.SERVER_PREFIX,
          dec_prefix=F.O.CLIENT_PREFIX, encode=True):
    """forward_model.model's arguments plus flags, src_ids[s] = (offset into
    plain, length) (PREPEND) and table (ROUTE, as lookup() takes it).  plain:
    the bytes `plain` holds before the call (None: the arena); the ids are read
    there.  Returns forward_model.model's dict plus dest (dest_out) and
    head[s][q]; pairs[p] = (stream, element, route slot, live, is id slot)."""
    if not flags:
        m = F.model(precoms, downgrade, arena, offs, lens, sids, peer, max_msg, max_frames, carry, plain, dst_sid,
                    routes, send, out_bytes, out_size, enc_prefix=enc_prefix, dec_prefix=dec_prefix, encode=encode)
        m["dest"] = None
        return m
    S, n_dst = len(offs), len(dst_sid)
    prepend, route = bool(flags & PREPEND), bool(flags & ROUTE)
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
    base = pair_base(flags, [len(c) for c in carry], [len(r) for r in routes], max_frames)
    N = base[-1]

    def payload(s, q):  # a returned frame's payload is what the receive side decoded; a carried part's is in plain
        _, _, off, ln = elems[s][q]
        return (src if q < len(carry[s]) else recv["out"])[off:off + ln].tobytes()

    def src_id(s):
        off, ln = src_ids[s]
        return src[off:off + ln].tobytes()

    head = [FS.heads([e[0] for e in elems[s]], fwd[s]["held_first"]) for s in range(S)]
    frame_stream, fl_p, lens_p, payloads, pairs, dest = [], [], [], [], [], []

    def emit(s, q, k, is_id, d, fl, data):
        live = d < MALFORMED
        pairs.append((s, q, k, live, is_id))
        dest.append(d)
        frame_stream.append(d if live else NO_STREAM), fl_p.append(fl & MORE if live else 0)
        lens_p.append(len(data) if live else 0), payloads.append(data if live else b"")

    for s in range(S):
        for q in range(len(carry[s]) + max_frames):
            forwarded = q < fwd[s]["seq"] and fwd[s]["live"][q]
            is_head = forwarded and head[s][q] == q
            if not route:
                if prepend:
                    for k, dst in enumerate(routes[s]):
                        emit(s, q, k, True, dst if is_head else NONE, MORE, src_id(s))
                for k, dst in enumerate(routes[s]):
                    emit(s, q, k, False, dst if forwarded else NONE, elems[s][q][0] if forwarded else 0,
                         payload(s, q) if forwarded else b"")
                continue
            d = NONE
            if forwarded:
                h = head[s][q]
                addr_more = True if prepend else bool(elems[s][h][0] & MORE)
                if not addr_more:
                    d = MALFORMED  # (h == q: a one-part message has no other part)
                elif is_head and not prepend:
                    d = ADDRESS
                else:
                    t = lookup(table, src_id(s) if prepend else payload(s, h), n_dst)
                    d = UNKNOWN if t is None else t
            emit(s, q, 0, False, d, elems[s][q][0] if forwarded else 0, payload(s, q) if forwarded else b"")
    assert len(pairs) == N
    enc = M.model(precoms, downgrade, dst_sid, frame_stream, None, fl_p, lens_p, payloads, out_bytes, out_size,
                  send=send, enc_prefix=enc_prefix, dec_prefix=dec_prefix, encode=encode)
    return dict(recv=recv, fwd=fwd, base=base, N=N, pairs=pairs, enc=enc, frame_stream=frame_stream, flags=fl_p,
                lens=lens_p, payloads=payloads, dest=dest, head=head)
