"""Pure-Python model of zmqg_subs_update_multi's contract (include/zmqg_curve.h)
-- test infrastructure, not a test.  The input is the model of
zmqg_decode_zmtp_multi's outputs that tests/forward_model.py's receive()
returns (or craft()'s, the same dict made by hand, without crypto); the store is
numpy arrays laid out as the call's; the whole call is a replay, one event at a
time: the clears in clear_dst order, then the elements in (stream, slot) order,
H counted over the store as it stands just before each event."""
import numpy as np

MORE, COMMAND, SUBSCRIBE, CANCEL = 1, 2, 12, 16  # ZMQG_MSG_*
NONE, ADDED, DUPLICATE, REMOVED, NOT_FOUND, FULL, TOO_LONG = range(7)  # ZMQG_SUB_*
VERBOSE, VERBOSER = 2, 4  # ZMQG_SUBS_*
NO_NOTE = 0xFFFFFFFF
MAX_DST = 8192


def classify(p, flags):
    """(ZMQG_MSG_SUBSCRIBE / ZMQG_MSG_CANCEL / 0, where the topic starts) for
    payload p with msg_t flags `flags`."""
    if flags & COMMAND:
        if p[:10] == b"\x09SUBSCRIBE":
            return SUBSCRIBE, 10
        if p[:7] == b"\x06CANCEL":
            return CANCEL, 7
        return 0, 0
    if len(p) >= 1 and p[0] in (0, 1):
        return (SUBSCRIBE if p[0] else CANCEL), 1
    return 0, 0


def empty_store(n_dst, cap, slot_bytes):
    return dict(n_dst=n_dst, cap=cap, slot_bytes=slot_bytes, cnt=np.zeros(n_dst, np.uint32),
                slot_len=np.zeros(n_dst * cap, np.uint32), bytes=np.zeros(n_dst * cap * slot_bytes, np.uint8))


def store_of(prefixes, cap, slot_bytes):
    """The store that holds prefixes[t] for destination t, in order."""
    st = empty_store(len(prefixes), cap, slot_bytes)
    for t, d in enumerate(prefixes):
        assert len(d) <= cap
        st["cnt"][t] = len(d)
        for i, p in enumerate(d):
            assert len(p) <= slot_bytes
            g = t * cap + i
            st["slot_len"][g] = len(p)
            st["bytes"][g * slot_bytes:g * slot_bytes + len(p)] = np.frombuffer(p, np.uint8)
    return st


def _count(st, t):
    return min(int(st["cnt"][t]), st["cap"])


def _slot(st, g):
    n = min(int(st["slot_len"][g]), st["slot_bytes"])
    return st["bytes"][g * st["slot_bytes"]:g * st["slot_bytes"] + n].tobytes()


def prefixes(st):
    """The store as the device reads it: a list of bytes per destination."""
    return [[_slot(st, t * st["cap"] + i) for i in range(_count(st, t))] for t in range(st["n_dst"])]


def holders(st, topic):
    """The live slots, over all destinations, that hold exactly `topic`."""
    return sum(p == topic for d in prefixes(st) for p in d)


def craft(streams, max_frames, frames=None, lead=1):
    """zmqg_decode_zmtp_multi's outputs, made by hand: streams[s] = [(msg_t
    flags, payload, status)], at most max_frames each; frames[s] overrides
    results[s].frames.  Every payload sits at an odd offset of `out`, junk
    between the payloads.  The dict is forward_model.receive()'s."""
    S = len(streams)
    slots = S * max_frames
    f_off, f_len = np.zeros(slots, np.uint64), np.zeros(slots, np.uint32)
    status, flags = np.full(slots, 0x10000011, np.int64), np.zeros(slots, np.uint8)  # (padding: empty, malformed)
    buf, results = bytearray(b"\xA5" * lead), []
    for s, st in enumerate(streams):
        assert len(st) <= max_frames
        for j, (fl, p, bad) in enumerate(st):
            if len(buf) % 2 == 0:
                buf += b"\x5A"
            k = s * max_frames + j
            f_off[k], f_len[k], status[k], flags[k] = len(buf), len(p) + 33, bad, fl
            buf += p
        results.append(dict(frames=len(st) if frames is None else frames[s], consumed=0, error=0, out_bytes=0))
    buf += b"\x5A" * 8
    return dict(results=results, f_off=f_off, f_len=f_len, status=status, flags=flags,
                out=np.frombuffer(bytes(buf), np.uint8).copy())


def invalid(n_dst, cap, slot_bytes, n_streams, max_frames, stream_dst, clear_dst, flags=0):
    """The contract's -EINVAL cases that depend on values (not on null pointers)."""
    if flags & ~(VERBOSE | VERBOSER):
        return True
    if n_dst > MAX_DST or cap < 1 or slot_bytes % 8 or not 8 <= slot_bytes <= 65536 or n_dst * cap > 2 ** 31 - 1:
        return True
    if max(n_streams, max_frames, n_streams * max_frames) > 2 ** 31 - 1:
        return True
    named = list(stream_dst) + list(clear_dst)
    return len(set(named)) != len(named) or any(t >= n_dst for t in named)


def update(store, recv, max_frames, stream_dst, clear_dst=(), flags=0):
    """The whole call.  store: empty_store()'s dict (not modified); recv:
    receive()'s or craft()'s dict.  Returns dict(store (the new one), sub_idx,
    sub_off, sub_len (the view's entries below sub_idx[-1]), sub_status,
    topic_off, topic_len, note_flags, note_stream (per slot), results (per
    stream), clear_cnt, clear_len and clear_note ({store slot: value}), notes
    (the notifications in event order: (subscribe?, topic))."""
    assert not invalid(store["n_dst"], store["cap"], store["slot_bytes"], len(stream_dst), max_frames, stream_dst,
                       clear_dst, flags)
    st = dict(store, cnt=store["cnt"].copy(), slot_len=store["slot_len"].copy(), bytes=store["bytes"].copy())
    cap, sb = st["cap"], st["slot_bytes"]
    verbose, verboser = bool(flags & (VERBOSE | VERBOSER)), bool(flags & VERBOSER)
    notes = []

    def put(g, p):
        st["slot_len"][g] = len(p)
        st["bytes"][g * sb:g * sb + len(p)] = np.frombuffer(p, np.uint8)

    clear_cnt, clear_len, clear_note = [], {}, {}
    for t in clear_dst:
        c = _count(st, t)
        clear_cnt.append(c)
        held = [_slot(st, t * cap + i) for i in range(c)]
        for i, p in enumerate(held):
            st["cnt"][t] = 0  # the destination holds slots i .. c - 1 now: count them by hand
            H = holders(st, p) + sum(q == p for q in held[i:])
            clear_len[t * cap + i] = len(p)
            clear_note[t * cap + i] = int(verboser or H == 1)
            if clear_note[t * cap + i]:
                notes.append((False, p))
        st["cnt"][t] = 0

    S = len(stream_dst)
    n = S * max_frames
    sub_status, topic_off, topic_len = np.zeros(n, np.int32), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    note_flags, note_stream = np.zeros(n, np.uint8), np.full(n, NO_NOTE, np.uint32)
    results = []
    for s, t in enumerate(stream_dst):
        res = dict(seen=0, changed=0, notes=0, rejected=0)
        c = _count(st, t)
        st["cnt"][t] = c
        for j in range(min(recv["results"][s]["frames"], max_frames)):
            k = s * max_frames + j
            if recv["status"][k] != 0:
                break
            off, ln = int(recv["f_off"][k]), int(recv["f_len"][k]) - 33
            kind, skip = classify(recv["out"][off:off + ln].tobytes(), int(recv["flags"][k])) if ln >= 0 else (0, 0)
            if not kind:
                continue
            topic = recv["out"][off + skip:off + ln].tobytes()
            topic_off[k], topic_len[k], note_flags[k] = off + skip, ln - skip, kind
            res["seen"] += 1
            H = holders(st, topic)
            mine = [_slot(st, t * cap + i) for i in range(c)]
            hit = mine.index(topic) if topic in mine else -1
            if kind == SUBSCRIBE:
                if len(topic) > sb:
                    status, note = TOO_LONG, False
                elif hit >= 0:
                    status, note = DUPLICATE, verbose
                elif c == cap:
                    status, note = FULL, False
                else:
                    put(t * cap + c, topic)
                    c += 1
                    status, note = ADDED, verbose or H == 0
            elif hit < 0:
                status, note = NOT_FOUND, True  # (rm_result != values_remain, src/xpub.cpp:118-122)
            else:
                if hit != c - 1:
                    put(t * cap + hit, mine[c - 1])
                c -= 1
                status, note = REMOVED, verboser or H == 1
            st["cnt"][t] = c
            sub_status[k] = status
            res["changed"] += status in (ADDED, REMOVED)
            res["rejected"] += status in (FULL, TOO_LONG)
            if note:
                note_stream[k] = 0
                res["notes"] += 1
                notes.append((kind == SUBSCRIBE, topic))
        results.append(res)

    counts = [_count(st, t) for t in range(st["n_dst"])]
    sub_idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    sub_off = np.array([(t * cap + i) * sb for t in range(st["n_dst"]) for i in range(counts[t])], np.uint64)
    sub_len = np.array([min(int(st["slot_len"][t * cap + i]), sb) for t in range(st["n_dst"])
                        for i in range(counts[t])], np.uint32)
    return dict(store=st, sub_idx=sub_idx, sub_off=sub_off, sub_len=sub_len, sub_status=sub_status,
                topic_off=topic_off, topic_len=topic_len, note_flags=note_flags, note_stream=note_stream,
                results=results, clear_cnt=clear_cnt, clear_len=clear_len, clear_note=clear_note, notes=notes)
