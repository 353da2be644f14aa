"""tests/forward_router_model.py (no GPU): the model's rule against a
restatement of the reference's state machines, written as the reference
writes them -- router_t::xsend with _more_out / _current_out and a map of
peers (src/router.cpp:161-261, lookup_out_pipe, src/socket_base.cpp:2187-2200)
and the prefix of router_t::xrecv (src/router.cpp:263-332); the search against
dict lookup on sorted tables; the ordering edge cases; and the model with
flags = 0 against tests/forward_model.py's model field by field."""
import numpy as np
import pytest

from tests import forward_model as F
from tests import forward_router_model as FR
from tests.test_forward_model import _random_case

MORE, CMD, LAST = F.MORE, F.COMMAND, 0


class RouterSend:
    """router_t::xsend, ZMQ_ROUTER_MANDATORY off, no raw socket, pipes that
    never fill: what each peer's pipe is written."""

    def __init__(self, peers):
        self.out_pipes = dict(peers)  # routing id -> pipe (socket_base_t::_out_pipes, a std::map<blob_t, out_pipe_t>)
        self.more_out, self.current_out = False, None
        self.written = {p: [] for p in set(self.out_pipes.values())}

    def xsend(self, flags, data):
        if not self.more_out:  # (:165) the first part is the id of the peer to send the message to
            assert self.current_out is None  # (:166)
            if flags & MORE:  # (:171) a prefix with no subsequent message is silently ignored
                self.more_out = True  # (:172)
                self.current_out = self.out_pipes.get(data)  # (:177-182) lookup_out_pipe: _out_pipes.find (blob)
            return  # (:207-211) the address part is closed, never written
        self.more_out = bool(flags & MORE)  # (:219)
        if self.current_out is not None:  # (:222) push the message into the pipe
            self.written[self.current_out].append((flags & MORE, data))  # (:236)
            if not self.more_out:  # (:246-249)
                self.current_out = None
        # (:251-254) no out pipe: the part is dropped


class RouterRecv:
    """router_t::xrecv's prefix: what the socket's reader gets for the parts
    one pipe delivers."""

    def __init__(self, routing_id):
        self.routing_id, self.more_in, self.got = routing_id, False, []

    def part(self, flags, data):
        if self.more_in:  # (:302-311) in the middle of a message: the next part as it is
            self.more_in = bool(flags & MORE)
            self.got.append((flags & MORE, data))
            return
        # (:312-329) the beginning of a message: the id of the peer first, with more set, then the prefetched part
        self.got.append((MORE, self.routing_id))
        self.more_in = bool(flags & MORE)  # (:275, on the prefetched part)
        self.got.append((flags & MORE, data))


IDS = [b"", b"\x00\x00\x00\x00\x01", b"\x00\x00\x00\x00\x02", b"peer", b"peer-long", b"pe"]


def _parts(rng, addresses, n_msgs, tail_open, fixed=()):
    """Random messages whose first part is drawn from `addresses` (None: any
    payload), one-part messages and commands in between; fixed: (parts, first
    part) of the first messages."""
    parts = []
    for i in range(n_msgs):
        n = fixed[i][0] if i < len(fixed) else int(rng.choice([1, 2, 2, 3, 4]))
        for j in range(n):
            if rng.integers(0, 4) == 0:
                parts.append((CMD | int(rng.integers(0, 2)), b"cmd"))
            data = rng.integers(0, 256, int(rng.choice([0, 1, 5, 40])), dtype=np.uint8).tobytes()
            if j == 0 and addresses is not None:
                data = fixed[i][1] if i < len(fixed) else addresses[int(rng.integers(0, len(addresses)))]
            last = j == n - 1 and not (tail_open and i == n_msgs - 1)
            parts.append((LAST if last else MORE, data))
    return parts


def _case(rng, parts_per_stream, routes, n_dst):
    S = len(parts_per_stream)
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(S + n_dst)]
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in enumerate(parts_per_stream)]
    arena, offs = F.arena_of(streams)
    return dict(precoms=precoms, down=[False] * (S + n_dst), arena=arena, offs=offs, lens=[len(s) for s in streams],
                sids=list(range(S)), peer=[2] * (S + n_dst), max_frames=max(len(p) for p in parts_per_stream) + 1,
                carry=[[] for _ in range(S)], plain=None, dst_sid=list(range(S, S + n_dst)), routes=routes,
                send=[1] * (S + n_dst))


def _args(c):
    return (c["precoms"], c["down"], c["arena"], c["offs"], c["lens"], c["sids"], c["peer"], -1, c["max_frames"],
            c["carry"], c["plain"], c["dst_sid"], c["routes"], c["send"])


def _sent(m, n_dst):
    """Per destination, the live pairs in pair order: (MORE bit, payload)."""
    out = [[] for _ in range(n_dst)]
    for p, pr in enumerate(m["pairs"]):
        if pr[3]:
            out[m["frame_stream"][p]].append((m["flags"][p], m["payloads"][p]))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_route_rule_is_router_xsend(seed):
    """Two source streams fair-queued whole message by whole message into one
    xsend: each peer's pipe holds, per source, what the model's live pairs
    hold.  Addresses: known ids, the empty id (in the table for odd seeds), a
    strict prefix of an id, an id plus a byte, unknown ones."""
    rng = np.random.default_rng(seed)
    known = IDS[1:5] + ([b""] if seed % 2 else [])
    pool = IDS + [b"peer-", b"nobody", b"\x00\x00\x00\x00"]
    n_dst = 3
    peers = {i: int(rng.integers(0, n_dst)) for i in known}  # (two ids may name one destination)
    fixed = [(1, IDS[1]), (3, b"nobody"), (2, IDS[1]), (3, b"")]  # one-part, unknown, known, the empty address
    parts = [_parts(rng, pool, 8, tail_open=bool(s), fixed=fixed) for s in range(2)]
    c = _case(rng, parts, [[], []], n_dst)
    table = FR.table_of(peers.items())
    m = FR.model(*_args(c), FR.ROUTE, None, table, 2 ** 62, 0, encode=False)
    assert m["N"] == 2 * c["max_frames"] and m["base"] == [0, c["max_frames"], 2 * c["max_frames"]]
    sent = _sent(m, n_dst)
    seen = set()
    want = [[] for _ in range(n_dst)]
    for s in range(2):
        r = RouterSend(peers)
        for q, (fl, data) in enumerate(parts[s]):
            if q < m["fwd"][s]["held_first"] and not fl & CMD:  # what the pipe shows the proxy: whole messages only
                r.xsend(fl, data)
        assert not r.more_out and r.current_out is None  # every message below held_first is complete
        for t in range(n_dst):
            want[t] += r.written.get(t, [])
        seen.update(m["dest"][m["base"][s]:m["base"][s + 1]])
    assert sent == want
    assert {FR.NONE, FR.ADDRESS, FR.UNKNOWN, FR.MALFORMED} <= seen and any(d < n_dst for d in seen)
    # dest_out, entry by entry
    for p, (s, q, _, live, _) in enumerate(m["pairs"]):
        fl = parts[s][q][0] if q < len(parts[s]) else CMD
        d = m["dest"][p]
        if q >= m["fwd"][s]["held_first"] or fl & CMD:
            assert d == FR.NONE
        elif m["head"][s][q] == q:
            assert d == (FR.ADDRESS if fl & MORE else FR.MALFORMED)
        else:
            t = peers.get(parts[s][m["head"][s][q]][1])
            assert d == (FR.UNKNOWN if t is None else t) and live == (t is not None)


@pytest.mark.parametrize("seed", range(4))
def test_prepend_rule_is_router_xrecv(seed):
    """One route per source: the destination's run is, per source, what
    router_t::xrecv hands the proxy for that pipe's whole messages."""
    rng = np.random.default_rng(100 + seed)
    parts = [_parts(rng, None, 5, tail_open=bool(s % 2)) for s in range(3)]
    c = _case(rng, parts, [[0], [1], [0]], 2)
    ids = [b"\x00ABCD", b"", b"x" * 40]
    # the ids parked behind the arena
    plain = np.concatenate([c["arena"], np.frombuffer(b"".join(ids), np.uint8)])
    src_ids, pos = [], len(c["arena"])
    for i in ids:
        src_ids.append((pos, len(i)))
        pos += len(i)
    c["plain"] = plain
    m = FR.model(*_args(c), FR.PREPEND, src_ids, None, 2 ** 62, 0, encode=False)
    assert m["N"] == 2 * 3 * c["max_frames"]
    want = [[], []]
    for s in range(3):
        r = RouterRecv(ids[s])
        for q, (fl, data) in enumerate(parts[s]):
            if q < m["fwd"][s]["held_first"] and not fl & CMD:
                r.part(fl, data)
        want[c["routes"][s][0]] += r.got
    assert _sent(m, 2) == want
    # the id slot is 2q, the element 2q + 1; dest_out is the route's destination or NONE
    for p, (s, q, k, live, is_id) in enumerate(m["pairs"]):
        assert p == m["base"][s] + (2 * q + (0 if is_id else 1)) and k == 0
        assert m["dest"][p] == (c["routes"][s][0] if live else FR.NONE)


def test_route_with_prepend_is_router_to_router():
    """Both flags: xrecv's prefix is xsend's address -- every whole message of
    a source goes, unchanged, to the peer whose id is the source's."""
    rng = np.random.default_rng(9)
    parts = [_parts(rng, None, 4, tail_open=False) for s in range(3)]
    c = _case(rng, parts, [[], [], []], 2)
    ids = [b"one", b"two", b"nobody"]
    c["plain"] = np.concatenate([c["arena"], np.frombuffer(b"".join(ids), np.uint8)])
    L = len(c["arena"])
    src_ids = [(L, 3), (L + 3, 3), (L + 6, 6)]
    peers = {b"one": 1, b"two": 0}
    m = FR.model(*_args(c), FR.ROUTE | FR.PREPEND, src_ids, FR.table_of(peers.items()), 2 ** 62, 0, encode=False)
    want = [[], []]
    for s in range(3):
        recv, send = RouterRecv(ids[s]), RouterSend(peers)
        for fl, data in parts[s]:
            if not fl & CMD:
                recv.part(fl, data)
        for fl, data in recv.got:
            send.xsend(fl, data)
        for t in (0, 1):
            want[t] += send.written[t]
    assert _sent(m, 2) == want and FR.ADDRESS not in m["dest"] and FR.MALFORMED not in m["dest"]
    assert set(m["dest"][m["base"][2]:]) == {FR.UNKNOWN, FR.NONE}


def _distinct_ids(rng, n):
    ids = set()
    while len(ids) < n:
        ids.add(bytes(rng.integers(0x7e, 0x82, int(rng.integers(0, 7)), dtype=np.uint8)) if n < 100 else
                b"\x00" + int(rng.integers(0, 2 ** 32)).to_bytes(4, "big"))
    return sorted(ids)


@pytest.mark.parametrize("n_ids", [0, 1, 2, 3, 63, 64, 65, 1000])
def test_search_is_dict_lookup_on_sorted_tables(n_ids):
    rng = np.random.default_rng(n_ids)
    ids = _distinct_ids(rng, n_ids)
    ref = {i: int(rng.integers(0, 50)) for i in ids}
    table = FR.table_of(ref.items())
    assert [FR.entry(table, j) for j in range(n_ids)] == ids  # (Python orders bytes as blob_t does)
    assert all(FR.less(a, b) and not FR.less(b, a) for a, b in zip(ids, ids[1:]))
    probes = ids[:200] + [i + b"\x7f" for i in ids[:100]] + [i[:-1] for i in ids[:100] if i] + [b"", b"\xff" * 9]
    probes += _distinct_ids(rng, min(n_ids, 60) + 3)
    for a in probes:
        assert FR.lookup(table, a, 50) == ref.get(a), a
    for i in ids[:20]:  # a destination at or above n_dst is no destination
        assert FR.lookup(table, i, ref[i]) is None and FR.lookup(table, i, ref[i] + 1) == ref[i]


def test_ordering_edge_cases():
    long_a = b"\x81" * 300
    cases = [(b"abc", b"abcd"), (b"abcd", b"abc"), (b"abc", b"abc"), (b"", b""), (b"", b"a"), (b"a", b""),
             (b"abc", b"abd"), (b"xbc", b"abc"), (b"abc", b"xbc"), (b"\x7f", b"\x80"), (b"\x80", b"\x7f"),
             (b"\x00", b""), (long_a, long_a[:-1] + b"\x82"), (long_a[:-1] + b"\x82", long_a), (long_a[:-1], long_a)]
    for a, b in cases:
        assert FR.less(a, b) == (a < b), (a, b)
    # a is a prefix of b; equal bytes, different length; the empty id; the last byte only; the first only
    assert FR.less(b"abc", b"abcd") and not FR.less(b"abcd", b"abc") and not FR.less(b"abc", b"abc")
    assert FR.less(b"", b"\x00") and not FR.less(b"", b"")
    assert FR.less(b"abc", b"abd") and FR.less(b"abc", b"bbc")


def test_void_entries_and_untrusted_tables():
    raw = b"abcXYZ"
    t = dict(off=[0, 4, 3, 2 ** 64 - 1, 1], len=[3, 3, 0, 2, 2 ** 32 - 1], dst=[0, 1, 2, 3, 4], raw=raw, n_ids=5,
             bytes_len=3)
    # within [0, 3): entry 0 "abc", entry 2 the empty id at the very end; void: offset past the end, off + len
    # overflowing, a length past the end
    assert [FR.entry(t, j) for j in range(5)] == [b"abc", None, b"", None, None]
    # the search still ends, and a void entry equals nothing, the empty address included
    assert FR.lookup(dict(t, n_ids=2), b"", 9) is None
    assert FR.lookup(dict(t, off=[9], len=[0], dst=[0], n_ids=1), b"", 9) is None
    assert FR.lookup(dict(t, off=[3], len=[0], dst=[0], n_ids=1), b"", 9) == 0
    # an unsorted table: the loop's answer, whatever it is, not find's
    u = FR.table_of([(b"a", 0), (b"b", 1), (b"c", 2)])
    u["off"], u["dst"] = [1, 0, 2], [1, 0, 2]  # now "b", "a", "c"
    assert [FR.lookup(u, x, 3) for x in (b"a", b"b", b"c")] == [None, None, 2]


@pytest.mark.parametrize("seed", range(3))
def test_flags_0_is_the_forward_model(seed):
    c = _random_case(seed)
    total = F.model(*_args(c), 2 ** 62, 0, encode=False)["enc"]["frame_off"][-1]
    cap = total - total // 3
    a = F.model(*_args(c), cap, total + 16)
    b = FR.model(*_args(c), 0, None, None, cap, total + 16)
    for k in ("fwd", "base", "N", "pairs", "frame_stream", "flags", "lens", "payloads"):
        assert a[k] == b[k], k
    for k in ("results", "f_off", "f_len", "status", "flags", "out", "peer"):
        assert np.array_equal(a["recv"][k], b["recv"][k]), k
    for k in a["enc"]:
        assert np.array_equal(a["enc"][k], b["enc"][k]), k
    # the element slots of a PREPEND call are the parent's pairs, slot by slot
    ids = [(0, 0)] * len(c["offs"])
    p = FR.model(*_args(c), FR.PREPEND, ids, None, 2 ** 62, 0, encode=False)
    elem = [i for i, pr in enumerate(p["pairs"]) if not pr[4]]
    assert [p["pairs"][i][:4] for i in elem] == a["pairs"] and p["N"] == 2 * a["N"]
    assert [p["payloads"][i] for i in elem] == a["payloads"]
