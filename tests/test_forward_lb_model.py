"""tests/forward_lb_model.py (no GPU): the model's choice against a literal
restatement of lb_t (src/lb.cpp:56-131) -- _pipes, _active, _current and _more,
sendpipe run part by part with every write succeeding -- under random
multi-part traffic over several calls with the cursor carried between them;
commands in between parts, a failing stream, carried heads, NO_GROUP; the
untrusted table; the pair layout with PREPEND."""
import numpy as np
import pytest

from tests import forward_lb_model as FL
from tests import forward_model as F
from tests import forward_router_model as FR

MORE, CMD, LAST = F.MORE, F.COMMAND, 0


class LbT:
    """lb_t with pipes that never fill: pipe_t::write always succeeds, so
    _dropping is never set and no pipe is deactivated."""

    def __init__(self, pipes, current=0):
        self._pipes, self._active, self._current, self._more = list(pipes), len(pipes), current, False
        self.written = []  # (pipe, MORE bit, payload) in order

    def sendpipe(self, flags, data):
        if self._active == 0:  # (:111-114) no pipes: the message cannot be sent
            return -1
        self.written.append((self._pipes[self._current], flags & MORE, data))  # (:72) _pipes[_current]->write
        self._more = bool(flags & MORE)  # (:118)
        if not self._more:  # (:119-124) the final part: flush, and go on round-robining
            self._current += 1
            if self._current >= self._active:
                self._current = 0
        return 0


def _parts(rng, n_msgs, tail_open):
    parts = []
    for i in range(n_msgs):
        n = int(rng.choice([1, 1, 2, 3, 4]))
        for j in range(n):
            if rng.integers(0, 4) == 0:  # a command between parts (or in front of a message)
                parts.append((CMD | int(rng.integers(0, 2)), b"cmd"))
            data = rng.integers(0, 256, int(rng.integers(1, 41)), dtype=np.uint8).tobytes()
            last = j == n - 1 and not (tail_open and i == n_msgs - 1)
            parts.append((LAST if last else MORE, data))
    return parts


def _case(precoms, parts_per_stream, nonce0, peer, n_dst, carry_parts=None, tamper=()):
    """One call's inputs: stream s sends parts_per_stream[s] from nonce
    nonce0[s]; carry_parts[s] = [(flags, payload)] held by the call before, laid
    behind the arena in `plain`; tamper: (stream, frame) whose last byte is
    flipped."""
    S = len(parts_per_stream)
    frames = [F.source_frames(precoms[s], p, nonce0=nonce0[s]) for s, p in enumerate(parts_per_stream)]
    for s, j in tamper:
        frames[s][j] = frames[s][j][:-1] + bytes([frames[s][j][-1] ^ 1])
    streams = [b"".join(f) for f in frames]
    arena, offs = F.arena_of(streams)
    carry_parts = carry_parts or [[] for _ in range(S)]
    blob, carry = bytearray(), []
    for s in range(S):
        row = []
        for fl, data in carry_parts[s]:
            row.append((len(arena) + len(blob), len(data), fl))
            blob += data
        carry.append(row)
    plain = np.concatenate([arena, np.frombuffer(bytes(blob), np.uint8)]) if blob else None
    ns = len(precoms)
    return dict(precoms=precoms, down=[False] * ns, arena=arena, offs=offs, lens=[len(s) for s in streams],
                sids=list(range(S)), peer=peer, max_frames=max([len(p) for p in parts_per_stream] + [0]) + 1,
                carry=carry, plain=plain, dst_sid=list(range(S, S + n_dst)), send=[1] * ns)


def _args(c):
    return (c["precoms"], c["down"], c["arena"], c["offs"], c["lens"], c["sids"], c["peer"], -1, c["max_frames"],
            c["carry"], c["plain"], c["dst_sid"], c["send"])


def _sent(m, n_dst):
    """Per destination, the live pairs in pair order: (MORE bit, payload)."""
    out = [[] for _ in range(n_dst)]
    for p, pr in enumerate(m["pairs"]):
        if pr[3]:
            out[m["frame_stream"][p]].append((m["flags"][p], m["payloads"][p]))
    return out


def _table(groups, cur, pad=0):
    """grp_idx / lb_dst for lists of destinations, `pad` entries in front."""
    idx, dst = [pad], [99] * pad
    for g in groups:
        dst += list(g)
        idx.append(len(dst))
    return dict(grp_idx=idx, lb_dst=dst, lb_cur=list(cur), n_lb=len(dst))


@pytest.mark.parametrize("seed", range(6))
def test_choice_is_lb_sendpipe_over_several_calls(seed):
    """Five streams, two load balancers with interleaved streams and one stream
    without a group, four calls: every lb_t is fed the whole messages of its
    streams in stream-major order, part by part; what each pipe is written, in
    order, is the destination's run, and _current is the cursor the next call
    starts from.  Held tails are carried into the next call, commands lie
    between parts, and one stream fails in the second call."""
    rng = np.random.default_rng(seed)
    S, n_dst = 5, 5
    group = [0, 1, 0, 1, FL.NO_GROUP]
    pipes = [[3, 0, 4], [1, 2]] if seed % 2 else [[2], [0, 1, 3, 4]]
    cur = [int(rng.integers(0, len(p))) for p in pipes]
    lbs = [LbT(p, c) for p, c in zip(pipes, cur)]
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(S + n_dst)]
    nonce0, peer, held = [3] * S, [2] * (S + n_dst), [[] for _ in range(S)]
    wrapped = False
    for call in range(4):
        parts = [_parts(rng, int(rng.integers(0, 6)), tail_open=bool(rng.integers(0, 2))) for _ in range(S)]
        tamper = [(2, len(parts[2]) // 2)] if call == 1 and parts[2] else []
        c = _case(precoms, parts, nonce0, peer, n_dst, carry_parts=held, tamper=tamper)
        table = _table(pipes, cur, pad=call % 2)
        m = FL.model(*_args(c), 0, None, group, table, 2 ** 62, 0, encode=False)
        assert m["base"] == [sum(len(h) + c["max_frames"] for h in held[:s]) for s in range(S + 1)]
        want = [[] for _ in range(n_dst)]
        new_held = []
        for s in range(S):
            q_all = held[s] + parts[s]
            fw = m["fwd"][s]
            assert fw["failed"] == int(bool(tamper) and s == 2)
            n0 = len(lbs[group[s]].written) if group[s] != FL.NO_GROUP else 0
            for fl, data in q_all[:fw["held_first"]]:
                if not fl & CMD and group[s] != FL.NO_GROUP:  # what the pipe shows the proxy: whole messages only
                    assert lbs[group[s]].sendpipe(fl, data) == 0
            if group[s] != FL.NO_GROUP:
                assert not lbs[group[s]]._more  # every message below held_first is complete
                for t, more, data in lbs[group[s]].written[n0:]:
                    want[t].append((more, data))
            # a failed connection's tail is dropped; otherwise the held data parts are carried
            new_held.append([] if fw["failed"] else [(fl, d) for fl, d in q_all[fw["held_first"]:fw["seq"]]
                                                      if not fl & CMD])
        assert _sent(m, n_dst) == want
        assert m["lb_cur"] == [lb._current for lb in lbs]
        wrapped = wrapped or any(n > 2 * len(p) for n, p in zip(m["msgs"], pipes))
        # the stream without a group: its forwarded parts found no destination
        for p, (s, q, _, live, _) in enumerate(m["pairs"]):
            if s == 4:
                fwd_q = q < m["fwd"][s]["seq"] and m["fwd"][s]["live"][q]
                assert not live and m["dest"][p] == (FL.NO_PEER if fwd_q else FL.NONE)
        cur, held, peer = m["lb_cur"], new_held, m["recv"]["peer"]
        nonce0 = [n + len(p) for n, p in zip(nonce0, parts)]
    assert wrapped  # some ring went round more than twice in one call


def test_carried_head_and_command_between_parts():
    """A head carried from the call before takes its turn in the call that
    forwards its message; a command between two parts neither ends nor breaks
    the message, and takes no turn."""
    rng = np.random.default_rng(50)
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(2 + 3)]
    parts = [[(MORE, b"b1"), (CMD, b"ping"), (LAST, b"b2"), (LAST, b"c")], [(LAST, b"d"), (MORE, b"e-open")]]
    held = [[(MORE, b"a-head")], []]
    c = _case(precoms, parts, [3, 3], [2] * 5, 3, carry_parts=held)
    m = FL.model(*_args(c), 0, None, [0, 0], _table([[2, 0, 1]], [5]), 2 ** 62, 0, encode=False)
    # cur0 = 5 mod 3 = 2: [a-head b1 b2] -> entry 2 (destination 1), [c] -> entry 0 (2), [d] -> entry 1 (0)
    assert _sent(m, 3) == [[(0, b"d")], [(MORE, b"a-head"), (MORE, b"b1"), (0, b"b2")], [(0, b"c")]]
    assert m["msgs"] == [3] and m["picks"] == [[2, 0, 1]] and m["lb_cur"] == [2]
    assert m["dest"][:5] == [1, 1, FL.NONE, 1, 2] and m["dest"][c["max_frames"] + 1:][:2] == [0, FL.NONE]
    assert m["fwd"][1]["held_first"] == 1


@pytest.mark.parametrize("A", [1, 2, 3, 7])
def test_cursor_values(A):
    rng = np.random.default_rng(A)
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(1 + A)]
    for M in (A - 1, A, A + 2):
        parts = [[(LAST, b"m%d" % i) for i in range(M)]]
        c = _case(precoms, parts, [3], [2] * (1 + A), A)
        for start in (0, A - 1, A, 0xffffffff):
            m = FL.model(*_args(c), 0, None, [0], _table([range(A)], [start]), 2 ** 62, 0, encode=False)
            lb = LbT(range(A), start % A)
            for fl, data in parts[0]:
                lb.sendpipe(fl, data)
            assert [(t, d) for t, _, d in lb.written] == [(m["dest"][q], parts[0][q][1]) for q in range(M)]
            assert m["lb_cur"] == [lb._current] == [(start % A + M) % A]


def test_untrusted_table():
    rng = np.random.default_rng(7)
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(3 + 2)]
    parts = [[(LAST, b"x"), (MORE, b"y1"), (LAST, b"y2")], [(LAST, b"z")], [(LAST, b"w")]]
    c = _case(precoms, parts, [3] * 3, [2] * 5, 2)
    # group 0: [0, 9) clamped to n_lb = 3 -> entries {1, 7, 0}; group 1: a falling pair -> empty; group 2: no stream
    table = dict(grp_idx=[0, 9, 2, 3], lb_dst=[1, 7, 0, 1, 1], lb_cur=[4, 6, 0xffffffff], n_lb=3)
    assert [FL.group_range(table, g) for g in range(3)] == [(0, 3), (3, 0), (2, 1)]
    m = FL.model(*_args(c), 0, None, [0, 1, 0], table, 2 ** 62, 0, encode=False)
    mf = c["max_frames"]
    # cur0 = 4 mod 3 = 1: x -> entry 1 = 7 (no destination, the turn is consumed), y -> entry 2 = 0, w -> entry 0 = 1
    assert m["dest"][:3] == [FL.NO_PEER, 0, 0] and m["dest"][mf] == FL.NO_PEER and m["dest"][2 * mf] == 1
    assert m["lb_cur"] == [1, 0, 0] and m["msgs"] == [3, 1, 0]
    assert _sent(m, 2) == [[(MORE, b"y1"), (0, b"y2")], [(0, b"w")]]


def test_prepend_layout_is_the_router_calls():
    """A = 1 with PREPEND: the pairs, payloads and flags are
    zmqg_forward_zmtp_router_multi's PREPEND with every stream routed to that
    destination; the id slots are live only in front of heads."""
    rng = np.random.default_rng(3)
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(3 + 2)]
    parts = [_parts(rng, 4, tail_open=bool(s % 2)) for s in range(3)]
    c = _case(precoms, parts, [3] * 3, [2] * 5, 2)
    ids = [b"\x00ABCD", b"", b"x" * 40]
    c["plain"] = np.concatenate([c["arena"], np.frombuffer(b"".join(ids), np.uint8)])
    src_ids, pos = [], len(c["arena"])
    for i in ids:
        src_ids.append((pos, len(i)))
        pos += len(i)
    m = FL.model(*_args(c), FL.PREPEND, src_ids, [0, 0, 0], _table([[1]], [0]), 2 ** 62, 0, encode=False)
    a = _args(c)
    r = FR.model(*a[:12], [[1], [1], [1]], a[12], FR.PREPEND, src_ids, None, 2 ** 62, 0, encode=False)
    for k in ("base", "N", "pairs", "frame_stream", "flags", "lens", "payloads", "head"):
        assert m[k] == r[k], k
    assert [FL.NONE if d == FR.NONE else d for d in r["dest"]] == m["dest"]
    for p, (s, q, _, live, is_id) in enumerate(m["pairs"]):
        assert p == m["base"][s] + 2 * q + (0 if is_id else 1)
        if is_id:
            assert live == (m["head"][s][q] == q if q < len(m["head"][s]) else False)
