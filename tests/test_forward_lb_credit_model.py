"""tests/forward_lb_credit_model.py (no GPU) against an independent restatement
of the reference: lb_t (src/lb.cpp:56-131) with _pipes, _active, _current,
_more and _dropping, run part by part over pipe objects that keep pipe_t's
counters (_msgs_written, _peers_msgs_read and the hwm; check_hwm,
src/pipe.cpp:535-541; write, :222-234).  A pipe that refuses a write is swapped
out of the active range (:103-107) and the part is offered to the next one.
What every pipe was written, part by part, must be the model's run for that
destination; a message lb_t answers with EAGAIN must be the model's refused
message; _current must name the entry lb_cur names.  With every credit
unlimited the model is forward_lb_model through forward_framed_model."""
import numpy as np
import pytest

from tests import forward_framed_model as FM
from tests import forward_lb_credit_model as LC
from tests import forward_lb_model as FL
from tests import forward_model as F
from tests import test_forward_lb_model as TL
from tests import zmtp_send_model as M

MORE, CMD, LAST = F.MORE, F.COMMAND, 0
UNL = LC.UNLIMITED


class Pipe:
    """pipe_t's send side as far as the high-water mark goes."""

    def __init__(self, hwm, written):
        self.hwm, self._msgs_written, self._peers_msgs_read = hwm, written, 0
        self.got = []

    def check_hwm(self):  # (:535-541)
        full = self.hwm > 0 and self._msgs_written - self._peers_msgs_read >= self.hwm
        return not full

    def write(self, flags, data):  # (:222-234) check_write first; the count rises on a part without MORE
        if not self.check_hwm():
            return False
        self.got.append((flags & MORE, data))
        if not flags & MORE:
            self._msgs_written += 1
        return True

    def credit(self):
        return UNL if self.hwm == 0 else self.hwm - (self._msgs_written - self._peers_msgs_read)


class LbT:
    """lb_t over (original position, pipe) entries, every one active at the start."""

    def __init__(self, entries, current):
        self._pipes, self._active, self._current = list(entries), len(entries), current
        self._more = self._dropping = False

    def sendpipe(self, flags, data):
        assert not self._dropping  # (:60) only whole messages are offered
        while self._active > 0:
            if self._pipes[self._current][1].write(flags, data):  # (:72)
                break
            assert not self._more  # (:81) a part after the head is never refused
            self._active -= 1  # (:103-107)
            if self._current < self._active:
                a, b = self._current, self._active
                self._pipes[a], self._pipes[b] = self._pipes[b], self._pipes[a]
            else:
                self._current = 0
        if self._active == 0:  # (:111-114)
            return -1
        self._more = bool(flags & MORE)  # (:118-124)
        if not self._more:
            self._current += 1
            if self._current >= self._active:
                self._current = 0
        return 0

    def cursor(self):
        """The original position of _pipes[_current], 0 without active pipes."""
        return self._pipes[self._current][0] if self._active else 0


def _whole(parts):
    """The data parts as whole messages, commands left out."""
    msgs, cur = [], []
    for fl, data in parts:
        if fl & CMD:
            continue
        cur.append((fl, data))
        if not fl & MORE:
            msgs.append(cur)
            cur = []
    assert not cur
    return msgs


def _lb_credit(c, credit, group, table, consume=True, flags=0, src_ids=None):
    return LC.model(FM.ZMTP, FM.ZMTP, credit, *TL._args(c), None, 16, flags=flags, src_ids=src_ids,
                    stream_group=group, table=table, consume=consume, encode=False)


def _calls(seed, seen):
    """Four calls over the same pipes; between them the peers read and the host refills the credits."""
    rng = np.random.default_rng(400 + seed)
    S, n_dst = 5, 5
    group = [0, 1, 0, 1, FL.NO_GROUP]
    rings = [[[3, 0, 4], [1, 2]], [[2], [0, 1, 3, 4]], [[3, 7, 0, 4], [9, 1, 2]]][seed % 3]  # (7, 9: no destination)
    cur = [int(rng.integers(0, 2 ** 32)) for _ in rings]
    pipes = [Pipe(0, 5) if rng.integers(0, 4) == 0 else Pipe(int(rng.integers(1, 5)), 0) for _ in range(n_dst)]
    for p in pipes:  # some pipes are full when the first call comes
        if p.hwm and rng.integers(0, 3) == 0:
            p._msgs_written = p.hwm
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(S + n_dst)]
    nonce0, peer, held = [3] * S, [2] * (S + n_dst), [[] for _ in range(S)]
    for call in range(4):
        parts = [TL._parts(rng, int(rng.integers(0, 6)), tail_open=bool(rng.integers(0, 2))) for _ in range(S)]
        c = TL._case(precoms, parts, nonce0, peer, n_dst, carry_parts=held)
        table = TL._table(rings, cur, pad=call % 2)
        credit = [p.credit() for p in pipes]
        m = _lb_credit(c, credit, group, table)
        lbs = []
        for g, ring in enumerate(rings):
            entries = [(j, pipes[t] if t < n_dst else Pipe(0, 0)) for j, t in enumerate(ring)]
            lbs.append(LbT(entries, cur[g] % len(ring)))
        n0 = [len(p.got) for p in pipes]
        w0 = [p._msgs_written for p in pipes]
        refused, new_held = [], []
        for s in range(S):
            q_all = held[s] + parts[s]
            fw = m["fwd"][s]
            if group[s] != FL.NO_GROUP:
                for msg in _whole(q_all[:fw["held_first"]]):
                    if lbs[group[s]].sendpipe(*msg[0]) < 0:  # EAGAIN at the head: the message is not sent
                        refused.append((s, msg))
                        continue
                    for part in msg[1:]:
                        assert lbs[group[s]].sendpipe(*part) == 0
                    assert not lbs[group[s]]._more
            new_held.append([(fl, d) for fl, d in q_all[fw["held_first"]:fw["seq"]] if not fl & CMD])
        assert TL._sent(m, n_dst) == [p.got[n:] for p, n in zip(pipes, n0)]
        assert m["lb_cur"] == [lb.cursor() for lb in lbs]
        assert m["taken"] == [p._msgs_written - w for p, w in zip(pipes, w0)] and m["dropped"] == [0] * n_dst
        assert m["credit_after"] == [p.credit() for p in pipes]
        # the refused messages, in order: every slot not live, NO_PEER, ERR_HWM
        mine = {}
        for p, (s, q, _, live, _) in enumerate(m["pairs"]):
            if m["hwm"][p]:
                assert not live and m["dest"][p] == FL.NO_PEER and m["enc"]["status"][p] == LC.ERR_HWM
                assert m["frame_stream"][p] == F.NO_STREAM
                mine.setdefault((s, m["head"][s][q]), []).append(q)
            else:
                assert m["enc"]["status"][p] != LC.ERR_HWM
        assert [(s, len(msg)) for s, msg in refused] == [(s, len(qs)) for (s, _), qs in sorted(mine.items())]
        for g, lb in enumerate(lbs):
            seen["skipped"] += len(rings[g]) - lb._active
            if LC.REFUSED in m["picks"][g]:
                assert lb._active == 0
        seen["refused"] += len(refused)
        seen["sent"] += sum(m["taken"])
        cur, held, peer = m["lb_cur"], new_held, m["recv"]["peer"]
        nonce0 = [n + len(p) for n, p in zip(nonce0, parts)]
        for p in pipes:  # the peers read some of what they were sent
            p._peers_msgs_read += int(rng.integers(0, p._msgs_written - p._peers_msgs_read + 1))


def test_choice_is_lb_sendpipe_over_pipes_that_fill():
    seen = dict(refused=0, skipped=0, sent=0)
    for seed in range(12):
        _calls(seed, seen)
    assert seen["skipped"] > 10 and seen["sent"] > 50 and seen["refused"] > 5, seen


def test_the_swap_is_visible():
    credit = lambda **kw: [kw.get("c%d" % t, UNL) for t in range(4)]
    # ring [0, 1, 2, 3] from cursor 1 with entry 1 full: 3 takes its place (a stable skip would give 2, 3, 0)
    assert LC.choose([0, 1, 2, 3], credit(c1=0), 1, 7) == ([3, 2, 0, 3, 2, 0, 3], 2)
    # ring [0, 1, 2] from cursor 2 with entry 2 full: nothing to swap with, the cursor goes back to 0
    assert LC.choose([0, 1, 2], credit(c2=0), 2, 3) == ([0, 1, 0], 1)
    # credits [1, 2, 1], eight messages: four go out, four are refused, and the ring is empty
    assert LC.choose([0, 1, 2], [1, 2, 1], 0, 8) == ([0, 1, 2, 1] + [LC.REFUSED] * 4, 0)
    assert LC.choose([0, 1, 2], [0, 0, 0], 1, 2) == ([LC.REFUSED] * 2, 0)
    # rem == L: the full entry is found by a later send only, and the cursor rests on it
    assert LC.choose([0, 1], [1, 1], 0, 2) == ([0, 1], 0)
    # an entry naming no destination takes its turn and is never deactivated
    assert LC.choose([0, 9, 1], [1, 0], 0, 5) == ([0, 1, 1, 1, 1], 1)
    # one destination named twice: each entry has the whole credit
    assert LC.choose([0, 0], [1], 0, 3) == ([0, 1, LC.REFUSED], 0)


def test_duplicate_entry_counts_and_saturates():
    rng = np.random.default_rng(77)
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(1 + 2)]
    parts = [[(LAST, b"m%d" % i) for i in range(5)]]
    c = TL._case(precoms, parts, [3], [2] * 3, 2)
    m = _lb_credit(c, [2, 1], [0], TL._table([[0, 1, 0]], [0]))
    # entries 0 and 2 both hold destination 0's credit of 2: 0 1 0' 0 0' and nobody left
    assert m["picks"] == [[0, 1, 2, 0, 2]] and m["sent"] == [4, 1]
    assert m["taken"] == [2, 1] and m["dropped"] == [2, 0] and m["credit_after"] == [0, 0]
    assert not any(m["hwm"]) and m["lb_cur"] == [0]


@pytest.mark.parametrize("seed", range(6))
def test_unlimited_is_the_lb_model(seed):
    rng = np.random.default_rng(900 + seed)
    S, n_dst = 4, 4
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(S + n_dst)]
    parts = [TL._parts(rng, int(rng.integers(0, 6)), tail_open=bool(rng.integers(0, 2))) for _ in range(S)]
    c = TL._case(precoms, parts, [3] * S, [2] * (S + n_dst), n_dst)
    ids = [b"\x00A", b"", b"x" * 9, b"id3"]
    c["plain"] = np.concatenate([c["arena"], np.frombuffer(b"".join(ids), np.uint8)])
    src_ids, pos = [], len(c["arena"])
    for i in ids:
        src_ids.append((pos, len(i)))
        pos += len(i)
    flags = FL.PREPEND if seed % 2 else 0
    group = [0, 1, 0, FL.NO_GROUP]
    table = dict(grp_idx=[0, 3, 9], lb_dst=[2, 8, 0, 1, 3], lb_cur=[7, 0xffffffff], n_lb=5)
    kw = dict(flags=flags, src_ids=src_ids if flags else None, stream_group=group, table=table)
    m = _lb_credit(c, [UNL] * n_dst, group, table, flags=flags, src_ids=kw["src_ids"])
    own = FM.model(FM.LB, FM.ZMTP, FM.ZMTP, *TL._args(c), None, 16, encode=False, **kw)
    for k in ("fwd", "base", "N", "pairs", "frame_stream", "flags", "lens", "payloads", "dest", "lb_cur", "total",
              "cap", "size"):
        assert m[k] == own[k], k
    for k in ("frame_off", "status", "results", "send"):
        assert m["enc"][k] == own["enc"][k], k
    assert not any(m["hwm"]) and m["dropped"] == [0] * n_dst and m["credit_after"] == [UNL] * n_dst
    assert sum(m["taken"]) == sum(1 for g in range(2) for j in own["picks"][g] if table["lb_dst"][
        FL.group_range(table, g)[0] + j] < n_dst)
    assert M.ERR_SESSION in m["enc"]["status"] or m["N"] == 0
