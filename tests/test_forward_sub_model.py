"""tests/forward_sub_model.py (no GPU): the prefix rule against a restatement of
the reference's trie (generic_mtrie_t::add / match, src/
generic_mtrie_impl.hpp:41-115, :523-561, written here as nodes with a child
per byte and walked as the reference walks them), the heads on hand cases,
and the model with the empty prefix on every destination against
tests/forward_model.py's model field by field."""
import numpy as np
import pytest

from tests import forward_model as F
from tests import forward_sub_model as FS
from tests.test_forward_model import _random_case

MORE, CMD, LAST = F.MORE, F.COMMAND, 0


class Trie:
    """generic_mtrie_t: a node holds the pipes subscribed to exactly the
    prefix that leads to it, and its children by the next byte (the
    reference's _min / _count / _next table is a dense form of this map)."""

    def __init__(self):
        self.pipes, self.next = None, {}

    def add(self, prefix, pipe):
        it = self
        for c in prefix:  # (:45-113: one node down per byte, created when missing)
            it = it.next.setdefault(c, Trie())
        if it.pipes is None:  # (:116-123)
            it.pipes = set()
        it.pipes.add(pipe)

    def match(self, data, func):
        current, i = self, 0
        while current is not None:
            for p in sorted(current.pipes or ()):  # (:530-536) signal the pipes attached to this node
                func(p)
            if i == len(data):                     # (:539-540) the end of the message
                break
            if not current.next:                   # (:543-544) no subnodes
                break
            current = current.next.get(data[i])    # (:546-559) out of range or an empty slot ends the walk
            i += 1


def trie_verdicts(subs, topic):
    """Per destination, whether xpub_t::xsend's match marks it (dist_t::match
    is idempotent: a pipe marked twice is marked)."""
    t = Trie()
    for d, prefixes in enumerate(subs):
        for p in prefixes:
            t.add(p, d)
    hit = set()
    t.match(topic, hit.add)
    return [d in hit for d in range(len(subs))]


def edge_table(topic):
    """One destination per prefix kind for a topic, and the verdicts."""
    t = topic
    subs, want = [[b""], [t], [t + b"\x00"], []], [True, True, False, False]
    if t:
        last = t[:-1] + bytes([t[-1] ^ 0x80])
        first = bytes([t[0] ^ 1]) + t[1:]
        subs += [[last], [first], [t[:-1]], [t[:1], t]]  # (the last one: two matching prefixes on one destination)
        want += [False, False, True, True]
    return subs, want


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 300])
def test_prefix_rule_on_the_edge_table(n):
    topic = bytes((7 * i + 1) & 0xff for i in range(n))
    subs, want = edge_table(topic)
    assert [FS.matches(p, topic) for p in subs] == want
    assert trie_verdicts(subs, topic) == want
    assert [FS.matches(p, topic, invert=True) for p in subs] == [not w for w in want]


@pytest.mark.parametrize("seed", range(8))
def test_prefix_rule_on_random_tables(seed):
    """A two-letter alphabet, so that prefixes and topics share long starts."""
    rng = np.random.default_rng(seed)
    word = lambda: bytes(rng.integers(97, 99, int(rng.integers(0, 7)), dtype=np.uint8))
    subs = [[word() for _ in range(int(rng.integers(0, 5)))] for _ in range(12)]
    seen = set()
    for _ in range(60):
        topic = word()
        got = [FS.matches(p, topic) for p in subs]
        assert got == trie_verdicts(subs, topic), topic
        seen.update(got)
    assert seen == {True, False}


def test_heads():
    # consecutive single-part messages: every element is its own head
    assert FS.heads([LAST, LAST, LAST], 3) == [0, 1, 2]
    # a command between the parts changes nothing
    assert FS.heads([MORE, CMD, MORE, LAST, LAST], 5) == [0, None, 0, 0, 4]
    # a command that carries MORE is still a command; one in front of the first part
    assert FS.heads([CMD, MORE, CMD | MORE, LAST, MORE], 4) == [None, 1, None, 1, None]
    # a carry that holds the head (elements 0 and 1), the returned frames bring the tail
    assert FS.heads([MORE, MORE] + [LAST, MORE, LAST], 5) == [0, 0, 0, 3, 3]
    # nothing at or behind held_first has a head
    assert FS.heads([LAST, MORE, MORE], 1) == [0, None, None]
    assert FS.heads([], 0) == []


def test_table_view_bounds():
    idx, off, ln, raw = [0, 2, 1, 9], [0, 1, 3], [1, 2, 4], b"abcdefg"
    # destination 0: both; 1: a falling pair; 2: clamped to n_subs, its prefix within the bytes
    assert FS.table_view(idx, off, ln, raw, 3) == [[b"a", b"bc"], [], [b"bc", b"defg"]]
    # the last prefix runs one byte past sub_bytes_len: it is dropped
    assert FS.table_view(idx, off, ln, raw, 3, sub_bytes_len=6) == [[b"a", b"bc"], [], [b"bc"]]
    assert FS.table_view(idx, off, ln, raw, 3, n_subs=1) == [[b"a"], [], []]


def _args(c):
    return (c["precoms"], c["down"], c["arena"], c["offs"], c["lens"], c["sids"], c["peer"], -1, c["max_frames"],
            c["carry"], c["plain"], c["dst_sid"], c["routes"], c["send"])


@pytest.mark.parametrize("seed", range(4))
def test_empty_prefix_everywhere_is_the_forward_model(seed):
    c = _random_case(seed)
    total = F.model(*_args(c), 2 ** 62, 0, encode=False)["enc"]["frame_off"][-1]
    cap = total - total // 3
    a = F.model(*_args(c), cap, total + 16)
    b = FS.model(*_args(c), [[b""]] * 3, cap, total + 16)
    for k in ("fwd", "base", "N", "pairs", "frame_stream", "flags", "lens", "payloads"):
        assert a[k] == b[k], k
    for k in ("results", "f_off", "f_len", "status", "flags", "out", "peer"):
        assert np.array_equal(a["recv"][k], b["recv"][k]), k
    for k in a["enc"]:
        assert np.array_equal(a["enc"][k], b["enc"][k]), k
    assert b["match"] == [int(p[3]) for p in a["pairs"]]
    # and with no subscriptions at all nothing is live, whatever is forwarded
    n = FS.model(*_args(c), [[]] * 3, cap, total + 16)
    assert not any(n["match"]) and n["fwd"] == a["fwd"] and n["enc"]["send"] == c["send"]
    # inverted, no subscriptions let everything through
    i = FS.model(*_args(c), [[]] * 3, cap, total + 16, invert=True)
    assert i["match"] == b["match"] and (i["enc"]["out"] == a["enc"]["out"]).all()
