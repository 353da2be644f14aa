"""tests/subs_update_model.py, the model the GPU tests of
zmqg_subs_update_multi compare against, held against a fresh restatement of the
reference: xpub_t::xread_activated (src/xpub.cpp:72-170) and
xpub_t::xpipe_terminated (src/xpub.cpp:253-277) over a trie whose nodes carry
pipe sets (generic_mtrie_t::add / rm, src/generic_mtrie_impl.hpp:41-126,
376-521).  Random command sequences over several calls, the verbose flags
included: the per-pipe prefix sets and the notification sequences agree.  In
these runs cap is at least the number of distinct topics and slot_bytes at
least the longest, so no command is FULL or TOO_LONG and none is left out of
the comparison; capacity, classification and hostile stores are checked against
statements of their own."""
import numpy as np
import pytest

from tests import subs_update_model as U


class _Node:
    def __init__(self):
        self.pipes, self.next = None, {}


class _Xpub:
    """The reference's XPUB, subscription side: a trie of pipe sets."""

    def __init__(self, verbose_subs=False, verbose_unsubs=False):
        self.root, self.verbose_subs, self.verbose_unsubs, self.pending = _Node(), verbose_subs, verbose_unsubs, []

    def _add(self, prefix, pipe):  # generic_mtrie_t::add: true when the node had no pipes
        node = self.root
        for ch in prefix:
            node = node.next.setdefault(ch, _Node())
        first = node.pipes is None
        if first:
            node.pipes = set()
        node.pipes.add(pipe)
        return first

    def _rm(self, prefix, pipe):  # generic_mtrie_t::rm (prefix, pipe): the three results
        node = self.root
        for ch in prefix:
            node = node.next.get(ch)
            if node is None:
                return "not_found"
        if node.pipes is None:
            return "not_found"
        erased = pipe in node.pipes
        node.pipes.discard(pipe)
        if not node.pipes:
            assert erased
            node.pipes = None
            return "last_value_removed"
        return "values_remain" if erased else "not_found"

    def read(self, pipe, data, is_command):
        """xread_activated for one message of `pipe` (not manual, every part processed)."""
        kind, skip = U.classify(data, U.COMMAND if is_command else 0)
        if not kind:
            return
        topic = data[skip:]
        if kind == U.CANCEL:
            notify = self._rm(topic, pipe) != "values_remain" or self.verbose_unsubs
        else:
            notify = self._add(topic, pipe) or self.verbose_subs
        if notify:
            self.pending.append((kind == U.SUBSCRIBE, topic))

    def terminated(self, pipe):
        """xpipe_terminated: rm (pipe, send_unsubscription, this, !verbose_unsubs)."""
        out = []

        def walk(node, prefix):
            if node.pipes is not None and pipe in node.pipes:
                node.pipes.discard(pipe)
                empty = not node.pipes
                if empty:
                    node.pipes = None
                if self.verbose_unsubs or empty:  # (call_on_uniq = !verbose_unsubs)
                    out.append((False, prefix))
            for ch, nxt in sorted(node.next.items()):
                walk(nxt, prefix + bytes([ch]))

        walk(self.root, b"")
        self.pending += out
        return out

    def held(self, n_pipes):
        sets = [set() for _ in range(n_pipes)]

        def walk(node, prefix):
            for p in node.pipes or ():
                sets[p].add(prefix)
            for ch, nxt in node.next.items():
                walk(nxt, prefix + bytes([ch]))

        walk(self.root, b"")
        return sets


def _payload(rng, subscribe, topic):
    """(msg_t flags, payload) of a subscription element, in one of its two forms."""
    if rng.integers(2):
        return U.COMMAND, (b"\x09SUBSCRIBE" if subscribe else b"\x06CANCEL") + topic
    return 0, bytes([int(subscribe)]) + topic


@pytest.mark.parametrize("flags", [0, U.VERBOSE, U.VERBOSER, U.VERBOSE | U.VERBOSER])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_against_the_reference_restated(flags, seed):
    rng = np.random.default_rng(100 * seed + flags)
    D, MF = 5, 9
    topics = [b"", b"a", b"ab", b"abc", b"b", b"abd", bytes(range(12)), bytes(range(11)) + b"\xff"]
    store = U.empty_store(D, len(topics), 16)
    verbose = bool(flags & (U.VERBOSE | U.VERBOSER))
    ref = _Xpub(verbose, bool(flags & U.VERBOSER))
    for call in range(8):
        gone = [int(t) for t in rng.permutation(D)[:rng.integers(0, 3)]] if call else []
        live = [t for t in rng.permutation(D) if t not in gone][:rng.integers(1, D + 1)]
        streams = []
        for t in live:
            st = []
            for _ in range(rng.integers(0, MF + 1)):
                r = rng.integers(10)
                if r == 0:
                    st.append((U.COMMAND, b"\x04PING", 0))  # dropped by the session
                elif r == 1:
                    st.append((0, b"\x02user", 0))  # an XPUB user message: no subscription element
                else:
                    fl, p = _payload(rng, r < 6, topics[rng.integers(len(topics))])
                    st.append((fl | (U.MORE if rng.integers(4) == 0 else 0), p, 0))
            streams.append(st)
        m = U.update(store, U.craft(streams, MF), MF, live, gone, flags)
        store = m["store"]
        # the reference: the terminated pipes, then every pipe's messages in order
        ref.pending, cleared = [], []
        for t in gone:
            cleared += ref.terminated(t)
        n_clear = len(cleared)
        for t, st in zip(live, streams):
            for fl, p, _ in st:
                ref.read(int(t), p, bool(fl & U.COMMAND))
        assert [set(d) for d in U.prefixes(store)] == ref.held(D), call
        assert all(len(set(d)) == len(d) for d in U.prefixes(store))
        # a pipe's prefixes leave the trie in trie order, the store's in slot order: the clears as sorted lists
        assert sorted(m["notes"][:n_clear]) == sorted(cleared) and m["notes"][n_clear:] == ref.pending[n_clear:], call
        assert sum(m["clear_note"].values()) == n_clear
        assert not any(s in (U.FULL, U.TOO_LONG) for s in m["sub_status"])
        assert sum(r["notes"] for r in m["results"]) == len(m["notes"]) - n_clear
        # the view names every live slot
        raw = store["bytes"].tobytes()
        view = [[raw[int(m["sub_off"][j]):int(m["sub_off"][j]) + int(m["sub_len"][j])]
                 for j in range(int(m["sub_idx"][t]), int(m["sub_idx"][t + 1]))] for t in range(D)]
        assert view == U.prefixes(store)


def test_classification_edges():
    S, C = U.SUBSCRIBE, U.CANCEL
    for p, fl, want in [(b"", U.COMMAND, (0, 0)), (b"", 0, (0, 0)), (b"\x09SUBSCRIBE", U.COMMAND, (S, 10)),
                        (b"\x09SUBSCRIB", U.COMMAND, (0, 0)), (b"\x09SUBSCRIBX", U.COMMAND, (0, 0)),
                        (b"\x06CANCEL", U.COMMAND, (C, 7)), (b"\x06CANCE", U.COMMAND, (0, 0)),
                        (b"\x06CANCELxy", U.COMMAND, (C, 7)), (b"\x04PING", U.COMMAND, (0, 0)),
                        (b"\x40AB", U.COMMAND, (0, 0)), (b"\x01", U.COMMAND, (0, 0)), (b"\x01", 0, (S, 1)),
                        (b"\x00", 0, (C, 1)), (b"\x02", 0, (0, 0)), (b"\x01abc", U.MORE, (S, 1)),
                        (b"\x09SUBSCRIBE", 0, (0, 0))]:
        assert U.classify(p, fl) == want, (p, fl)


def test_capacity_and_length():
    """FULL at cnt == cap and TOO_LONG change nothing and do not notify; a
    cancel frees a slot (the last one moves into the hole); a cancel of a topic
    longer than slot_bytes is NOT_FOUND and, like every not-found, notifies."""
    store = U.store_of([[b"x", b"y"]], 2, 8)
    cmds = [(0, b"\x01z", 0), (0, b"\x01" + b"q" * 9, 0), (0, b"\x00" + b"q" * 9, 0), (0, b"\x00x", 0),
            (0, b"\x01z", 0), (0, b"\x01z", 0)]
    m = U.update(store, U.craft([cmds], 6), 6, [0])
    assert list(m["sub_status"]) == [U.FULL, U.TOO_LONG, U.NOT_FOUND, U.REMOVED, U.ADDED, U.DUPLICATE]
    assert list(m["note_stream"]) == [U.NO_NOTE, U.NO_NOTE, 0, 0, 0, U.NO_NOTE]
    assert U.prefixes(m["store"]) == [[b"y", b"z"]]
    assert m["results"] == [dict(seen=6, changed=2, notes=3, rejected=2)]


def test_order_of_verdicts_and_a_failed_stream():
    """H is taken in (stream, slot) order whatever destination a stream edits;
    nothing at or behind a failed frame is examined."""
    store = U.store_of([[b"t"], [], []], 4, 8)
    sub, can = (0, b"\x01t", 0), (0, b"\x00t", 0)
    m = U.update(store, U.craft([[can], [sub]], 1), 1, [0, 1])
    assert m["notes"] == [(False, b"t"), (True, b"t")]  # the last holder leaves, then a first one arrives
    m = U.update(store, U.craft([[sub], [can]], 1), 1, [1, 0])
    assert m["notes"] == []  # a second holder arrives, then one of two leaves
    m = U.update(store, U.craft([[sub, (0, b"\x01u", 0x10000011), (0, b"\x01v", 0)]], 3), 3, [2])
    assert list(m["sub_status"]) == [U.ADDED, U.NONE, U.NONE] and U.prefixes(m["store"])[2] == [b"t"]
    m = U.update(store, U.craft([[sub, sub]], 2, frames=[1]), 2, [2])
    assert list(m["note_flags"]) == [U.SUBSCRIBE, 0]


def test_hostile_store_is_read_under_the_clamps():
    store = U.store_of([[b"aa", b"bb"], [b"aa"]], 2, 8)
    store["cnt"][0] = 2 + 7
    store["slot_len"][1] = 0xffffffff
    assert U.prefixes(store) == [[b"aa", b"bb" + bytes(6)], [b"aa"]]
    m = U.update(store, U.craft([[(0, b"\x00aa", 0)]], 1), 1, [0])
    assert list(m["sub_status"]) == [U.REMOVED] and list(m["note_stream"]) == [U.NO_NOTE]
    assert U.prefixes(m["store"]) == [[b"bb" + bytes(6)], [b"aa"]] and int(m["store"]["cnt"][0]) == 1
    assert list(m["sub_idx"]) == [0, 1, 2]


def test_invalid_cases():
    ok = dict(n_dst=3, cap=2, slot_bytes=8, n_streams=2, max_frames=4, stream_dst=[0, 2], clear_dst=[1])
    assert not U.invalid(**ok)
    for change in (dict(n_dst=8193), dict(cap=0), dict(slot_bytes=12), dict(slot_bytes=0), dict(slot_bytes=65544),
                   dict(n_dst=8192, cap=2 ** 18), dict(max_frames=2 ** 31), dict(n_streams=2 ** 16, max_frames=2 ** 15),
                   dict(stream_dst=[0, 0]), dict(stream_dst=[0, 3]), dict(clear_dst=[2]), dict(clear_dst=[1, 1]),
                   dict(flags=1), dict(flags=8)):
        assert U.invalid(**dict(ok, **change)), change
