"""tests/forward_credit_model.py against a sequential restatement of the
reference (CPU only).  The restatement knows nothing of pairs: it walks every
stream's parts in order, completes messages as pipe_t::write does
(src/pipe.cpp:222-234), hands each to its pipes in route order and asks every
pipe's check_write (src/pipe.cpp:207-220, check_hwm :535-541: full when hwm > 0
and msgs_written - peers_msgs_read >= hwm) at the first part; a pipe that
refuses is out for the rest of the call (dist_t::write, src/dist.cpp:196-210),
and a ROUTER drops the message for its one peer (router_t::xsend,
src/router.cpp:185-200).  What each pipe was handed, part by part, must be what
the model's pairs hold for that destination in pair order.  With every credit
unlimited the model is forward_framed_model.model."""
import numpy as np
import pytest

from tests import forward_credit_model as FC
from tests import forward_framed_model as FM
from tests import forward_model as F
from tests import forward_router_model as FR

MORE, CMD, LAST = F.MORE, F.COMMAND, 0
PEER0 = 2
UNL = FC.UNLIMITED
TOPICS = [b"a", b"ab", b"b", b""]
IDS = [b"idA", b"idB", b"\x00x", b"nobody"]


def _rng_bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _messages(rng, mode):
    """One stream's parts: messages of 1-3 parts whose first part is a topic or
    an address, commands between parts, sometimes an open message at the end."""
    parts = []
    for _ in range(int(rng.integers(0, 5))):
        n = int(rng.integers(1, 4))
        first = {FM.SUB: TOPICS, FM.ROUTER: IDS}.get(mode, [b"x"])
        first = first[int(rng.integers(len(first)))] + (_rng_bytes(rng, 2) if mode != FM.ROUTER else b"")
        for i in range(n):
            if rng.random() < 0.15:
                parts.append((CMD, _rng_bytes(rng, 3)))
            parts.append((MORE if i + 1 < n else LAST, first if i == 0 else _rng_bytes(rng, int(rng.integers(0, 12)))))
    if rng.random() < 0.3:
        parts.append((MORE, _rng_bytes(rng, 4)))
    return parts


def _case(seed, mode):
    rng = np.random.default_rng(seed)
    S, D = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    precoms = [_rng_bytes(rng, 32) for _ in range(S + D)]
    parts = [_messages(rng, mode) for _ in range(S)]
    # the first parts of some streams were held back by an earlier call: they arrive through the carry
    ncar = [int(rng.integers(0, min(len(p), 3) + 1)) if rng.random() < 0.4 else 0 for p in parts]
    max_frames = int(rng.integers(1, 9))
    streams = [b"".join(F.source_frames(precoms[s], p[ncar[s]:])) for s, p in enumerate(parts)]
    arena, offs = F.arena_of(streams)
    park, carry = bytearray(), []
    for s, p in enumerate(parts):
        carry.append([])
        for fl, pay in p[:ncar[s]]:
            carry[s].append((len(arena) + len(park), len(pay), fl))
            park += pay
    src_ids = []
    for s in range(S):
        i = IDS[int(rng.integers(len(IDS)))]
        src_ids.append((len(arena) + len(park), len(i)))
        park += i
    plain = np.concatenate([np.full(len(arena), 0x77, np.uint8), np.frombuffer(bytes(park), np.uint8)])
    routes = [[int(t) for t in rng.integers(0, D, int(rng.integers(0, 4)))] for _ in range(S)]
    kw = {}
    if mode == FM.SUB:
        kw = dict(subs=[[TOPICS[int(j)] for j in rng.integers(0, 3, int(rng.integers(0, 3)))] for _ in range(D)],
                  invert=bool(rng.random() < 0.2))
    if mode == FM.ROUTER:
        known = [(i, int(rng.integers(0, D))) for i in IDS[:3] if rng.random() < 0.8]
        kw = dict(flags=int(rng.integers(1, 4)), src_ids=src_ids, table=FR.table_of(known))
    credit = [[0, 1, 2, 3, UNL][int(rng.integers(5))] for _ in range(D)]
    Q = [p[:ncar[s]] + p[ncar[s]:ncar[s] + max_frames] for s, p in enumerate(parts)]
    ids = [plain[o:o + n].tobytes() for o, n in src_ids]
    return dict(mode=mode, S=S, D=D, precoms=precoms, arena=arena, offs=offs, lens=[len(x) for x in streams],
                carry=carry, plain=plain, routes=routes, kw=kw, credit=credit, max_frames=max_frames, Q=Q, ids=ids,
                send=[1] * (S + D))


class Pipe:
    """pipe_t's send side as far as the high-water mark goes; the peer reads nothing during the call."""

    def __init__(self, credit, rng):
        if credit == UNL:
            self.hwm, self.written = 0, int(rng.integers(0, 100))
        else:  # credit = hwm - (msgs_written - peers_msgs_read)
            self.written = int(rng.integers(1, 50))
            self.hwm = self.written + credit
        self.read, self.got, self.refused = 0, [], 0

    def check_write(self):
        return not (self.hwm > 0 and self.written - self.read >= self.hwm)

    def write(self, part):
        self.got.append(part)
        if not part[0] & MORE:
            self.written += 1


def _sequential(c):
    """What every pipe is handed, by the reference's rules alone."""
    rng = np.random.default_rng(99)
    pipes = [Pipe(x, rng) for x in c["credit"]]
    mode, kw = c["mode"], c["kw"]
    fl = kw.get("flags", 0) if mode == FM.ROUTER else 0
    prepend, route = bool(fl & FR.PREPEND), bool(fl & FR.ROUTE)
    table = dict((bytes(i), d) for i, d in zip(
        [kw["table"]["raw"][o:o + n] for o, n in zip(kw["table"]["off"], kw["table"]["len"])],
        kw["table"]["dst"])) if route else {}
    for s in range(c["S"]):
        msg = []
        for flags, pay in c["Q"][s]:
            if flags & CMD:
                continue
            msg.append((flags & MORE, pay))
            if flags & MORE:
                continue
            # a whole message: what goes out, and to whom
            out = ([(MORE, c["ids"][s])] if prepend else []) + msg
            msg = []
            if route:
                if len(out) < 2:
                    continue  # an address that is the whole message
                to = [table[out[0][1]]] if out[0][1] in table else []
                out = out[1:]
            elif mode == FM.SUB:
                hit = lambda t: any(out[0][1].startswith(p) for p in kw["subs"][t]) != kw["invert"]
                to = [t for t in c["routes"][s] if hit(t)]
            else:
                to = list(c["routes"][s])
            # check_write at the first part, slot by slot.  A destination named twice is two deliveries: the
            # second slot sees the message the first one has begun (the reference has no such pipe; the header
            # defines it so).  Then the parts, each to every admitted slot, as dist_t::distribute walks them.
            admitted = []
            for t in to:
                pipes[t].written += admitted.count(t)
                ok = pipes[t].check_write()
                pipes[t].written -= admitted.count(t)
                if ok:
                    admitted.append(t)
                else:
                    pipes[t].refused += 1
            for part in out:
                for t in admitted:
                    pipes[t].write(part)
    return pipes


def _run(c, credit, **over):
    return FC.model(c["mode"], FM.ZMTP, FM.ZMTP, credit, c["precoms"], [False] * len(c["precoms"]), c["arena"],
                    c["offs"], c["lens"], list(range(c["S"])), [PEER0] * len(c["precoms"]), -1, c["max_frames"],
                    c["carry"], c["plain"], list(range(c["S"], c["S"] + c["D"])), c["send"], None, 16,
                    routes=c["routes"], encode=False, **dict(c["kw"], **over))


@pytest.mark.parametrize("mode", [FM.STATIC, FM.SUB, FM.ROUTER])
def test_model_is_the_reference_walk(mode):
    seen = dict(dropped=0, taken=0, cut=0)
    for seed in range(120):
        c = _case(1000 * mode + seed, mode)
        m = _run(c, c["credit"])
        pipes = _sequential(c)
        for t, pipe in enumerate(pipes):
            mine = [(m["flags"][p], m["payloads"][p]) for p in range(m["N"]) if m["frame_stream"][p] == t]
            assert mine == pipe.got, (seed, t)
            done = sum(1 for f, _ in pipe.got if not f & MORE)
            assert (m["taken"][t], m["dropped"][t]) == (done, pipe.refused), (seed, t)
            assert pipe.hwm == 0 or pipe.written - pipe.read <= pipe.hwm
            seen["cut"] += bool(done and pipe.refused)
        # a cleared pair was live in the plan, and only such a pair is cleared
        plan = FM.plan(c["mode"], c["precoms"], [False] * len(c["precoms"]), c["arena"], c["offs"], c["lens"],
                       list(range(c["S"])), [PEER0] * len(c["precoms"]), -1, c["max_frames"], c["carry"], c["plain"],
                       list(range(c["S"], c["S"] + c["D"])), c["send"], routes=c["routes"], **c["kw"])
        for p in range(m["N"]):
            if m["hwm"][p]:
                assert plan["frame_stream"][p] != F.NO_STREAM and m["frame_stream"][p] == F.NO_STREAM
                assert m["enc"]["status"][p] == FC.ERR_HWM
            else:
                assert m["frame_stream"][p] == plan["frame_stream"][p]
        for k in ("match", "dest"):  # the routing decision is reported as before
            if k in plan:
                assert m[k] == plan[k]
        assert m["credit_after"] == c["credit"]
        seen["dropped"] += sum(m["dropped"])
        seen["taken"] += sum(m["taken"])
    assert seen["dropped"] > 50 and seen["taken"] > 50 and seen["cut"] > 10


@pytest.mark.parametrize("mode", [FM.STATIC, FM.SUB, FM.ROUTER])
def test_unlimited_is_the_framed_model(mode):
    for seed in range(25):
        c = _case(5000 * (mode + 1) + seed, mode)
        m = _run(c, [UNL] * c["D"], consume=True)
        own = FM.model(c["mode"], FM.ZMTP, FM.ZMTP, c["precoms"], [False] * len(c["precoms"]), c["arena"], c["offs"],
                       c["lens"], list(range(c["S"])), [PEER0] * len(c["precoms"]), -1, c["max_frames"], c["carry"],
                       c["plain"], list(range(c["S"], c["S"] + c["D"])), c["send"], None, 16, routes=c["routes"],
                       encode=False, **c["kw"])
        for k in ("fwd", "base", "N", "pairs", "frame_stream", "flags", "lens", "payloads", "total", "cap", "size"):
            assert m[k] == own[k], k
        for k in ("frame_off", "status", "results", "send"):
            assert m["enc"][k] == own["enc"][k], k
        assert not any(m["hwm"]) and m["dropped"] == [0] * c["D"] and m["credit_after"] == [UNL] * c["D"]
        assert sum(m["taken"]) == len(FC.deliveries(own, mode, c["kw"], c["carry"], c["routes"], c["max_frames"]))


def test_consume():
    """credit - taken is written back, and unlimited stays."""
    c = _case(7, FM.STATIC)
    c["credit"] = [1, UNL, 0][:c["D"]] + [2] * max(c["D"] - 3, 0)
    m = _run(c, c["credit"], consume=True)
    for t, (x, k, a) in enumerate(zip(c["credit"], m["taken"], m["credit_after"])):
        assert a == (UNL if x == UNL else x - k) and (x == UNL or k <= x)
