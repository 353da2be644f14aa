"""tests/forward_model.py against hand-written cases (no GPU): the rule of what
a source stream forwards, the pair layout, and the send side over the pairs
against tests/zmtp_send_model.py's model called on the live frames alone."""
import numpy as np
import pytest

from tests import forward_model as F
from tests import zmtp_send_model as M

MORE, CMD, LAST = F.MORE, F.COMMAND, 0
ok = lambda *flags: [(f, False) for f in flags]
FAIL = (0, True)  # (a failed frame's flags are 0)


@pytest.mark.parametrize("elements, seq, held_first, forwarded, failed, live", [
    # [more, last, more]: the first message goes, the open one is held
    (ok(MORE, LAST, MORE), 3, 2, 2, 0, [True, True, False]),
    # [cmd, more, cmd, last]: commands neither go nor break the message around them
    (ok(CMD, MORE, CMD, LAST), 4, 4, 2, 0, [False, True, False, True]),
    # a command that carries MORE as well is still a command
    (ok(MORE, CMD | MORE, LAST), 3, 3, 2, 0, [True, False, True]),
    # a command with MORE clear closes nothing
    (ok(MORE, CMD), 2, 0, 0, 0, [False, False]),
    # [ok, FAIL, ok]: what was complete before the failure goes, nothing behind it
    (ok(LAST) + [FAIL] + ok(LAST), 3, 1, 1, 1, [True, False, False]),
    # [more, FAIL]: the incomplete tail of a failed connection is dropped
    (ok(MORE) + [FAIL], 2, 0, 0, 1, [False, False]),
    # [last, more, FAIL, last]: held_first names the open part, failed tells the host to drop it
    (ok(LAST, MORE) + [FAIL] + ok(LAST), 4, 1, 1, 1, [True, False, False, False]),
    # all commands
    (ok(CMD, CMD, CMD), 3, 0, 0, 0, [False, False, False]),
    # a command behind the last complete message is held (the host's to process)
    (ok(LAST, CMD), 2, 1, 1, 0, [True, False]),
    # empty
    ([], 0, 0, 0, 0, []),
    # single-part messages only
    (ok(LAST, LAST, LAST), 3, 3, 3, 0, [True, True, True]),
])
def test_rule(elements, seq, held_first, forwarded, failed, live):
    assert F.rule(elements) == dict(seq=seq, held_first=held_first, forwarded=forwarded, failed=failed, live=live)


def test_rule_with_a_carry():
    """carry [more] + [last]: the carried part leaves with the frame that
    closes its message; carry [more] + nothing stays held; a carried command
    is skipped."""
    assert F.rule(ok(MORE) + ok(LAST)) == dict(seq=2, held_first=2, forwarded=2, failed=0, live=[True, True])
    assert F.rule(ok(MORE)) == dict(seq=1, held_first=0, forwarded=0, failed=0, live=[False])
    assert F.rule(ok(CMD, MORE) + ok(LAST))["live"] == [False, True, True]
    assert F.rule(ok(MORE) + [FAIL])["forwarded"] == 0  # the stream failed: the carried part is dropped too


def test_pair_base_with_uneven_carries_and_routes():
    # c = 1, 0, 3, 0; d = 2, 1, 0, 2; max_frames = 6
    base = F.pair_base([1, 0, 3, 0], [2, 1, 0, 2], 6)
    assert base == [0, 14, 20, 20, 32]
    # p = base(s) + q * d(s) + k enumerates [0, N) once, in (stream, element, route) order
    c, d = [1, 0, 3, 0], [2, 1, 0, 2]
    ps = [base[s] + q * d[s] + k for s in range(4) for q in range(c[s] + 6) for k in range(d[s])]
    assert ps == list(range(32))
    assert F.pair_base([], [], 6) == [0] and F.pair_base([2], [3], 0) == [0, 6] and F.pair_base([0], [3], 0) == [0, 0]


def _random_case(seed):
    rng = np.random.default_rng(seed)
    n_sessions, S, n_dst, max_frames = 5, 4, 3, 5
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n_sessions)]
    down = [False] * n_sessions
    sids, dst_sid = [0, 1, 2, 3], [4, 3, 4]  # (destinations 0 and 2 share session 4)
    streams = []
    for s in range(S):
        parts = [(int(rng.choice([0, 1, 1, 2, 3])), rng.integers(0, 256, int(rng.choice([0, 1, 40, 223, 300])),
                                                                   dtype=np.uint8).tobytes())
                 for _ in range(int(rng.integers(0, 7)))]
        fr = F.source_frames(precoms[sids[s]], parts)
        if fr and rng.integers(0, 3) == 0:  # a tampered tag somewhere
            i = int(rng.integers(0, len(fr)))
            b = bytearray(fr[i])
            b[-1] ^= 1
            fr[i] = bytes(b)
        streams.append(b"".join(fr))
    arena, offs = F.arena_of(streams)
    plain = rng.integers(0, 256, len(arena) + 64, dtype=np.uint8)
    carry = [[(len(arena) + 8 * i, int(rng.integers(0, 8)), int(rng.choice([1, 1, 3]))) for i in range(int(c))]
             for c in rng.integers(0, 3, S)]
    routes = [[int(x) for x in rng.integers(0, n_dst, int(rng.integers(0, 3)))] for _ in range(S)]
    send = [int(x) for x in rng.integers(1, 2 ** 40, n_sessions)]
    return dict(precoms=precoms, down=down, arena=arena, offs=offs, lens=[len(s) for s in streams], sids=sids,
                peer=[2] * n_sessions, max_frames=max_frames, carry=carry, plain=plain, dst_sid=dst_sid,
                routes=routes, send=send)


@pytest.mark.parametrize("seed", range(6))
def test_send_side_is_the_send_model_over_the_live_frames(seed):
    """The pairs that are not live change nothing: zmtp_send_model.model on the
    live frames alone, in pair order, gives the same bytes, the same offsets
    for those frames, the same per-destination results and send counters."""
    c = _random_case(seed)
    m = F.model(c["precoms"], c["down"], c["arena"], c["offs"], c["lens"], c["sids"], c["peer"], -1, c["max_frames"],
                c["carry"], c["plain"], c["dst_sid"], c["routes"], c["send"], 2 ** 62, 0, encode=False)
    total = m["enc"]["frame_off"][-1]
    cap = total - total // 3  # (some frames do not fit)
    m = F.model(c["precoms"], c["down"], c["arena"], c["offs"], c["lens"], c["sids"], c["peer"], -1, c["max_frames"],
                c["carry"], c["plain"], c["dst_sid"], c["routes"], c["send"], cap, total + 16)
    assert m["N"] == len(m["pairs"]) == m["base"][-1]
    live = [p for p in range(m["N"]) if m["pairs"][p][3]]
    assert sum(len(r) * f["forwarded"] for r, f in zip(c["routes"], m["fwd"])) == len(live)
    direct = M.model(c["precoms"], c["down"], c["dst_sid"], [m["frame_stream"][p] for p in live], None,
                     [m["flags"][p] for p in live], [m["lens"][p] for p in live], [m["payloads"][p] for p in live],
                     cap, total + 16, send=c["send"], enc_prefix=F.O.SERVER_PREFIX, dec_prefix=F.O.CLIENT_PREFIX)
    e = m["enc"]
    assert (e["out"] == direct["out"]).all() and e["results"] == direct["results"] and e["send"] == direct["send"]
    assert [e["frame_off"][p] for p in live] + [e["frame_off"][-1]] == direct["frame_off"]
    assert [e["status"][p] for p in live] == direct["status"]
    dead = [p for p in range(m["N"]) if not m["pairs"][p][3]]
    assert all(e["status"][p] == F.ERR_SESSION and e["frame_off"][p] == M.UINT64_MAX for p in dead)
    # every live pair is a non-command part of a whole message, with its MORE bit alone
    for s, f in enumerate(m["fwd"]):
        assert f["held_first"] <= f["seq"] == len(c["carry"][s]) + m["recv"]["results"][s]["frames"]
    assert all(fl in (0, 1) for fl in m["flags"])
