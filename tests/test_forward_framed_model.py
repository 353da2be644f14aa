"""tests/forward_framed_model.py against the pieces it composes (CPU only):
with both framings ZMTP it is the mode's own model; its WebSocket receive side
is ws_model.parse on a hand-written stream with a ping in the middle; and the
plan it makes of a WebSocket input is the plan the mode's model makes of the
same MESSAGE bodies in ZMTP frames."""
import numpy as np
import pytest

from oracle import zmtp_oracle as Z
from tests import forward_framed_model as FM
from tests import forward_lb_model as FL
from tests import forward_model as F
from tests import forward_router_model as FR
from tests import forward_sub_model as FS
from tests import ws_model as W

MORE, CMD, LAST = F.MORE, F.COMMAND, 0
PEER0 = 2


def _rng_bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _parts(rng):
    """Three streams' parts: whole messages with a command between, a held tail; an address and a body."""
    pay = lambda n: _rng_bytes(rng, n)
    return [[(LAST, b"news" + pay(9)), (CMD, pay(5)), (MORE, b"nope" + pay(3)), (LAST, pay(30)), (MORE, pay(2))],
            [(MORE, b"idA"), (LAST, pay(12)), (LAST, b"new")],
            [(LAST, pay(1))]]


def _setup(seed=17):
    rng = np.random.default_rng(seed)
    precoms = [_rng_bytes(rng, 32) for _ in range(5)]
    parts = _parts(rng)
    ids = [b"\x00peer0", b"idA", b"zz"]
    return rng, precoms, parts, ids


def _plain_with_ids(n, ids):
    """A `plain` of n FILL bytes with the ids parked behind it; returns (plain, src_ids)."""
    buf, src_ids = bytearray(), []
    for i in ids:
        src_ids.append((n + len(buf), len(i)))
        buf += i
    return np.concatenate([np.full(n, 0x77, np.uint8), np.frombuffer(bytes(buf), np.uint8)]), src_ids


def _mode_kw(mode, ids_at):
    """(framed model keywords, routes) for a mode over 3 streams and 2 destinations."""
    routes = [[0, 1], [1], [0, 0]]
    if mode == FM.SUB:
        return dict(subs=[[b"new"], []]), routes
    if mode == FM.ROUTER:
        return dict(flags=FR.ROUTE, src_ids=None, table=FR.table_of([(b"idA", 1), (b"idB", 0)])), routes
    if mode == FM.LB:
        return dict(flags=FL.PREPEND, src_ids=ids_at, stream_group=[0, 0, FL.NO_GROUP],
                    table=dict(grp_idx=[0, 2], lb_dst=[1, 0], lb_cur=[1], n_lb=2)), None
    return {}, routes


def _own_model(mode, common, routes, send, kw, cap, size):
    if mode == FM.STATIC:
        return F.model(*common, routes, send, cap, size)
    if mode == FM.SUB:
        return FS.model(*common, routes, send, kw["subs"], cap, size)
    if mode == FM.ROUTER:
        return FR.model(*common, routes, send, kw["flags"], kw["src_ids"], kw["table"], cap, size)
    return FL.model(*common, send, kw["flags"], kw["src_ids"], kw["stream_group"], kw["table"], cap, size)


PLAN_KEYS = ("fwd", "base", "N", "pairs", "frame_stream", "flags", "lens", "payloads")
EXTRA = {FM.STATIC: (), FM.SUB: ("match",), FM.ROUTER: ("dest",), FM.LB: ("dest", "lb_cur")}


@pytest.mark.parametrize("mode", [FM.STATIC, FM.SUB, FM.ROUTER, FM.LB])
def test_both_zmtp_is_the_modes_own_model(mode):
    rng, precoms, parts, ids = _setup()
    streams = [b"".join(F.source_frames(precoms[s], p)) for s, p in enumerate(parts)]
    arena, offs = F.arena_of(streams)
    plain, ids_at = _plain_with_ids(len(arena), ids)
    kw, routes = _mode_kw(mode, ids_at)
    send = [1, 1, 1, 9, 2 ** 32 - 1]
    common = (precoms, [False] * 5, arena, offs, [len(s) for s in streams], [0, 1, 2], [PEER0] * 5, -1, 6,
              [[], [], []], plain, [3, 4])
    m = FM.model(mode, FM.ZMTP, FM.ZMTP, *common, send, None, 64, routes=routes, **kw)
    own = _own_model(mode, common, routes, send, kw, m["cap"], m["size"])
    for k in PLAN_KEYS + EXTRA[mode]:
        assert m[k] == own[k], k
    for k in ("frame_off", "status", "results", "send"):
        assert m["enc"][k] == own["enc"][k], k
    assert (m["enc"]["out"] == own["enc"]["out"]).all() and m["total"] == own["enc"]["frame_off"][-1] > 0
    for k in ("results", "peer"):
        assert m["recv"][k] == own["recv"][k]
    for k in ("f_off", "f_len", "status", "flags", "out"):
        assert (m["recv"][k] == own["recv"][k]).all(), k


@pytest.mark.parametrize("masked", [False, True])
def test_ws_receive_is_ws_model_parse(masked):
    """binary, ping, binary: the parse ends behind the ping, whose payload is
    reported (and unmasked); the first frame alone is returned and decoded."""
    rng, precoms, parts, _ = _setup(23)
    b = FM.bodies(precoms[0], [(LAST, b"first"), (MORE, b"second")])
    key = (lambda k: k) if masked else (lambda k: None)
    stream = (W.frame(b[0], key(0x01020304), 0) + W.frame(b"ping", key(0xA1B2C3D4), opcode=W.OP_PING) +
              W.frame(b[1], key(0x0F0E0D0C), W.MORE))
    arena, offs = F.arena_of([stream])
    r = FM.ws_receive(arena, offs, [len(stream)], [0], precoms[:1], [PEER0], masked, -1, 4)
    p = W.parse(stream, masked, -1, 4)
    assert len(p["frames"]) == 1 and p["ctl"][0] == W.OP_PING and p["error"] == 0
    hdr = 2 + (4 if masked else 0)
    assert p["consumed"] == len(W.frame(b[0], key(1), 0)) + hdr + 4 < len(stream)
    res = r["results"][0]
    assert (res["frames"], res["consumed"], res["error"]) == (1, p["consumed"], 0)
    assert (res["ctl_opcode"], res["ctl_off"], res["ctl_len"]) == (9, offs[0] + p["ctl"][1], 4)
    assert res["out_bytes"] == 5
    assert r["plain"][res["ctl_off"]:res["ctl_off"] + 4].tobytes() == b"ping"
    fl, boff, size, _ = p["frames"][0]
    assert (int(r["f_off"][0]), int(r["f_len"][0])) == (offs[0] + boff, size) and size == len(b[0])
    assert r["plain"][offs[0] + boff:offs[0] + boff + size].tobytes() == b[0]
    assert r["status"][0] == 0 and r["flags"][0] == 0 and (r["status"][1:] != 0).all()
    assert r["out"][int(r["f_off"][0]):int(r["f_off"][0]) + 5].tobytes() == b"first"
    assert r["peer"] == [3]  # the nonce of the one frame decoded
    # the second call, from `consumed`: the frame behind the ping, its MORE bit from the WebSocket flags byte
    o2 = offs[0] + res["consumed"]
    r2 = FM.ws_receive(arena, [o2], [len(stream) - res["consumed"]], [0], precoms[:1], r["peer"], masked, -1, 4)
    assert r2["results"][0]["frames"] == 1 and r2["status"][0] == 0 and r2["flags"][0] == MORE
    assert r2["results"][0]["consumed"] == len(stream) - res["consumed"] and r2["peer"] == [4]


@pytest.mark.parametrize("mode", [FM.STATIC, FM.SUB, FM.ROUTER, FM.LB])
def test_the_plan_of_a_ws_input_is_its_zmtp_twins(mode):
    """The same MESSAGE bodies in masked WebSocket frames and in ZMTP frames:
    the same plan from the mode's model, a control frame cutting one stream."""
    rng, precoms, parts, ids = _setup(29)
    bodies = [FM.bodies(precoms[s], p) for s, p in enumerate(parts)]
    keys = lambda n: [int(k) for k in rng.integers(0, 2 ** 32, n)]
    ws = [b"".join(W.frame(b, k, 0) for b, k in zip(bs, keys(len(bs)))) for bs in bodies]
    # stream 1 ends at a pong in front of its last frame: the twin holds the two frames before it
    cut = sum(len(W.frame(b, 0, 0)) for b in bodies[1][:2])
    ws[1] = ws[1][:cut] + W.frame(b"", 7, opcode=W.OP_PONG) + ws[1][cut:]
    zs = [b"".join(Z.frame(b) for b in bs) for bs in (bodies[0], bodies[1][:2], bodies[2])]
    arena, offs = F.arena_of(ws)
    zarena, zoffs = F.arena_of(zs)
    n = max(len(arena), len(zarena))
    plain, ids_at = _plain_with_ids(n, ids)
    kw, routes = _mode_kw(mode, ids_at)
    send = [1, 1, 1, 9, 2 ** 32 - 1]
    tail = ([0, 1, 2], [PEER0] * 5, -1, 6, [[], [], []], plain, [3, 4])
    m = FM.model(mode, FM.WS_MASKED, FM.WS_PLAIN, precoms, [False] * 5, arena, offs, [len(s) for s in ws], *tail, send,
                 None, 64, routes=routes, encode=False, **kw)
    own = _own_model(mode, (precoms, [False] * 5, zarena, zoffs, [len(s) for s in zs]) + tail, routes, send, kw,
                     2 ** 62, 0)
    assert [r["frames"] for r in m["recv"]["results"]] == [5, 2, 1] and m["recv"]["results"][1]["ctl_opcode"] == 10
    assert m["twin"][2] == [len(s) for s in zs]
    for k in PLAN_KEYS + EXTRA[mode]:
        assert m[k] == own[k], k
    assert sum(p[3] for p in m["pairs"]) > 0
    assert m["enc"]["send"] == own["enc"]["send"] and m["enc"]["status"] == own["enc"]["status"]
    assert m["recv"]["peer"] == own["recv"]["peer"]
