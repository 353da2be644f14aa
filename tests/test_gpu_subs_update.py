"""zmqg_subs_update_multi: the XPUB subscription store kept on the device, against
tests/subs_update_model.py.  Bit for bit: every per-slot output, results_out,
sub_idx, clear_cnt, clear_len, clear_note.  As per-destination sets: the store
and the published view.  Every output region the contract leaves alone is
prefilled with a sentinel and must keep it.  The inputs are crafted device
arrays (subs_update_model.craft: no crypto) except in the end-to-end case."""
import ctypes

import numpy as np
import pytest

from tests import subs_update_model as U

S32, S64, S8 = -3, -3, 0xCC  # sentinels of the int32 / int64 / uint8 outputs
SUB, CAN = (lambda t: (0, b"\x01" + t, 0)), (lambda t: (0, b"\x00" + t, 0))            # what a downgrade_sub peer sends
CSUB, CCAN = (lambda t: (U.COMMAND, b"\x09SUBSCRIBE" + t, 0)), (lambda t: (U.COMMAND, b"\x06CANCEL" + t, 0))


def _t(torch, a, dt, vt):
    a = np.ascontiguousarray(a, dt)
    return torch.from_numpy((a if a.size else np.zeros(1, dt)).view(vt)).to(torch.device("cuda", 0))


def _dev_store(torch, st):
    """The model's store on the device, the view's arrays at their sentinels."""
    dev, n = torch.device("cuda", 0), max(st["n_dst"] * st["cap"], 1)
    return dict(n_dst=st["n_dst"], cap=st["cap"], slot_bytes=st["slot_bytes"], cnt=_t(torch, st["cnt"], np.uint32, np.int32),
                slot_len=_t(torch, st["slot_len"], np.uint32, np.int32), bytes=_t(torch, st["bytes"], np.uint8, np.uint8),
                sub_idx=torch.full((st["n_dst"] + 1,), S32, dtype=torch.int32, device=dev),
                sub_off=torch.full((n,), S64, dtype=torch.int64, device=dev),
                sub_len=torch.full((n,), S32, dtype=torch.int32, device=dev))


def _buffers(torch, recv, S, MF, store, n_clear):
    """The decode call's outputs on the device and this call's outputs at their sentinels."""
    dev, n, g = torch.device("cuda", 0), max(S * MF, 1), max(store["n_dst"] * store["cap"], 1)
    res = np.array([[r["frames"], r["consumed"], r["out_bytes"], r["error"]] for r in recv["results"]] or [[0] * 4],
                   np.uint64)
    full = lambda k, v, dt: torch.full((k,), v, dtype=dt, device=dev)
    return dict(results=_t(torch, res, np.uint64, np.int64), frame_len=_t(torch, recv["f_len"], np.uint32, np.int32),
                plain_off=_t(torch, recv["f_off"], np.uint64, np.int64), flags_out=_t(torch, recv["flags"], np.uint8, np.uint8),
                status_out=_t(torch, recv["status"].astype(np.uint32), np.uint32, np.int32),
                plain=_t(torch, recv["out"], np.uint8, np.uint8),
                sub_status=full(n, S32, torch.int32), topic_off=full(n, S64, torch.int64),
                topic_len=full(n, S32, torch.int32), note_flags=full(n, S8, torch.uint8),
                note_stream=full(n, S32, torch.int32),
                results_out=torch.full((max(S, 1), 4), S64, dtype=torch.int64, device=dev),
                clear_cnt=full(max(n_clear, 1), S32, torch.int32), clear_len=full(g, S32, torch.int32),
                clear_note=full(g, S8, torch.uint8))


INPUTS = ("results", "frame_len", "plain_off", "flags_out", "status_out", "plain")
OUTPUTS = ("sub_status", "topic_off", "topic_len", "note_flags", "note_stream", "results_out")
CLEARS = ("clear_cnt", "clear_len", "clear_note")


def _call(ctx, d_store, b, stream_dst, MF, clear_dst=(), flags=0):
    ctx.subs_update_multi(d_store, stream_dst, MF, *[b[k] for k in INPUTS + OUTPUTS], clear_dst=list(clear_dst),
                          **{k: b[k] for k in CLEARS}, flags=flags)


def _check(torch, C, d_store, b, m, S, MF, clear_dst=()):
    """Everything the call has written, and left alone, against the model's result m."""
    torch.cuda.synchronize()
    n, st = S * MF, m["store"]
    u32 = lambda x: x.cpu().numpy().view(np.uint32)
    assert (b["sub_status"].cpu().numpy()[:n] == m["sub_status"]).all(), (b["sub_status"].cpu().numpy()[:n], m["sub_status"])
    assert (b["topic_off"].cpu().numpy().view(np.uint64)[:n] == m["topic_off"]).all()
    assert (u32(b["topic_len"])[:n] == m["topic_len"]).all()
    assert (b["note_flags"].cpu().numpy()[:n] == m["note_flags"]).all()
    assert (u32(b["note_stream"])[:n] == m["note_stream"]).all(), (u32(b["note_stream"])[:n], m["note_stream"])
    if S:
        assert C.CurveContext.subs_results(b["results_out"])[:S] == m["results"]
    else:
        assert (b["results_out"].cpu().numpy() == S64).all()
    # the store and the view, as sets by destination; the view names exactly the live slots
    want = [sorted(d) for d in U.prefixes(st)]
    assert [sorted(d) for d in C.CurveContext.subs_store_view(d_store)] == want
    assert [sorted(d) for d in C.CurveContext.subs_store_view(d_store, view=True)] == want
    total = int(m["sub_idx"][-1])
    assert (u32(d_store["sub_idx"]) == m["sub_idx"]).all()
    off = d_store["sub_off"].cpu().numpy().view(np.uint64)
    cap, sb = st["cap"], st["slot_bytes"]
    assert all(int(off[int(m["sub_idx"][t]) + i]) == (t * cap + i) * sb for t in range(st["n_dst"])
               for i in range(int(m["sub_idx"][t + 1] - m["sub_idx"][t])))
    assert (d_store["sub_off"].cpu().numpy()[total:] == S64).all() and (d_store["sub_len"].cpu().numpy()[total:] == S32).all()
    # the clears: the former slots' entries, every other entry at its sentinel
    cl, cn = b["clear_len"].cpu().numpy().copy(), b["clear_note"].cpu().numpy().copy()
    for g, v in m["clear_len"].items():
        assert cl[g] == v and cn[g] == m["clear_note"][g], (g, cl[g], v, cn[g], m["clear_note"][g])
        cl[g], cn[g] = S32, S8
    assert (cl == S32).all() and (cn == S8).all()
    k = len(clear_dst)
    assert list(b["clear_cnt"].cpu().numpy()[:k]) == m["clear_cnt"] and (b["clear_cnt"].cpu().numpy()[k:] == S32).all()


def _run(torch, C, ctx, store, streams, MF, stream_dst, clear_dst=(), flags=0, frames=None, d_store=None):
    """One call on crafted inputs against the model.  store: the model's store
    before the call; d_store: its device copy (made when None).  Returns (the
    model's result, the device store) for the next call."""
    recv = U.craft(streams, MF, frames=frames)
    m = U.update(store, recv, MF, stream_dst, clear_dst, flags)
    d_store = d_store or _dev_store(torch, store)
    for k, v in (("sub_idx", S32), ("sub_off", S64), ("sub_len", S32)):
        d_store[k].fill_(v)
    b = _buffers(torch, recv, len(streams), MF, store, len(clear_dst))
    _call(ctx, d_store, b, stream_dst, MF, clear_dst, flags)
    _check(torch, C, d_store, b, m, len(streams), MF, clear_dst)
    return m, d_store


@pytest.fixture(scope="module")
def ctx(torch_cuda, C):
    c = C.CurveContext(0, 1)
    yield c
    c.close()


def _topic(i, n=6):
    return (b"%04d" % i + b"abcdefghijklmnop")[:n]


# 1 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("cap,held", [(65, 64), (65, 65), (130, 64), (130, 65), (130, 129)])
def test_slab_scans_cross_a_wave_step(torch_cuda, C, ctx, cap, held):
    """The hit in the last slot; a removal from the first slot, so that the last
    one moves into the hole and is found there; an append behind it."""
    mine = [_topic(i) for i in range(held)]
    store = U.store_of([[b"other"], mine, []], cap, 16)
    cmds = [SUB(mine[-1]), CAN(mine[0]), CCAN(mine[-1]), CSUB(b"fresh"), SUB(mine[0]), CAN(b"never")]
    m, _ = _run(torch_cuda, C, ctx, store, [cmds], len(cmds), [1])
    want = [U.DUPLICATE, U.REMOVED, U.REMOVED, U.ADDED, U.ADDED, U.NOT_FOUND]
    assert list(m["sub_status"]) == want
    assert int(m["store"]["cnt"][1]) == held


# 2 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_seventy_dependent_commands_in_one_stream(torch_cuda, C, ctx):
    """One stream of 70 commands (more than a wave step of slots) that depend on
    each other: subscribe, cancel and subscribe of one topic, a duplicate, a
    not-found, over three topics."""
    cmds = []
    for j in range(70):
        t = _topic(j // 5 % 3)
        cmds.append([SUB(t), CCAN(t), CSUB(t), SUB(t), CAN(_topic(9))][j % 5])
    m, _ = _run(torch_cuda, C, ctx, U.empty_store(2, 4, 8), [cmds], 70, [1])
    st = list(m["sub_status"])
    assert set(st) == {U.ADDED, U.REMOVED, U.DUPLICATE, U.NOT_FOUND} and set(st[64:]) == set(st)
    assert st[:5] == [U.ADDED, U.REMOVED, U.ADDED, U.DUPLICATE, U.NOT_FOUND] and st[15] == U.DUPLICATE


# 3 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_length_edges(torch_cuda, C, ctx):
    """slot_bytes 40: topics of 0 .. 41 bytes, pairs that differ only in the
    last byte and only in length, topics at odd and even offsets of plain."""
    rng = np.random.default_rng(5)
    lens = [0, 1, 7, 8, 9, 39, 40, 41]
    tops = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    tops[5] = tops[6][:39]  # 39 and 40 bytes: only the length differs
    flip = lambda t: t[:-1] + bytes([t[-1] ^ 1])
    cmds = [(SUB, CSUB)[i % 2](t) for i, t in enumerate(tops)]
    cmds += [(CSUB, SUB)[i % 2](flip(t)) for i, t in enumerate(tops) if t]
    cmds += [SUB(t) for t in tops]                                   # duplicates (and TOO_LONG again)
    cmds += [(CAN, CCAN)[i % 2](t) for i, t in enumerate(tops)]       # 41 bytes: NOT_FOUND
    cmds += [CAN(t) for t in tops[:3]]                               # gone: NOT_FOUND
    m, _ = _run(torch_cuda, C, ctx, U.empty_store(1, 32, 40), [cmds], len(cmds), [0])
    st = list(m["sub_status"])
    assert st[:8] == [U.ADDED] * 7 + [U.TOO_LONG] and st[8:15] == [U.ADDED] * 6 + [U.TOO_LONG]
    assert st[15:23] == [U.DUPLICATE] * 7 + [U.TOO_LONG] and st[23:31] == [U.REMOVED] * 7 + [U.NOT_FOUND]
    assert st[31:] == [U.NOT_FOUND] * 3
    assert sorted(U.prefixes(m["store"])[0]) == sorted(flip(t) for t in tops[1:7])
    assert {int(o) % 2 for o in m["topic_off"]} == {0, 1}
    assert m["results"][0]["rejected"] == 3


# 4 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_full_then_a_cancel_makes_room(torch_cuda, C, ctx):
    store = U.store_of([[b"a", b"b", b"c"]], 3, 8)
    m, _ = _run(torch_cuda, C, ctx, store, [[SUB(b"d"), CSUB(b"a"), CAN(b"b"), SUB(b"d")]], 4, [0])
    assert list(m["sub_status"]) == [U.FULL, U.DUPLICATE, U.REMOVED, U.ADDED]
    assert list(m["note_stream"]) == [U.NO_NOTE, U.NO_NOTE, 0, 0]


# 5 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, U.VERBOSE, U.VERBOSER])
def test_order_of_upstream_verdicts(torch_cuda, C, ctx, flags):
    """H is taken in (stream, slot) order: the lower stream cancels what only
    its destination holds while a higher stream subscribes to it, and the
    reverse assignment; three destinations share a topic across two calls."""
    store = U.store_of([[b"t"], [], []], 2, 8)
    m, _ = _run(torch_cuda, C, ctx, store, [[CAN(b"t")], [SUB(b"t")]], 1, [0, 1], flags=flags)
    assert m["notes"] == [(False, b"t"), (True, b"t")]
    m, _ = _run(torch_cuda, C, ctx, store, [[SUB(b"t")], [CAN(b"t")]], 1, [1, 0], flags=flags)
    assert m["notes"] == [(True, b"t")] * bool(flags) + [(False, b"t")] * (flags == U.VERBOSER)
    # persistence: the store of the first call is the second call's
    m1, d = _run(torch_cuda, C, ctx, U.empty_store(3, 2, 8), [[SUB(b"s")], [CSUB(b"s")], [SUB(b"s"), SUB(b"s")]], 2,
                 [2, 0, 1], flags=flags)
    assert [int(x) for x in m1["note_stream"]] == [0, U.NO_NOTE] + ([0, U.NO_NOTE, 0, 0] if flags else [U.NO_NOTE] * 4)
    m2, _ = _run(torch_cuda, C, ctx, m1["store"], [[CAN(b"s")], [CCAN(b"s")], [CAN(b"s")]], 1, [1, 2, 0], flags=flags,
                 d_store=d)
    assert [int(x) for x in m2["note_stream"]] == ([0, 0, 0] if flags == U.VERBOSER else [U.NO_NOTE, U.NO_NOTE, 0])
    assert U.prefixes(m2["store"]) == [[], [], []]


# 6 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_every_classification_branch(torch_cuda, C, ctx):
    """PING, an unknown command, commands shorter than a name, a data message,
    both forms of both commands, MORE; a frame with a non-zero status ends its
    stream; results[s].frames below max_frames; a stream without frames."""
    bad = 0x11000001
    s0 = [(U.COMMAND, b"\x04PING\x00\x05ctx", 0), (U.COMMAND, b"\x05HELLOxyz", 0), (U.COMMAND, b"", 0), (0, b"", 0),
          (U.COMMAND, b"\x09SUBSCRIB", 0), (U.COMMAND, b"\x09SUBSCRIBXab", 0), (U.COMMAND, b"\x06CANCE", 0),
          (U.COMMAND, b"\x40AB", 0), (U.COMMAND, b"\x01ab", 0), (0, b"\x02data", 0), (0, b"data", 0),
          SUB(b"ab"), CSUB(b"cd"), (U.MORE, b"\x01ef", 0), (U.COMMAND | U.MORE, b"\x09SUBSCRIBEgh", 0), CSUB(b""),
          CAN(b"ab"), CCAN(b"cd"), CCAN(b"")]
    s1 = [SUB(b"x"), (0, b"\x01y", bad), SUB(b"z")]          # the connection fails at its second frame
    s2 = [SUB(b"p"), SUB(b"q"), SUB(b"r")]                   # frames = 2: the third slot is not the call's
    s3 = [(0, b"\x01w", bad)]                                # fails at once
    MF = len(s0)
    m, _ = _run(torch_cuda, C, ctx, U.empty_store(5, 8, 8), [s0, s1, s2, [], s3], MF, [4, 3, 2, 1, 0],
                frames=[len(s0), 3, 2, 0, 1])
    assert list(m["sub_status"][:MF]) == [U.NONE] * 11 + [U.ADDED] * 5 + [U.REMOVED] * 3
    assert [r["seen"] for r in m["results"]] == [8, 1, 2, 0, 0]
    assert U.prefixes(m["store"]) == [[], [], [b"p", b"q"], [b"x"], [b"ef", b"gh"]]
    # max_frames above results[s].frames everywhere, and the padding slots' statuses non-zero
    assert (m["sub_status"][MF + 1:2 * MF] == U.NONE).all() and (m["note_flags"][2 * MF + 2:] == 0).all()


# 7 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, U.VERBOSER])
def test_clear(torch_cuda, C, ctx, flags):
    """Two destinations cleared: one held a topic alone, shared one with a live
    destination and one with the other cleared destination; a live stream
    cancels what a cleared destination shared with it.  The bytes stay; in the
    next call a new peer on the same index subscribes."""
    store = U.store_of([[b"alone", b"shared", b"both"], [b"shared"], [b"both", b"x", b"with3"], [b"with3"]], 4, 8)
    m, d = _run(torch_cuda, C, ctx, store, [[CAN(b"shared")], [SUB(b"alone")]], 1, [1, 3], clear_dst=[2, 0], flags=flags)
    assert m["clear_cnt"] == [3, 3]
    v = int(bool(flags))
    assert [m["clear_note"][g] for g in (8, 9, 10, 0, 1, 2)] == [v, 1, v, 1, v, 1]  # both: the second clear is the last
    assert [m["clear_len"][g] for g in (8, 9, 10, 0, 1, 2)] == [4, 1, 5, 5, 6, 4]
    assert list(m["note_stream"]) == [0, 0] and list(m["sub_status"]) == [U.REMOVED, U.ADDED]
    raw = d["bytes"].cpu().numpy()
    assert (raw[:4 * 8] == store["bytes"][:4 * 8]).all() and (raw[8 * 8:12 * 8] == store["bytes"][8 * 8:12 * 8]).all()
    assert U.prefixes(m["store"]) == [[], [], [], [b"with3", b"alone"]]
    m2, _ = _run(torch_cuda, C, ctx, m["store"], [[SUB(b"with3"), SUB(b"new")]], 2, [0], clear_dst=[1], flags=flags,
                 d_store=d)
    assert m2["clear_cnt"] == [0] and list(m2["sub_status"]) == [U.ADDED, U.ADDED]
    assert [int(x) for x in m2["note_stream"]] == [0 if flags else U.NO_NOTE, 0]


# 8 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_hostile_store(torch_cuda, C, ctx):
    """cnt above cap and a slot_len of 0xffffffff: the model's outcome under the clamps."""
    store = U.store_of([[b"aa", b"bb", b"cc"], [b"aa", b"bb"], [b"zz"]], 3, 8)
    store["cnt"][0] = 3 + 7
    store["cnt"][2] = 0xffffffff
    store["slot_len"][1] = 0xffffffff       # destination 0, slot 1: "bb" and six zero bytes
    store["slot_len"][2 * 3 + 2] = 0x80000000  # destination 2, slot 2 (live under the clamp): eight zero bytes
    cmds0 = [SUB(b"dd"), CAN(b"bb"), CAN(b"bb" + bytes(6)), CAN(b"aa"), SUB(b"dd")]
    m, _ = _run(torch_cuda, C, ctx, store, [cmds0, [CAN(bytes(8)), SUB(b"zz")]], 5, [0, 2], clear_dst=[1],
                frames=[5, 2])
    assert list(m["sub_status"][:5]) == [U.FULL, U.NOT_FOUND, U.REMOVED, U.REMOVED, U.ADDED]
    assert list(m["sub_status"][5:7]) == [U.REMOVED, U.DUPLICATE]
    assert [int(c) for c in m["store"]["cnt"]] == [2, 0, 2]


# 9 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_invalid_arguments_queue_nothing(torch_cuda, C, ctx):
    torch = torch_cuda
    store = U.store_of([[b"a"], [b"b"], []], 2, 8)
    streams = [[SUB(b"c")], [CAN(b"b")]]
    recv = U.craft(streams, 1)
    d = _dev_store(torch, store)
    b = _buffers(torch, recv, 2, 1, store, 1)
    many = np.arange(65536, dtype=np.uint32)

    def call(change=None, sd=(0, 1), cd=(2,), c=ctx._ctx, null_args=False, **fields):
        a, keep = C.CurveContext._subs_args(d, list(sd), 1, *[b[k] for k in INPUTS + OUTPUTS], list(cd),
                                            *[b[k] for k in CLEARS], 0)
        for k, v in fields.items():
            setattr(a, k, v)
        if change:
            change(a)
        return C._lib.zmqg_subs_update_multi(c, None if null_args else ctypes.byref(a), C._stream_handle(None))

    bad = [dict(c=None), dict(null_args=True), dict(size=232), dict(flags=1), dict(flags=8), dict(n_dst=8193), dict(cap=0),
           dict(slot_bytes=12), dict(slot_bytes=0), dict(slot_bytes=65544), dict(cap=2 ** 31), dict(n_dst=8192, cap=2 ** 18),
           dict(max_frames=2 ** 31), dict(n_streams=65536, max_frames=2 ** 15, stream_dst=many.ctypes.data),
           dict(n_streams=2 ** 31, stream_dst=many.ctypes.data),
           dict(sd=(0, 0)), dict(sd=(0, 3)), dict(sd=(0, 2)), dict(cd=(3,)), dict(sd=(0,), cd=(1, 1), n_streams=1),
           dict(bytes=d["bytes"].data_ptr() + 4)]
    bad += [{k: None} for k in ("cnt", "slot_len", "bytes", "sub_idx", "sub_off", "sub_len", "stream_dst", "clear_dst")]
    bad += [{k: None} for k in INPUTS + OUTPUTS + CLEARS]
    for kw in bad:
        assert call(**kw) == -22, kw
    torch.cuda.synchronize()
    for k, v in (("sub_idx", S32), ("sub_off", S64), ("sub_len", S32), ("sub_status", S32), ("topic_off", S64),
                 ("topic_len", S32), ("note_flags", S8), ("note_stream", S32), ("results_out", S64), ("clear_cnt", S32),
                 ("clear_len", S32), ("clear_note", S8)):
        assert ((d[k] if k in d else b[k]).cpu().numpy() == v).all(), k
    assert C.CurveContext.subs_store_view(d) == U.prefixes(store)
    # the same arguments unchanged are a valid call
    assert call() == 0
    _check(torch, C, d, b, U.update(store, recv, 1, [0, 1], [2]), 2, 1, [2])


# 10 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_nothing_to_apply_republishes_the_view(torch_cuda, C, ctx):
    """n_streams == 0 and n_clear == 0: only the view; max_frames == 0 with
    streams: results_out zeroed, the view; a store without destinations."""
    store = U.store_of([[b"a", b"bc"], [], [b"d"]], 2, 8)
    m, d = _run(torch_cuda, C, ctx, store, [], 7, [])
    assert list(m["sub_idx"]) == [0, 2, 2, 3]
    m, _ = _run(torch_cuda, C, ctx, store, [[], []], 0, [2, 0], d_store=d)
    assert m["results"] == [dict(seen=0, changed=0, notes=0, rejected=0)] * 2
    # with no input arrays at all
    for k in ("sub_idx", "sub_off", "sub_len"):
        d[k].fill_(-3)
    ctx.subs_update_multi(d)
    torch_cuda.cuda.synchronize()
    assert list(d["sub_idx"].cpu().numpy()) == [0, 2, 2, 3]
    m, _ = _run(torch_cuda, C, ctx, U.empty_store(0, 1, 8), [], 0, [])
    assert list(m["sub_idx"]) == [0]


# 11 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_many_destinations(torch_cuda, C, ctx):
    """300 destinations: the count of a topic's holders crosses the sixteen
    destinations a wave and the sixty-four a workgroup takes a step, the view's
    sums the 256 a step.  Seven holders of one topic cancel it in one call:
    only the last one notifies; a first subscriber of a fresh topic notifies,
    the second does not."""
    D, hot = 300, [0, 15, 16, 17, 255, 256, 299]
    held = [[b"hot", b"d%03d" % t] if t in hot else [b"d%03d" % t] for t in range(D)]
    store = U.store_of(held, 3, 8)
    dst = hot + [100, 200]
    streams = [[CAN(b"hot")] for _ in hot] + [[CSUB(b"new")], [SUB(b"new")]]
    m, d = _run(torch_cuda, C, ctx, store, streams, 1, dst)
    assert [int(x) for x in m["note_stream"]] == [U.NO_NOTE] * 6 + [0, 0, U.NO_NOTE]
    assert list(m["sub_status"]) == [U.REMOVED] * 7 + [U.ADDED] * 2
    assert int(m["sub_idx"][-1]) == D + 2
    # the other direction in the next call: the lowest stream holds it last
    m, _ = _run(torch_cuda, C, ctx, m["store"], [[SUB(b"hot")], [CAN(b"new")], [CAN(b"new")], [SUB(b"hot")]], 1,
                [299, 200, 100, 0], d_store=d)
    assert [int(x) for x in m["note_stream"]] == [0, U.NO_NOTE, 0, U.NO_NOTE]


# 12 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_end_to_end_through_the_existing_calls(torch_cuda, C):
    """Subscribers seal SUBSCRIBE / CANCEL messages (zmqg_encode_zmtp_multi, both
    downgrade_sub values); the broker decodes them (zmqg_decode_zmtp_multi),
    runs this call and feeds its per-slot outputs unchanged to
    zmqg_encode_zmtp_multi for the one upstream session; the upstream peer's
    decode yields exactly the model's notifications.  Then
    zmqg_forward_zmtp_sub_multi on test_gpu_forward_sub's core case gives the
    same outputs with the published view (its arrays read back as they are) as
    with the table built on the host from the model's final state."""
    from tests import test_gpu_forward_sub as TS
    torch, dev = torch_cuda, torch_cuda.device("cuda", 0)
    t = lambda a, dt, vt: _t(torch, a, dt, vt)
    rng = np.random.default_rng(11)
    precoms = [TS._rng_bytes(rng, 32) for _ in range(5)]
    down = [False, True, True, False]
    # the traffic: its final state is the core case's table, CORE_SUBS = [[A], [B, BB], [C], [A, C, Ax]]
    traffic = [[(1, b"A"), (1, b"Q"), (0, b"Q")], [(1, b"B"), (1, b"BB"), (1, b"B"), (0, b"nope")],
               [(1, b"A"), (1, b"C"), (0, b"A")], [(1, b"Ax"), (1, b"C"), (1, b"A")]]
    frames = [(s, C.SUBSCRIBE if on else C.CANCEL, tp) for j in range(4) for s, tr in enumerate(traffic)
              for on, tp in tr[j:j + 1]]  # arrival order: interleaved over the connections
    MF = 5
    subs = C.CurveContext(0, 4)
    for s in range(4):
        subs.session_set(s, precoms[s], C.CLIENT_PREFIX, C.SERVER_PREFIX, down[s], 1)
        subs.set_nonce(s, 3)
    broker = C.CurveContext(0, 5)
    for s in range(5):
        broker.session_set(s, precoms[s], C.SERVER_PREFIX, C.CLIENT_PREFIX, False, 2)
        broker.set_nonce(s, 7)
    upstream = C.CurveContext(0, 1)
    upstream.session_set(0, precoms[4], C.CLIENT_PREFIX, C.SERVER_PREFIX, False, 2)

    def encode(ctx, sids, frame_stream, flags, in_off, length, inp, n):
        out = torch.zeros(4096, dtype=torch.uint8, device=dev)
        foff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        res = torch.full((len(sids), 4), -1, dtype=torch.int64, device=dev)
        ctx.encode_zmtp_multi(t(sids, np.uint32, np.int32), frame_stream, None, flags, in_off, length, inp, out, foff, st,
                              res)
        return out, st, res

    def decode(ctx, sids, wire, res, max_frames):
        S = len(sids)
        r = res.cpu().numpy().view(np.uint64).reshape(-1, 4)
        n = S * max_frames
        o = dict(foff=torch.zeros(n, dtype=torch.int64, device=dev), flen=torch.zeros(n, dtype=torch.int32, device=dev),
                 poff=torch.zeros(n, dtype=torch.int64, device=dev), plain=torch.full((4096,), 0x77, dtype=torch.uint8, device=dev),
                 fl=torch.full((n,), 0xEE, dtype=torch.uint8, device=dev), st=torch.full((n,), -1, dtype=torch.int32, device=dev),
                 res=torch.full((S, 4), -1, dtype=torch.int64, device=dev))
        ctx.decode_zmtp_multi(t(sids, np.uint32, np.int32), t(r[:, 1], np.uint64, np.int64),
                              t(r[:, 2].astype(np.uint32), np.uint32, np.int32), wire, -1, max_frames, o["foff"], o["flen"],
                              o["poff"], o["plain"], o["fl"], o["st"], o["res"])
        return o

    topics = b"".join(tp for _, _, tp in frames)
    offs = np.cumsum([0] + [len(tp) for _, _, tp in frames])[:-1]
    wire, st, res = encode(subs, [0, 1, 2, 3], t([s for s, _, _ in frames], np.uint32, np.int32),
                           t([f for _, f, _ in frames], np.uint8, np.uint8), t(offs, np.uint64, np.int64),
                           t([len(tp) for _, _, tp in frames], np.uint32, np.int32), t(list(topics), np.uint8, np.uint8),
                           len(frames))
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    o = decode(broker, [0, 1, 2, 3], wire, res, MF)
    # this call, queued behind the decode; its outputs straight into the encode for the upstream session (4)
    store = U.empty_store(4, 4, 8)
    d_store = _dev_store(torch, store)
    recv0 = dict(results=[dict(frames=0, consumed=0, out_bytes=0, error=0)] * 4, f_len=np.zeros(4 * MF, np.uint32),
                 f_off=np.zeros(4 * MF, np.uint64), flags=np.zeros(4 * MF, np.uint8), status=np.zeros(4 * MF, np.int64),
                 out=np.zeros(1, np.uint8))
    b = _buffers(torch, recv0, 4, MF, store, 0)
    b.update(results=o["res"], frame_len=o["flen"], plain_off=o["poff"], flags_out=o["fl"], status_out=o["st"],
             plain=o["plain"])
    _call(broker, d_store, b, [0, 1, 2, 3], MF)
    up_wire, up_st, up_res = encode(broker, [4], b["note_stream"], b["note_flags"], b["topic_off"], b["topic_len"],
                                    o["plain"], 4 * MF)
    torch.cuda.synchronize()
    # the model, on what the decode has left (the decode itself is zmqg_decode_zmtp_multi's tests' business)
    recv = dict(results=broker.zmtp_results(o["res"]), f_off=o["poff"].cpu().numpy().view(np.uint64),
                f_len=o["flen"].cpu().numpy().view(np.uint32), flags=o["fl"].cpu().numpy(),
                status=o["st"].cpu().numpy().astype(np.int64) & 0xffffffff, out=o["plain"].cpu().numpy())
    assert [r["frames"] for r in recv["results"]] == [3, 4, 3, 3]
    pay = lambda k: recv["out"][int(recv["f_off"][k]):int(recv["f_off"][k]) + int(recv["f_len"][k]) - 33].tobytes()
    assert pay(0) == b"\x09SUBSCRIBEA" and recv["flags"][0] & U.COMMAND       # ZMTP 3.1 commands
    assert pay(MF) == b"\x01B" and not recv["flags"][MF] & U.COMMAND          # downgrade_sub: old-style messages
    assert pay(MF + 3) == b"\x00nope" and pay(3 * MF + 2) == b"\x09SUBSCRIBEA"
    m = U.update(store, recv, MF, [0, 1, 2, 3])
    _check(torch, C, d_store, b, m, 4, MF)
    assert [sorted(d) for d in U.prefixes(m["store"])] == [sorted(d) for d in TS.CORE_SUBS]
    assert len(m["notes"]) == 8 and (False, b"nope") in m["notes"]
    # upstream: one frame per note, in slot order; the peer decodes the model's notification commands
    ust = up_st.cpu().numpy().astype(np.int64) & 0xffffffff
    assert [int(x == 0) for x in ust] == [int(x == 0) for x in m["note_stream"]]
    assert all(x == C.ERR_SESSION for x in ust[m["note_stream"] != 0])
    u = decode(upstream, [0], up_wire, up_res, len(m["notes"]) + 1)
    torch.cuda.synchronize()
    ur = upstream.zmtp_results(u["res"])[0]
    assert ur["frames"] == len(m["notes"]) and ur["error"] == 0
    up_plain, up_off, up_len = u["plain"].cpu().numpy(), u["poff"].cpu().numpy(), u["flen"].cpu().numpy()
    got_notes = [up_plain[int(up_off[k]):int(up_off[k]) + int(up_len[k]) - 33].tobytes() for k in range(ur["frames"])]
    assert (u["st"].cpu().numpy()[:ur["frames"]] == 0).all() and all(f & U.COMMAND for f in u["fl"].cpu().numpy()[:ur["frames"]])
    assert got_notes == [(b"\x09SUBSCRIBE" if on else b"\x06CANCEL") + tp for on, tp in m["notes"]]
    for c in (subs, broker, upstream):
        c.close()
    # the data direction: the published view against the host-built table
    view = dict(idx=d_store["sub_idx"].cpu().numpy().view(np.uint32), off=d_store["sub_off"].cpu().numpy().view(np.uint64),
                len=d_store["sub_len"].cpu().numpy().view(np.uint32), raw=d_store["bytes"].cpu().numpy(),
                n_subs=4 * 4, bytes_len=4 * 4 * 8)
    c, fm = TS._core(), TS._model(TS._core(), U.prefixes(m["store"]))
    host = TS._forward_sub(torch, C, c, fm["N"], fm["cap"], fm["total"] + TS.PAD, TS._table(U.prefixes(m["store"])))
    mine = TS._forward_sub(torch, C, c, fm["N"], fm["cap"], fm["total"] + TS.PAD, view)
    TS._compare(mine, fm, c)
    assert fm["match"] == TS._core_model()["match"]
    for k in ("results", "peer", "send", "fwd", "pair_off", "pair_status", "dst_results", "match"):
        assert mine[k] == host[k], k
    for k in TS.TF.RECV_KEYS + ("out",):
        assert mine[k].shape == host[k].shape and (mine[k] == host[k]).all(), k
