"""The server side of the CURVE handshake on the device, end to end:
zmqg_curve_server_hello_batch / _initiate_batch / _ready_batch
(include/zmqg_curve.h; reference curve_server_t::process_hello,
produce_welcome, process_initiate, produce_ready, src/curve_server.cpp:117-458)
against the libsodium 1.0.18 transcripts of tests/golden/box_vectors.json and
the Python model (tests/curve_handshake_model.py), into
zmqg_session_set_batch_ex and a MESSAGE in each direction.

Every rejected input is an ordinary protocol rejection.  The model's results
for the shared handshakes are computed once per module."""
import ctypes
import errno
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import curve_handshake_model as M

pytestmark = pytest.mark.gpu

SENT = 0xA5
SERVER_SK = bytes(range(1, 33))
POOL_N = 130


@functools.lru_cache(maxsize=None)
def pool():
    """130 valid random handshakes with one server key (the model's view)."""
    rng = np.random.default_rng(130)
    return [M.random_handshake(rng, SERVER_SK, hello_nonce=1 + int(rng.integers(0, 3)) * (2 ** 31 + 5))
            for _ in range(POOL_N)]


@functools.lru_cache(maxsize=None)
def base_hs():
    return M.random_handshake(np.random.default_rng(2024), SERVER_SK, meta_len=40)


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to("cuda")


def place(chunks, rng, max_gap):
    """The chunks at random byte offsets with random gaps in a buffer filled
    with the sentinel; (buffer, offsets, mask of the bytes the chunks own)."""
    offs, pos = [], 0
    for c in chunks:
        pos += int(rng.integers(0, max_gap + 1)) if max_gap else 0
        offs.append(pos)
        pos += len(c)
    pos += 8
    buf = np.full(pos, SENT, np.uint8)
    own = np.zeros(pos, bool)
    for o, c in zip(offs, chunks):
        buf[o:o + len(c)] = np.frombuffer(bytes(c), np.uint8)
        own[o:o + len(c)] = True
    return buf, np.array(offs, np.uint64), own


def dev_hello(torch, ctx, server_sk, cmds, randoms, rng, gap=13):
    """(status, welcomes, states) of one zmqg_curve_server_hello_batch call."""
    n = len(cmds)
    buf, off, _ = place(cmds, rng, gap)
    cmd = _dev(torch, buf)
    state = torch.full((128 * n,), SENT, dtype=torch.uint8, device="cuda")
    wel = torch.full((168 * n,), SENT, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ctx.server_hello_batch(_dev(torch, np.frombuffer(server_sk, np.uint8)), _dev(torch, off),
                           _dev(torch, np.array([len(c) for c in cmds], np.uint32)), cmd,
                           _dev(torch, np.frombuffer(b"".join(randoms), np.uint8)), state, wel, st)
    torch.cuda.synchronize()
    assert np.array_equal(cmd.cpu().numpy(), buf), "the command buffer was written"
    w, s = wel.cpu().numpy().tobytes(), state.cpu().numpy().tobytes()
    return (st.cpu().numpy(), [w[168 * i:168 * i + 168] for i in range(n)],
            [s[128 * i:128 * i + 128] for i in range(n)])


def dev_initiate(torch, ctx, states, cmds, rng, gap=13):
    """One zmqg_curve_server_initiate_batch call: dict of status, client keys,
    precoms (bytes and the device tensor), peer nonces, metadata lengths and
    the metadata of each item; meta_out outside the accepted items' ranges
    must still hold the sentinel (every item has a slot of len - 257 bytes)."""
    n = len(cmds)
    buf, off, _ = place(cmds, rng, gap)
    slots = [bytes(max(len(c) - 257, 0)) for c in cmds]
    mbuf, moff, _ = place(slots, rng, gap)
    mbuf[:] = SENT
    cmd = _dev(torch, buf)
    meta = _dev(torch, mbuf)
    ck = torch.full((32 * n,), SENT, dtype=torch.uint8, device="cuda")
    pre = torch.full((32 * n,), SENT, dtype=torch.uint8, device="cuda")
    peer = torch.full((n,), -3, dtype=torch.int64, device="cuda")
    mlen = torch.full((n,), -3, dtype=torch.int32, device="cuda")
    st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ctx.server_initiate_batch(_dev(torch, np.frombuffer(b"".join(states), np.uint8)), _dev(torch, off),
                              _dev(torch, np.array([len(c) for c in cmds], np.uint32)), cmd, ck, pre, peer,
                              _dev(torch, moff), meta, mlen, st)
    torch.cuda.synchronize()
    assert np.array_equal(cmd.cpu().numpy(), buf), "the command buffer was written"
    status = st.cpu().numpy()
    got = meta.cpu().numpy()
    written = np.zeros(len(mbuf), bool)
    metas = []
    for i in range(n):
        if status[i] == 0:
            a, l = int(moff[i]), len(cmds[i]) - 257
            written[a:a + l] = True
            metas.append(got[a:a + l].tobytes())
        else:
            metas.append(None)
    assert (got[~written] == SENT).all(), "meta_out was written outside the accepted items' ranges"
    k, p = ck.cpu().numpy().tobytes(), pre.cpu().numpy().tobytes()
    return dict(status=status, client_key=[k[32 * i:32 * i + 32] for i in range(n)],
                precom=[p[32 * i:32 * i + 32] for i in range(n)], precom_dev=pre,
                peer=peer.cpu().numpy().view(np.uint64), meta_len=mlen.cpu().numpy().view(np.uint32), meta=metas)


def dev_ready(torch, ctx, precoms, nonces, metas, rng, gap=13):
    n = len(metas)
    mbuf, moff, _ = place(metas, rng, gap)
    obuf, ooff, own = place([bytes(30 + len(m)) for m in metas], rng, gap)
    obuf[:] = SENT
    out = _dev(torch, obuf)
    ctx.server_ready_batch(_dev(torch, np.frombuffer(b"".join(precoms), np.uint8)),
                           _dev(torch, np.array(nonces, np.uint64)), _dev(torch, moff),
                           _dev(torch, np.array([len(m) for m in metas], np.uint32)), _dev(torch, mbuf),
                           _dev(torch, ooff), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[~own] == SENT).all(), "READY wrote outside its commands"
    return [got[int(a):int(a) + 30 + len(m)].tobytes() for a, m in zip(ooff, metas)]


def check_initiate(got, want):
    """got: dev_initiate's dict; want: the model's tuples, item by item."""
    for i, (st, c, precom, peer, meta) in enumerate(want):
        assert int(got["status"][i]) == st, (i, hex(int(got["status"][i])), hex(st))
        assert got["client_key"][i] == c, i
        assert got["precom"][i] == precom, i
        assert int(got["peer"][i]) == peer, i
        assert int(got["meta_len"][i]) == (len(meta) if st == 0 else 0), i
        assert got["meta"][i] == meta, i


def test_golden_transcripts_into_sessions_and_messages(torch_cuda, C):
    """The six libsodium transcripts: WELCOME, state, C, precom, peer nonce,
    metadata and READY byte-exact; then the sessions installed from
    precom_out / peer_nonce_out with send nonce 2 carry a MESSAGE each way.

    The transcripts have six different server keys and the HELLO call takes
    one per batch, so the HELLOs are six calls of one item; INITIATE, READY and
    the session install are one batch of 6.  The client's MESSAGE uses the
    nonce after its INITIATE's (3 for the first transcript, whose HELLO used
    1; the later transcripts start higher), as a curve_client_t would."""
    torch = torch_cuda
    T = M.golden_transcripts()
    rng = np.random.default_rng(6)
    ctx = C.CurveContext(0, 6)
    states = []
    for t in T:
        st, wel, sta = dev_hello(torch, ctx, t["server_sk"], [t["hello"]], [t["random"]], rng)
        assert int(st[0]) == 0
        assert wel[0] == t["welcome"]
        assert sta[0] == t["state"]
        states.append(sta[0])
    got = dev_initiate(torch, ctx, states, [t["initiate"] for t in T], rng)
    check_initiate(got, [(0, t["client_pk"], t["precom"], t["peer_nonce"], t["meta"]) for t in T])
    ready = dev_ready(torch, ctx, got["precom"], [t["ready_nonce"] for t in T], [t["ready_meta"] for t in T], rng)
    assert ready == [t["ready"] for t in T]

    sid = np.arange(6, dtype=np.uint32)
    ctx.session_set_batch(sid, got["precom_dev"], C.SERVER_PREFIX, C.CLIENT_PREFIX, None, got["peer"],
                          send_nonce=np.full(6, 2, np.uint64))
    # client -> server: the oracle encodes as the client, the device decodes
    payloads = [rng.integers(0, 256, 20 + 9 * j, dtype=np.uint8).tobytes() for j in range(6)]
    lens = np.array([len(p) for p in payloads], np.uint32)
    inp = np.frombuffer(b"".join(payloads), np.uint8)
    in_off = (np.cumsum(lens) - lens).astype(np.uint64)
    flags = np.zeros(6, np.uint8)
    wl = np.array([O.wire_size(0, 0, int(l)) for l in lens], np.uint32)
    w_off = (np.cumsum(wl) - wl).astype(np.uint64)
    nonce = (got["peer"] + np.uint64(1)).astype(np.uint64)
    assert int(nonce[0]) == 3
    client = O.make_sessions([t["precom"] for t in T], O.CLIENT_PREFIX, O.SERVER_PREFIX)
    wire = O.encode_batch(client, sid, nonce, flags, in_off, lens, inp, w_off, int(wl.sum()))
    out = torch.zeros(len(inp), dtype=torch.uint8, device="cuda")
    fl = torch.zeros(6, dtype=torch.uint8, device="cuda")
    st = torch.full((6,), 7, dtype=torch.int32, device="cuda")
    ctx.decode_batch(_dev(torch, sid), _dev(torch, w_off), _dev(torch, wl), _dev(torch, wire), _dev(torch, in_off),
                     out, fl, st)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    assert out.cpu().numpy().tobytes() == inp.tobytes()
    # server -> client: the device encodes with its send counters (2), the oracle opens
    back = torch.zeros(int(wl.sum()), dtype=torch.uint8, device="cuda")
    ctx.encode_batch(_dev(torch, sid), None, _dev(torch, flags), _dev(torch, in_off), _dev(torch, lens),
                     _dev(torch, inp), _dev(torch, w_off), back, nonce_auto=True)
    torch.cuda.synchronize()
    frames = back.cpu().numpy()
    for j in range(6):
        assert frames[int(w_off[j]) + 8:int(w_off[j]) + 16].tobytes() == M.be64(2)
    peer = np.ones(6, np.uint64)
    o_out, o_fl, o_st = O.decode_batch(client, peer, sid, w_off, wl, frames, in_off, len(inp))
    assert (o_st == 0).all() and o_out.tobytes() == inp.tobytes()
    assert [ctx.get_nonce(j) for j in range(6)] == [3] * 6


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_batch_edges_against_model(torch_cuda, C, n):
    """Partial last workgroups and partial waves: n random valid handshakes,
    the commands at random byte offsets with random gaps."""
    torch = torch_cuda
    P = pool()[:n]
    rng = np.random.default_rng(1000 + n)
    ctx = C.CurveContext(0, 1)
    st, wel, sta = dev_hello(torch, ctx, SERVER_SK, [p["hello"] for p in P], [p["random"] for p in P], rng)
    assert (st == 0).all()
    assert wel == [p["welcome"] for p in P]
    assert sta == [p["state"] for p in P]
    got = dev_initiate(torch, ctx, sta, [p["initiate"] for p in P], rng)
    check_initiate(got, [(0, p["client_pk"], p["precom"], p["peer_nonce"], p["meta"]) for p in P])
    nonces = [1 + (i % 3) for i in range(n)]
    ready = dev_ready(torch, ctx, got["precom"], nonces, [p["meta"] for p in P], rng)
    assert ready == [M.server_ready(p["precom"], k, p["meta"]) for p, k in zip(P, nonces)]
    for p, r in zip(P[:3], ready):
        assert M.client_open_ready(r, p["precom"]) == p["meta"]


def test_initiate_sizes(torch_cuda, C):
    """Metadata of 0 .. 600 bytes: the plaintext of 128 + m bytes ends just
    before, on and just after the 64-byte keystream window edges (m = 31, 32,
    33 around stream byte 192; 95, 96, 97 around 256); 257 bytes exactly, and
    256 bytes -> MALFORMED_INITIATE."""
    torch = torch_cuda
    hs = base_hs()
    rng = np.random.default_rng(257)
    cmds = []
    for m in (0, 1, 31, 32, 33, 95, 96, 97, 600):
        meta = rng.integers(0, 256, m, dtype=np.uint8).tobytes()
        cmds.append(M.client_initiate(hs["client_pk"], hs["client_sk"], hs["server_pk"], hs["cn_sk"], hs["sn_pk"],
                                      hs["cookie"], 2, meta, bytes(range(16))))
    assert len(cmds[0]) == 257
    cmds.append(cmds[0][:256])
    cmds.append(cmds[5][:256])
    want = [M.server_initiate(hs["state"], c) for c in cmds]
    assert [w[0] for w in want] == [0] * 9 + [M.ERR_MALFORMED_INITIATE] * 2
    got = dev_initiate(torch, C.CurveContext(0, 1), [hs["state"]] * len(cmds), cmds, rng)
    check_initiate(got, want)


@functools.lru_cache(maxsize=None)
def reject_batches():
    """The reject cases of both commands, each between good items of the pool."""
    hs, P = base_hs(), pool()
    hello, k = [], 0
    for name, cmd, code in M.hello_cases(hs):
        hello.append((name, cmd, hs["random"], code))
        hello.append(("good %d" % k, P[k]["hello"], P[k]["random"], 0))
        k += 1
    ini, k = [], 0
    for name, cmd, code in M.initiate_cases(hs, SERVER_SK):
        ini.append((name, cmd, hs["state"], code))
        ini.append(("good %d" % k, P[k]["initiate"], P[k]["state"], 0))
        k += 1
    return hello, ini


_DEVICE = {}


def device_rejects(torch, C):
    """The two reject batches run once on the device."""
    if not _DEVICE:
        hello, ini = reject_batches()
        ctx = C.CurveContext(0, 1)
        _DEVICE["hello"] = dev_hello(torch, ctx, SERVER_SK, [h[1] for h in hello], [h[2] for h in hello],
                                     np.random.default_rng(11))
        _DEVICE["initiate"] = dev_initiate(torch, ctx, [x[2] for x in ini], [x[1] for x in ini],
                                           np.random.default_rng(12))
    return _DEVICE["hello"], _DEVICE["initiate"]


def test_hello_reject_rules(torch_cuda, C):
    """One batch mixes good items with one item per rule (and inputs that
    break two rules at once): statuses as the model's, failed items zero,
    neighbours byte-exact."""
    hello, _ = reject_batches()
    (st, wel, sta), _ = device_rejects(torch_cuda, C)
    for i, (name, cmd, random96, code) in enumerate(hello):
        w_st, w_wel, w_sta = M.server_hello(SERVER_SK, cmd, random96)
        assert w_st == code, name
        assert int(st[i]) == w_st, (name, hex(int(st[i])), hex(w_st))
        assert wel[i] == w_wel, name
        assert sta[i] == w_sta, name
        if code != 0:
            assert wel[i] == bytes(168) and sta[i] == bytes(128), name
    assert {h[3] for h in hello} == {0, M.ERR_MALFORMED_UNSPECIFIED, M.ERR_UNEXPECTED_COMMAND,
                                     M.ERR_MALFORMED_HELLO, M.ERR_CRYPTOGRAPHIC}


def test_initiate_reject_rules(torch_cuda, C):
    """The same for INITIATE: a flipped bit in the cookie, the tag, the
    ciphertext (vouch region and metadata) and the vouch, a valid cookie box
    with foreign content, a valid vouch for a foreign C' (KEY_EXCHANGE)."""
    _, ini = reject_batches()
    _, got = device_rejects(torch_cuda, C)
    want = [M.server_initiate(state, cmd) for _, cmd, state, _ in ini]
    assert [w[0] for w in want] == [x[3] for x in ini]
    check_initiate(got, want)
    for i, x in enumerate(ini):
        if x[3] != 0:
            assert got["client_key"][i] == bytes(32) and got["precom"][i] == bytes(32), x[0]
            assert int(got["peer"][i]) == 0 and int(got["meta_len"][i]) == 0 and got["meta"][i] is None, x[0]
    assert {x[3] for x in ini} == {0, M.ERR_MALFORMED_UNSPECIFIED, M.ERR_UNEXPECTED_COMMAND,
                                   M.ERR_MALFORMED_INITIATE, M.ERR_CRYPTOGRAPHIC, M.ERR_KEY_EXCHANGE}


def test_small_order_points(torch_cuda, C):
    """C' = 0 and C' = 1 in a HELLO, C = 0 inside an otherwise valid INITIATE:
    CRYPTOGRAPHIC, the outputs zero."""
    hello, ini = reject_batches()
    (st, wel, sta), got = device_rejects(torch_cuda, C)
    seen = 0
    for i, h in enumerate(hello):
        if h[0] in ("C' = 0", "C' = 1"):
            assert int(st[i]) == M.ERR_CRYPTOGRAPHIC and wel[i] == bytes(168) and sta[i] == bytes(128)
            seen += 1
    for i, x in enumerate(ini):
        if x[0] == "C = 0":
            assert int(got["status"][i]) == M.ERR_CRYPTOGRAPHIC
            assert got["client_key"][i] == bytes(32) and got["precom"][i] == bytes(32) and got["meta"][i] is None
            seen += 1
    assert seen == 3


def test_ready_sizes_and_nonces(torch_cuda, C):
    torch = torch_cuda
    rng = np.random.default_rng(30)
    metas, nonces, keys = [], [], []
    for m in (0, 1, 31, 32, 33, 97):
        for nonce in (1, 2 ** 64 - 1):
            metas.append(rng.integers(0, 256, m, dtype=np.uint8).tobytes())
            nonces.append(nonce)
            keys.append(rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
    got = dev_ready(torch, C.CurveContext(0, 1), keys, nonces, metas, rng)
    assert got == [M.server_ready(k, n, m) for k, n, m in zip(keys, nonces, metas)]


def test_arguments(torch_cuda, C):
    """n = 0 returns 0 and writes nothing; a null status_out (READY: a null
    out) with n = 1 gives -EINVAL."""
    torch = torch_cuda
    lib, ctx = C.lib(), C.CurveContext(0, 1)
    hs = base_hs()
    t = lambda nbytes: torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")
    cmd = _dev(torch, np.frombuffer(hs["hello"], np.uint8))
    sk, rnd, state, wel, st = t(32), t(96), t(128), t(168), t(4)
    off, ln, key, pre, peer, moff, meta, mlen = t(8), t(4), t(32), t(32), t(8), t(8), t(64), t(4)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    hello = lambda n, status: lib.zmqg_curve_server_hello_batch(ctx._ctx, n, p(sk), p(off), p(ln), p(cmd), p(rnd),
                                                                p(state), p(wel), status, None)
    ini = lambda n, status: lib.zmqg_curve_server_initiate_batch(ctx._ctx, n, p(state), p(off), p(ln), p(cmd),
                                                                 p(key), p(pre), p(peer), p(moff), p(meta), p(mlen),
                                                                 status, None)
    ready = lambda n, out: lib.zmqg_curve_server_ready_batch(ctx._ctx, n, p(pre), p(peer), p(moff), p(ln), p(meta),
                                                             p(off), out, None)
    assert hello(0, p(st)) == 0 and ini(0, p(st)) == 0 and ready(0, p(meta)) == 0
    assert hello(0, None) == 0 and ini(0, None) == 0 and ready(0, None) == 0
    assert hello(1, None) == -errno.EINVAL
    assert ini(1, None) == -errno.EINVAL
    assert ready(1, None) == -errno.EINVAL
    assert hello(2 ** 31, p(st)) == -errno.EINVAL
    torch.cuda.synchronize()
    for x in (sk, rnd, state, wel, st, off, ln, key, pre, peer, moff, meta, mlen):
        assert bool((x == SENT).all())
