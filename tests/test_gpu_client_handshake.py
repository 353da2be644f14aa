"""The client side of the CURVE handshake on the device, end to end:
zmqg_curve_client_hello_batch / _welcome_batch / _ready_batch
(include/zmqg_curve.h; reference crypto_box_keypair, produce_hello,
process_welcome, produce_initiate, process_ready, src/curve_client_tools.hpp,
src/curve_client.cpp:112-214) against the libsodium 1.0.18 transcripts of
tests/golden/box_vectors.json and the Python model
(tests/curve_client_model.py), and in a loopback against the server calls on
the same device, into zmqg_session_set_batch_ex and a MESSAGE in each
direction.

Every rejected input is an ordinary protocol rejection.  The model's results
for the shared handshakes are computed once per module."""
import ctypes
import errno
import functools
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import curve_client_model as CM
from tests import curve_handshake_model as M

pytestmark = pytest.mark.gpu

SENT = 0xA5
SERVER_SK = bytes(range(1, 33))
POOL_N = 130


@functools.lru_cache(maxsize=None)
def pool():
    """130 valid random handshakes (the model's view), each with the client
    model's state record, INITIATE and READY."""
    rng = np.random.default_rng(131)
    rb = lambda n: rng.integers(0, 256, n, dtype="uint8").tobytes()
    out = []
    for _ in range(POOL_N):
        hn = 1 + int(rng.integers(0, 3)) * (2 ** 31 + 5)
        hs = M.random_handshake(rng, SERVER_SK, hello_nonce=hn)
        hs["hello_nonce"] = hn
        st, hello, hs["cstate"] = CM.client_hello(hs["server_pk"], hs["cn_sk"], hn)
        assert st == 0 and hello == hs["hello"]
        hs["vouch_nonce"] = rb(16)
        st, hs["cinitiate"], precom = CM.client_welcome(hs["cstate"], hs["client_pk"], hs["client_sk"], hs["welcome"],
                                                        hs["vouch_nonce"], hn + 1, hs["meta"])
        assert st == 0 and precom == hs["precom"]
        hs["ready_meta"] = rb(int(rng.integers(0, 90)))
        hs["ready_nonce"] = 1 + int(rng.integers(0, 2)) * (2 ** 40 + 3)
        hs["ready"] = M.server_ready(precom, hs["ready_nonce"], hs["ready_meta"])
        out.append(hs)
    return out


@functools.lru_cache(maxsize=None)
def base_hs():
    hs = M.random_handshake(np.random.default_rng(2024), SERVER_SK, meta_len=40)
    hs["cstate"] = CM.client_state(hs)
    return hs


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to("cuda")


def _packed(torch, items):
    return _dev(torch, np.frombuffer(b"".join(items), np.uint8))


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


def _unchanged(pairs):
    for t, a in pairs:
        assert np.array_equal(t.cpu().numpy().view(np.uint8).ravel(), np.ascontiguousarray(a).view(np.uint8).ravel()), \
            "an input was written"


def dev_client_hello(torch, ctx, server_pks, cn_secrets, nonces):
    """(status, hellos, states) of one zmqg_curve_client_hello_batch call."""
    n = len(nonces)
    spk, cns = np.frombuffer(b"".join(server_pks), np.uint8), np.frombuffer(b"".join(cn_secrets), np.uint8)
    non = np.array(nonces, np.uint64)
    d_spk, d_cns, d_non = _dev(torch, spk), _dev(torch, cns), _dev(torch, non)
    state = torch.full((128 * n,), SENT, dtype=torch.uint8, device="cuda")
    hello = torch.full((200 * n,), SENT, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ctx.client_hello_batch(d_spk, d_cns, d_non, state, hello, st)
    torch.cuda.synchronize()
    _unchanged([(d_spk, spk), (d_cns, cns), (d_non, non)])
    h, s = hello.cpu().numpy().tobytes(), state.cpu().numpy().tobytes()
    return (st.cpu().numpy(), [h[200 * i:200 * i + 200] for i in range(n)],
            [s[128 * i:128 * i + 128] for i in range(n)])


def dev_client_welcome(torch, ctx, states, client_pks, client_sks, cmds, vouch_nonces, nonces, metas, rng, gap=13):
    """One zmqg_curve_client_welcome_batch call: dict of status, the INITIATE
    of each accepted item (None otherwise), precoms (bytes and the device
    tensor).  Every item has an output slot of 257 + len(meta) bytes; `out`
    outside the accepted items' slots must still hold the sentinel."""
    n = len(cmds)
    cbuf, coff, _ = place(cmds, rng, gap)
    mbuf, moff, _ = place(metas, rng, gap)
    obuf, ooff, _ = place([bytes(257 + len(m)) for m in metas], rng, gap)
    obuf[:] = SENT
    sta, cpk, csk = (np.frombuffer(b"".join(x), np.uint8) for x in (states, client_pks, client_sks))
    vn, non = np.frombuffer(b"".join(vouch_nonces), np.uint8), np.array(nonces, np.uint64)
    clen, mlen = np.array([len(c) for c in cmds], np.uint32), np.array([len(m) for m in metas], np.uint32)
    ins = [(_dev(torch, a), a) for a in (sta, cpk, csk, coff, clen, cbuf, vn, non, moff, mlen, mbuf, ooff)]
    d = [t for t, _ in ins]
    out = _dev(torch, obuf)
    pre = torch.full((32 * n,), SENT, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ctx.client_welcome_batch(*d, out, pre, st)
    torch.cuda.synchronize()
    _unchanged(ins)
    status = st.cpu().numpy()
    got = out.cpu().numpy()
    written = np.zeros(len(obuf), bool)
    initiates = []
    for i in range(n):
        if status[i] == 0:
            a, l = int(ooff[i]), 257 + len(metas[i])
            written[a:a + l] = True
            initiates.append(got[a:a + l].tobytes())
        else:
            initiates.append(None)
    assert (got[~written] == SENT).all(), "out was written outside the accepted items' ranges"
    p = pre.cpu().numpy().tobytes()
    return dict(status=status, initiate=initiates, precom=[p[32 * i:32 * i + 32] for i in range(n)], precom_dev=pre)


def dev_client_ready(torch, ctx, precoms, cmds, rng, gap=13):
    """One zmqg_curve_client_ready_batch call: dict of status, peer nonces,
    metadata lengths and the metadata of each accepted item; meta_out outside
    the accepted items' ranges must still hold the sentinel."""
    n = len(cmds)
    cbuf, coff, _ = place(cmds, rng, gap)
    mbuf, moff, _ = place([bytes(max(len(c) - 30, 0)) for c in cmds], rng, gap)
    mbuf[:] = SENT
    pk, clen = np.frombuffer(b"".join(precoms), np.uint8), np.array([len(c) for c in cmds], np.uint32)
    ins = [(_dev(torch, a), a) for a in (pk, coff, clen, cbuf, moff)]
    d_pk, d_coff, d_clen, d_cmd, d_moff = [t for t, _ in ins]
    meta = _dev(torch, mbuf)
    peer = torch.full((n,), -3, dtype=torch.int64, device="cuda")
    mlen = torch.full((n,), -3, dtype=torch.int32, device="cuda")
    st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ctx.client_ready_batch(d_pk, d_coff, d_clen, d_cmd, peer, d_moff, meta, mlen, st)
    torch.cuda.synchronize()
    _unchanged(ins)
    status = st.cpu().numpy()
    got = meta.cpu().numpy()
    written = np.zeros(len(mbuf), bool)
    metas = []
    for i in range(n):
        if status[i] == 0:
            a, l = int(moff[i]), len(cmds[i]) - 30
            written[a:a + l] = True
            metas.append(got[a:a + l].tobytes())
        else:
            metas.append(None)
    assert (got[~written] == SENT).all(), "meta_out was written outside the accepted items' ranges"
    return dict(status=status, peer=peer.cpu().numpy().view(np.uint64), peer_dev=peer,
                meta_len=mlen.cpu().numpy().view(np.uint32), meta=metas)


def check_welcome(got, want):
    """got: dev_client_welcome's dict; want: the model's tuples."""
    for i, (st, initiate, precom) in enumerate(want):
        assert int(got["status"][i]) == st, (i, hex(int(got["status"][i])), hex(st))
        assert got["initiate"][i] == initiate, i
        assert got["precom"][i] == precom, i


def check_ready(got, want):
    for i, (st, peer, meta) in enumerate(want):
        assert int(got["status"][i]) == st, (i, hex(int(got["status"][i])), hex(st))
        assert int(got["peer"][i]) == peer, i
        assert int(got["meta_len"][i]) == (len(meta) if st == 0 else 0), i
        assert got["meta"][i] == meta, i


def golden():
    """golden_transcripts() plus each transcript's client-side secrets."""
    here = os.path.dirname(os.path.abspath(__file__))
    vec = json.load(open(os.path.join(here, "golden", "box_vectors.json")))["items"]
    T = M.golden_transcripts()
    for j, t in enumerate(T):
        t["k1"] = bytes.fromhex(vec[6 * j]["key"])
        t["client_sk"] = bytes.fromhex(vec[6 * j + 3]["sk"])
        t["vouch_nonce"] = bytes.fromhex(vec[6 * j + 3]["nonce"])[8:]
        t["hello_nonce"] = int.from_bytes(t["hello"][112:120], "big")
    return T


def test_golden_transcripts(torch_cuda, C):
    """The six libsodium transcripts through the three calls, one batch of six
    each (six different server keys): HELLO, state, INITIATE, precom, READY's
    metadata and peer nonce byte-exact."""
    torch = torch_cuda
    T = golden()
    rng = np.random.default_rng(6)
    ctx = C.CurveContext(0, 1)
    st, hello, state = dev_client_hello(torch, ctx, [t["server_pk"] for t in T], [t["cn_sk"] for t in T],
                                        [t["hello_nonce"] for t in T])
    assert (st == 0).all()
    assert hello == [t["hello"] for t in T]
    assert state == [t["cn_pk"] + t["cn_sk"] + t["k1"] + t["server_pk"] for t in T]
    got = dev_client_welcome(torch, ctx, state, [t["client_pk"] for t in T], [t["client_sk"] for t in T],
                             [t["welcome"] for t in T], [t["vouch_nonce"] for t in T], [t["peer_nonce"] for t in T],
                             [t["meta"] for t in T], rng)
    check_welcome(got, [(0, t["initiate"], t["precom"]) for t in T])
    rdy = dev_client_ready(torch, ctx, got["precom"], [t["ready"] for t in T], rng)
    check_ready(rdy, [(0, t["ready_nonce"], t["ready_meta"]) for t in T])


def test_loopback_both_sides_on_the_device(torch_cuda, C):
    """n = 65 whole handshakes, both sides on the device: client HELLO ->
    server HELLO -> client WELCOME -> server INITIATE -> server READY -> client
    READY; then 2n sessions in one ctx from the calls' own outputs (clients:
    send nonce 3 and READY's peer nonce; servers: send nonce 2 and INITIATE's
    peer nonce) and a MESSAGE each way under device nonces."""
    import tests.test_gpu_handshake as SH
    torch = torch_cuda
    n = 65
    rng = np.random.default_rng(65)
    rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    server_pk = M.public(SERVER_SK)
    client_sk = [rb(32) for _ in range(n)]
    client_pk = [M.public(s) for s in client_sk]
    cmeta = [rb(int(rng.integers(0, 120))) for _ in range(n)]
    smeta = [rb(int(rng.integers(0, 120))) for _ in range(n)]
    ctx = C.CurveContext(0, 2 * n)

    st, hello, cstate = dev_client_hello(torch, ctx, [server_pk] * n, [rb(32) for _ in range(n)], [1] * n)
    assert (st == 0).all()
    st, welcome, sstate = SH.dev_hello(torch, ctx, SERVER_SK, hello, [rb(96) for _ in range(n)], rng)
    assert (st == 0).all()
    cw = dev_client_welcome(torch, ctx, cstate, client_pk, client_sk, welcome, [rb(16) for _ in range(n)], [2] * n,
                            cmeta, rng)
    assert (cw["status"] == 0).all()
    si = SH.dev_initiate(torch, ctx, sstate, cw["initiate"], rng)
    assert (si["status"] == 0).all()
    assert si["client_key"] == client_pk
    assert si["meta"] == cmeta
    assert si["precom"] == cw["precom"]
    assert [int(p) for p in si["peer"]] == [2] * n
    ready = SH.dev_ready(torch, ctx, si["precom"], [1] * n, smeta, rng)
    cr = dev_client_ready(torch, ctx, cw["precom"], ready, rng)
    assert (cr["status"] == 0).all()
    assert cr["meta"] == smeta
    assert [int(p) for p in cr["peer"]] == [1] * n

    csid, ssid = np.arange(n, dtype=np.uint32), np.arange(n, 2 * n, dtype=np.uint32)
    ctx.session_set_batch(csid, cw["precom_dev"], C.CLIENT_PREFIX, C.SERVER_PREFIX, None, cr["peer"],
                          send_nonce=np.full(n, 3, np.uint64))
    ctx.session_set_batch(ssid, si["precom_dev"], C.SERVER_PREFIX, C.CLIENT_PREFIX, None, si["peer"],
                          send_nonce=np.full(n, 2, np.uint64))
    payloads = [rb(1 + 7 * (j % 11)) for j in range(n)]
    lens = np.array([len(p) for p in payloads], np.uint32)
    inp = np.frombuffer(b"".join(payloads), np.uint8)
    in_off = (np.cumsum(lens) - lens).astype(np.uint64)
    wl = np.array([O.wire_size(0, 0, int(l)) for l in lens], np.uint32)
    w_off = (np.cumsum(wl) - wl).astype(np.uint64)
    d_flags, d_in_off, d_lens, d_inp = (_dev(torch, a) for a in (np.zeros(n, np.uint8), in_off, lens, inp))
    d_w_off, d_wl = _dev(torch, w_off), _dev(torch, wl)
    for send, recv, first in ((csid, ssid, 3), (ssid, csid, 2)):
        wire = torch.zeros(int(wl.sum()), dtype=torch.uint8, device="cuda")
        ctx.encode_batch(_dev(torch, send), None, d_flags, d_in_off, d_lens, d_inp, d_w_off, wire, nonce_auto=True)
        out = torch.zeros(len(inp), dtype=torch.uint8, device="cuda")
        fl = torch.zeros(n, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        ctx.decode_batch(_dev(torch, recv), d_w_off, d_wl, wire, d_in_off, out, fl, st)
        torch.cuda.synchronize()
        frames = wire.cpu().numpy()
        assert all(frames[int(o) + 8:int(o) + 16].tobytes() == M.be64(first) for o in w_off)
        assert (st.cpu().numpy() == 0).all()
        assert out.cpu().numpy().tobytes() == inp.tobytes()
        assert ctx.get_nonce(int(send[0])) == first + 1 and ctx.get_peer_nonce(int(recv[n - 1])) == first


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_batch_edges_against_model(torch_cuda, C, n):
    """Partial waves, a partial last workgroup and both waves' lanes past n:
    n random valid handshakes, the commands at random byte offsets with
    random gaps."""
    torch = torch_cuda
    P = pool()[:n]
    rng = np.random.default_rng(2000 + n)
    ctx = C.CurveContext(0, 1)
    st, hello, state = dev_client_hello(torch, ctx, [p["server_pk"] for p in P], [p["cn_sk"] for p in P],
                                        [p["hello_nonce"] for p in P])
    assert (st == 0).all()
    assert hello == [p["hello"] for p in P]
    assert state == [p["cstate"] for p in P]
    got = dev_client_welcome(torch, ctx, state, [p["client_pk"] for p in P], [p["client_sk"] for p in P],
                             [p["welcome"] for p in P], [p["vouch_nonce"] for p in P],
                             [p["hello_nonce"] + 1 for p in P], [p["meta"] for p in P], rng)
    check_welcome(got, [(0, p["cinitiate"], p["precom"]) for p in P])
    for p, ini in zip(P[:3], got["initiate"]):
        assert M.server_initiate(p["state"], ini)[0] == 0
    rdy = dev_client_ready(torch, ctx, got["precom"], [p["ready"] for p in P], rng)
    check_ready(rdy, [(0, p["ready_nonce"], p["ready_meta"]) for p in P])


META_SIZES = (0, 1, 31, 32, 33, 95, 96, 97, 600)


def test_initiate_sizes(torch_cuda, C):
    """Metadata of 0 .. 600 bytes in the INITIATE: the plaintext of 128 + m
    bytes ends just before, on and just after the 64-byte keystream window
    edges (m = 31, 32, 33 around stream byte 192; 95, 96, 97 around 256)."""
    torch = torch_cuda
    hs = base_hs()
    rng = np.random.default_rng(258)
    metas = [rng.integers(0, 256, m, dtype=np.uint8).tobytes() for m in META_SIZES]
    k = len(metas)
    vn = [bytes(range(j, j + 16)) for j in range(k)]
    want = [CM.client_welcome(hs["cstate"], hs["client_pk"], hs["client_sk"], hs["welcome"], vn[j], 2, metas[j])
            for j in range(k)]
    assert [len(w[1]) for w in want] == [257 + m for m in META_SIZES]
    got = dev_client_welcome(torch, C.CurveContext(0, 1), [hs["cstate"]] * k, [hs["client_pk"]] * k,
                             [hs["client_sk"]] * k, [hs["welcome"]] * k, vn, [2] * k, metas, rng)
    check_welcome(got, want)
    for ini, meta in zip(got["initiate"], metas):
        assert M.server_initiate(hs["state"], ini) == (0, hs["client_pk"], hs["precom"], 2, meta)


def test_ready_sizes(torch_cuda, C):
    """READY of 30 bytes (empty metadata), 29 bytes, and the same metadata
    lengths; nonces 1 and 2^64 - 1."""
    torch = torch_cuda
    rng = np.random.default_rng(31)
    keys, cmds = [], []
    for j, m in enumerate(META_SIZES):
        keys.append(rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
        cmds.append(M.server_ready(keys[-1], 1 if j % 2 else 2 ** 64 - 1,
                                   rng.integers(0, 256, m, dtype=np.uint8).tobytes()))
    assert len(cmds[0]) == 30
    keys += [keys[0], keys[2]]
    cmds += [cmds[0][:29], cmds[2][:29]]
    want = [CM.client_ready(k, c) for k, c in zip(keys, cmds)]
    assert [w[0] for w in want] == [0] * len(META_SIZES) + [CM.ERR_MALFORMED_READY] * 2
    got = dev_client_ready(torch, C.CurveContext(0, 1), keys, cmds, rng)
    check_ready(got, want)


def test_welcome_reject_rules(torch_cuda, C):
    """One batch mixes good items of the pool with one item per rule of
    welcome_cases (and inputs that break two rules at once): statuses as the
    model's, failed items' precom zero and nothing written to `out`,
    neighbours byte-exact.  S' = 0 and S' = 1 inside a valid WELCOME box are
    among the cases."""
    hs, P = base_hs(), pool()
    vn = bytes(range(100, 116))
    items = []
    for k, (name, cmd, code) in enumerate(CM.welcome_cases(hs)):
        items.append((name, hs["cstate"], hs["client_pk"], hs["client_sk"], cmd, vn, 2, hs["meta"], code))
        p = P[k]
        items.append(("good %d" % k, p["cstate"], p["client_pk"], p["client_sk"], p["welcome"], p["vouch_nonce"],
                      p["hello_nonce"] + 1, p["meta"], 0))
    want = [CM.client_welcome(*x[1:8]) for x in items]
    assert [w[0] for w in want] == [x[8] for x in items]
    got = dev_client_welcome(torch_cuda, C.CurveContext(0, 1), *[[x[j] for x in items] for j in range(1, 8)],
                             np.random.default_rng(13))
    check_welcome(got, want)
    small = 0
    for i, x in enumerate(items):
        if x[8] != 0:
            assert got["precom"][i] == bytes(32) and got["initiate"][i] is None, x[0]
        if x[0].startswith("S' = "):
            assert int(got["status"][i]) == CM.ERR_CRYPTOGRAPHIC, x[0]
            small += 1
    assert small == 2
    assert {x[8] for x in items} == {0, CM.ERR_UNEXPECTED_COMMAND, CM.ERR_CRYPTOGRAPHIC}


def test_ready_reject_rules(torch_cuda, C):
    """The same for READY: every rule of ready_cases between good items."""
    hs, P = base_hs(), pool()
    items = []
    for k, (name, cmd, code) in enumerate(CM.ready_cases(hs)):
        items.append((name, hs["precom"], cmd, code))
        items.append(("good %d" % k, P[k]["precom"], P[k]["ready"], 0))
    want = [CM.client_ready(x[1], x[2]) for x in items]
    assert [w[0] for w in want] == [x[3] for x in items]
    got = dev_client_ready(torch_cuda, C.CurveContext(0, 1), [x[1] for x in items], [x[2] for x in items],
                           np.random.default_rng(14))
    check_ready(got, want)
    for i, x in enumerate(items):
        if x[3] != 0:
            assert int(got["peer"][i]) == 0 and int(got["meta_len"][i]) == 0 and got["meta"][i] is None, x[0]
    assert {x[3] for x in items} == {0, CM.ERR_UNEXPECTED_COMMAND, CM.ERR_MALFORMED_READY, CM.ERR_CRYPTOGRAPHIC}


def test_small_order_server_keys_at_hello(torch_cuda, C):
    """server_pk = 0 and = 1 between good items: CRYPTOGRAPHIC, the HELLO slot
    and the state record zero."""
    P = pool()[:3]
    pks = [P[0]["server_pk"], bytes(32), P[1]["server_pk"], b"\x01" + bytes(31), P[2]["server_pk"]]
    sks = [P[0]["cn_sk"], P[0]["cn_sk"], P[1]["cn_sk"], P[1]["cn_sk"], P[2]["cn_sk"]]
    st, hello, state = dev_client_hello(torch_cuda, C.CurveContext(0, 1), pks, sks, [1] * 5)
    want = [CM.client_hello(pk, sk, 1) for pk, sk in zip(pks, sks)]
    assert [w[0] for w in want] == [0, CM.ERR_CRYPTOGRAPHIC, 0, CM.ERR_CRYPTOGRAPHIC, 0]
    assert [int(s) for s in st] == [w[0] for w in want]
    assert hello == [w[1] for w in want] and state == [w[2] for w in want]
    assert hello[1] == bytes(200) and state[3] == bytes(128)


def test_ladder_edges_through_hello(torch_cuda, C):
    """The (scalar, point) pairs of tests/golden/x25519_edge_vectors.json as
    (cn_secret, server_pk): both of HELLO's ladders at the field arithmetic's
    edges.  state[64:96] against the oracle's box_beforenm (and the fixture's
    libsodium value), state[0:32] against x25519(scalar, 9); the fixture's
    failing pairs are rejected."""
    here = os.path.dirname(os.path.abspath(__file__))
    V = json.load(open(os.path.join(here, "golden", "x25519_edge_vectors.json")))["vectors"]
    H = bytes.fromhex
    sks, pks = [H(v["scalar"]) for v in V], [H(v["point"]) for v in V]
    st, hello, state = dev_client_hello(torch_cuda, C.CurveContext(0, 1), pks, sks, [1] * len(V))
    fails = 0
    for i, v in enumerate(V):
        rc, k = O.box_beforenm(pks[i], sks[i])
        assert rc == v["brc"], i
        if rc != 0:
            assert int(st[i]) == CM.ERR_CRYPTOGRAPHIC and state[i] == bytes(128) and hello[i] == bytes(200), i
            fails += 1
            continue
        assert int(st[i]) == 0, i
        assert state[i][64:96] == k == H(v["k"]), (i, v["cls"])
        assert state[i][0:32] == hello[i][80:112] == M.public(sks[i]), (i, v["cls"])
        assert state[i][32:64] == sks[i] and state[i][96:128] == pks[i], i
    assert fails == sum(v["brc"] != 0 for v in V) > 0


def test_arguments(torch_cuda, C):
    """n = 0 returns 0 and writes nothing; each null pointer with n = 1, and
    n = 2^31, give -EINVAL."""
    torch = torch_cuda
    lib, ctx = C.lib(), C.CurveContext(0, 1)
    t = lambda nbytes: torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    bufs = {k: t(v) for k, v in dict(a32=32, b32=32, n8=8, state=128, hello=200, st=4, off=8, ln=4, cmd=168,
                                     vn=16, moff=8, mlen=4, meta=64, ooff=8, out=512, pre=32, peer=8).items()}
    B = {k: p(v) for k, v in bufs.items()}
    calls = [
        (lib.zmqg_curve_client_hello_batch, [B["a32"], B["b32"], B["n8"], B["state"], B["hello"], B["st"]]),
        (lib.zmqg_curve_client_welcome_batch, [B["state"], B["a32"], B["b32"], B["off"], B["ln"], B["cmd"], B["vn"],
                                               B["n8"], B["moff"], B["mlen"], B["meta"], B["ooff"], B["out"],
                                               B["pre"], B["st"]]),
        (lib.zmqg_curve_client_ready_batch, [B["pre"], B["off"], B["ln"], B["cmd"], B["peer"], B["moff"], B["meta"],
                                             B["mlen"], B["st"]]),
    ]
    for fn, args in calls:
        assert fn(ctx._ctx, 0, *args, None) == 0
        assert fn(ctx._ctx, 0, *([None] * len(args)), None) == 0
        assert fn(None, 1, *args, None) == -errno.EINVAL
        assert fn(ctx._ctx, 2 ** 31, *args, None) == -errno.EINVAL
        for j in range(len(args)):
            holed = list(args)
            holed[j] = None
            assert fn(ctx._ctx, 1, *holed, None) == -errno.EINVAL, (fn.__name__, j)
    torch.cuda.synchronize()
    for x in bufs.values():
        assert bool((x == SENT).all())
