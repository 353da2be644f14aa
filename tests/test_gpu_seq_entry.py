"""k_frames_seq's entry (variant ZMQG_FRAMES_G=0) against the oracle, byte for
byte: the kernel arguments, the call state every wave reads for itself, the
two groups of descriptor loads, window 0's words waited for behind its
keystream, and the look-back exchange beside them.

* grid edges: 1, 63, 64, 65, 255, 256, 257 and 1027 frames, payloads drawn
  from 0, 1, 30, 31, 32, 33, 95 and 1024 bytes under every plaintext header
  (1, 2, 8 and 11 bytes), every frame start modulo 16 and one batch with
  every start on a 64-byte boundary; encode with the caller's nonces and
  with the device's send counter, then decode; with and without
  ZMQG_OPT_STREAM_OUT;
* the call state across launches: three counter-driven encodes and their
  decodes back to back without a host synchronisation, one context used from
  two streams in turn, and the same sequence captured as a graph and replayed
  twice -- the nonces run on without gap or repeat and the decoder's peer
  nonce is the last one;
* decode header failures inside a wave -- a wrong command name, a wire length
  below 33, a wire length not above the first byte, a session out of range, a
  length above max_len -- each as the wave's first lane, its last lane, its
  longest and its shortest frame, beside good neighbours;
* the look-back: 600 frames with a replayed nonce in the third workgroup below
  the first workgroup's maximum, and one equal to the session's stored peer
  nonce."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_parity import dev, host
from tests.test_gpu_seq_startup import check_decode, check_encode, make
from tests.test_gpu_timed_path import _ctx

pytestmark = pytest.mark.gpu

PAYLOADS = [0, 1, 30, 31, 32, 33, 95, 1024]
HEADER_FLAGS = [0, 1, 2, 3, 12, 13, 16, 17]  # plain, SUBSCRIBE (12, 13), CANCEL (16, 17)
GRID_N = [1, 63, 64, 65, 255, 256, 257, 1027]


def _aligned(b, precoms_downgrade):
    """The batch with every payload and every wire frame on a 64-byte
    boundary (the oracle's wire made again at the new places)."""
    n = b["n"]
    slot = (int(b["wl"].max()) + 63) // 64 * 64
    off = np.arange(n, dtype=np.uint64) * slot
    b2 = dict(b)
    b2["in_off"], b2["out_off"], b2["dec_off"] = off, off, off
    b2["in_size"] = b2["w_size"] = b2["dec_size"] = n * slot + 16
    rng = np.random.default_rng(2100 + n)
    b2["inp"] = rng.integers(0, 256, b2["in_size"], dtype=np.uint8)
    sess = O.make_sessions(b["precoms"], downgrade_sub=precoms_downgrade)
    b2["wire"] = O.encode_batch(sess, b["sid"], b["nonce"], b["flags"], off, b["lens"], b2["inp"], off, b2["w_size"])
    return b2


@pytest.fixture(scope="module")
def grid_batches():
    out = {}
    for n in GRID_N:
        rng = np.random.default_rng(2000 + n)
        lens = np.array([PAYLOADS[k] for k in rng.integers(0, len(PAYLOADS), n)], np.uint32)
        lens[: min(n, len(PAYLOADS))] = PAYLOADS[: min(n, len(PAYLOADS))] if n > 1 else [32]
        flags = np.array([HEADER_FLAGS[k] for k in rng.integers(0, len(HEADER_FLAGS), n)], np.uint8)
        downgrade = n % 2 == 1 and n > 1  # (2-byte headers in the odd grids, 8 and 11 in the others and in n = 1)
        b = make(2001 + n, lens, flags=flags, downgrade=downgrade, in_mod=(np.arange(n) + n) % 16,
                 out_mod=(np.arange(n) * 5 + 3) % 16)
        out[n, False] = b
    out[257, True] = _aligned(out[257, False], True)
    return out


@pytest.mark.parametrize("stream_out", [False, True])
@pytest.mark.parametrize("n,aligned", [(n, False) for n in GRID_N] + [(257, True)])
def test_grid_edges(torch_cuda, C, grid_batches, n, aligned, stream_out):
    b = grid_batches[n, aligned]
    starts = {int(v) % 16 for v in b["in_off"]}
    assert (starts == {0}) if aligned else (n < 16 or starts == set(range(16)))
    check_encode(torch_cuda, C, b, stream_out=stream_out)
    check_encode(torch_cuda, C, b, nonce_auto=True, stream_out=stream_out)
    check_decode(torch_cuda, C, b, stream_out=stream_out)


# ------------------------------------------------------------------ the call state
def _calls_setup(torch, C, n, P, K, seed, stream_out):
    W = P + 33
    rng = np.random.default_rng(seed)
    precom = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    enc = _ctx(C, "0")
    enc.session_set(0, precom, O.CLIENT_PREFIX, O.SERVER_PREFIX)
    enc.set_nonce(0, 3)
    dec = _ctx(C, "0")
    dec.session_set(0, precom, O.SERVER_PREFIX, O.CLIENT_PREFIX, False, 2)
    s = dict(n=n, P=P, W=W, K=K, enc=enc, dec=dec, sess=O.make_sessions([precom]), stream_out=stream_out)
    s["inp_np"] = [rng.integers(0, 256, n * P, dtype=np.uint8) for _ in range(K)]
    s["flags_np"] = rng.integers(0, 4, n).astype(np.uint8)
    s["in_off_np"], s["out_off_np"] = np.arange(n, dtype=np.uint64) * P, np.arange(n, dtype=np.uint64) * W
    s["sid"], s["flags"] = dev(torch, np.zeros(n, np.uint32)), dev(torch, s["flags_np"])
    s["in_off"], s["out_off"] = dev(torch, s["in_off_np"]), dev(torch, s["out_off_np"])
    s["lens"], s["wl"] = dev(torch, np.full(n, P, np.uint32)), dev(torch, np.full(n, W, np.uint32))
    s["inp"] = [torch.from_numpy(a).to("cuda") for a in s["inp_np"]]
    s["wire"] = [torch.zeros(n * W, dtype=torch.uint8, device="cuda") for _ in range(K)]
    s["back"] = [torch.zeros(n * P, dtype=torch.uint8, device="cuda") for _ in range(K)]
    s["fl"] = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(K)]
    s["st"] = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(K)]
    return s


def _call(s, k, stream):
    s["enc"].encode_batch(s["sid"], None, s["flags"], s["in_off"], s["lens"], s["inp"][k], s["out_off"], s["wire"][k],
                          stream, max_len=s["P"], nonce_auto=True, stream_out=s["stream_out"])
    s["dec"].decode_batch(s["sid"], s["out_off"], s["wl"], s["wire"][k], s["in_off"], s["back"][k], s["fl"][k],
                          s["st"][k], stream, max_len=s["W"], stream_out=s["stream_out"])


def _check_calls(torch, s, first):
    """Call k of the sequence took the nonces first + k n .. first + (k + 1) n - 1."""
    torch.cuda.synchronize()
    n, K = s["n"], s["K"]
    for k in range(K):
        nonce = np.arange(first + k * n, first + (k + 1) * n, dtype=np.uint64)
        want = O.encode_batch(s["sess"], np.zeros(n, np.uint32), nonce, s["flags_np"], s["in_off_np"],
                              np.full(n, s["P"], np.uint32), s["inp_np"][k], s["out_off_np"], n * s["W"])
        assert np.array_equal(host(s["wire"][k], np.uint8), want), k
        assert int((s["st"][k] != 0).sum()) == 0, k
        assert torch.equal(s["back"][k], s["inp"][k]), k
        assert np.array_equal(host(s["fl"][k], np.uint8), s["flags_np"]), k
    assert s["enc"].get_nonce(0) == first + K * n
    assert s["dec"].get_peer_nonce(0) == first + K * n - 1


@pytest.mark.parametrize("stream_out", [False, True])
def test_three_calls_no_host_sync(torch_cuda, C, stream_out):
    torch = torch_cuda
    s = _calls_setup(torch, C, 300, 200, 3, 2201, stream_out)
    st = torch.cuda.current_stream()
    for k in range(3):
        _call(s, k, st)
    _check_calls(torch, s, 3)


@pytest.mark.parametrize("stream_out", [False, True])
def test_two_streams_in_turn(torch_cuda, C, stream_out):
    torch = torch_cuda
    s = _calls_setup(torch, C, 300, 200, 3, 2202, stream_out)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    a.wait_stream(torch.cuda.current_stream())
    order = [a, b, a]
    for k in range(3):
        if k:
            order[k].wait_stream(order[k - 1])
        with torch.cuda.stream(order[k]):
            _call(s, k, order[k])
    torch.cuda.current_stream().wait_stream(order[2])
    _check_calls(torch, s, 3)


@pytest.mark.parametrize("stream_out", [False, True])
def test_three_calls_graph_replayed_twice(torch_cuda, C, stream_out):
    torch = torch_cuda
    s = _calls_setup(torch, C, 300, 200, 3, 2203, stream_out)
    for k in range(3):  # (the workspaces are allocated outside the capture)
        _call(s, k, torch.cuda.current_stream())
    _check_calls(torch, s, 3)
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=cap):
        for k in range(3):
            _call(s, k, torch.cuda.current_stream())
    torch.cuda.synchronize()
    for r in range(2):
        for k in range(3):
            s["wire"][k].zero_()
            s["back"][k].zero_()
            s["st"][k].fill_(-1)
        graph.replay()
        _check_calls(torch, s, 3 + 3 * 300 * (r + 1))


# ------------------------------------------------------------------ header failures inside a wave
KINDS = ["name", "short", "first_byte", "sid", "max_len"]


@pytest.fixture(scope="module")
def wave_batch():
    """Four waves of 64 frames (one workgroup) and a fifth of 40: payloads of
    40 .. 150 bytes, in each wave one frame of 200 (its longest) and one of 34
    (its shortest), every start modulo 16."""
    n = 296
    rng = np.random.default_rng(2301)
    lens = rng.integers(40, 151, n).astype(np.uint32)
    longest, shortest = [], []
    for w in range(5):
        lo, hi = 64 * w, min(64 * w + 64, n)
        a, z = lo + 17 + w, lo + 30 - w
        lens[a], lens[z] = 200, 34
        longest.append(a)
        shortest.append(z)
        assert lens[lo:hi].argmax() + lo == a and lens[lo:hi].argmin() + lo == z
    b = make(2302, lens, flags=rng.integers(0, 4, n), in_mod=rng.integers(0, 16, n), out_mod=np.arange(n) % 16)
    return b, longest, shortest


@pytest.mark.parametrize("stream_out", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_header_failures_in_a_wave(torch_cuda, C, wave_batch, kind, stream_out):
    """Wave 0: the failure on its first lane; wave 1: on its last lane; wave
    2: on its longest frame; wave 3: on its shortest; wave 4 (partial): on its
    last frame.  (A frame above max_len is long wherever it stands, and one
    cut below 33 bytes short: the place is the frame's, not the length's.)"""
    b0, longest, shortest = wave_batch
    b = dict(b0)
    where = [0, 127, longest[2], shortest[3], b["n"] - 1]
    wire, wl, sid = b["wire"].copy(), b["wl"].copy(), b["sid"].copy()
    max_len = 0
    for i in where:
        a = int(b["out_off"][i])
        if kind == "name":
            wire[a + 1 + i % 7] ^= 0x20
        elif kind == "short":
            wl[i] = [32, 8, 20, 1, 0][where.index(i)]
        elif kind == "first_byte":
            wire[a] = 0xFF  # (every wire length here is below 255)
        elif kind == "sid":
            sid[i] = [1, 7, 0xffffffff, 2, 1][where.index(i)]
        else:
            max_len = 33 + 200
            wl[i] = max_len + 1 + where.index(i)  # (claims the next frames' bytes: window 0 is loaded from them, nothing behind it is moved or read)
    b["sid"], b["known"] = sid, sid < 1
    if kind == "max_len":  # (room behind the last frame for the length it claims)
        wire = np.concatenate([wire, np.zeros(256, np.uint8)])
    st = check_decode(torch_cuda, C, b, wire=wire, wl=wl, stream_out=stream_out, max_len=max_len)
    code = {"name": C.ERR_UNEXPECTED_COMMAND, "first_byte": C.ERR_MALFORMED_UNSPECIFIED, "sid": C.ERR_SESSION,
            "max_len": C.ERR_BOUND}
    for k, i in enumerate(where):
        if kind == "short":
            want = [C.ERR_MALFORMED_MESSAGE, C.ERR_MALFORMED_MESSAGE, C.ERR_MALFORMED_MESSAGE,
                    C.ERR_MALFORMED_UNSPECIFIED, C.ERR_MALFORMED_UNSPECIFIED][k]
        else:
            want = code[kind]
        assert st[i] == want, (kind, i, hex(int(st[i]) & 0xffffffff))
    assert (np.delete(st, where) == 0).all()  # good neighbours decode


# ------------------------------------------------------------------ the look-back behind window 0
@pytest.mark.parametrize("stream_out", [False, True])
def test_lookback_replays_across_workgroups(torch_cuda, C, stream_out):
    torch = torch_cuda
    n, P = 600, 100
    W = P + 33
    rng = np.random.default_rng(2401)
    precom = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    sid = np.zeros(n, np.uint32)
    in_off, out_off = np.arange(n, dtype=np.uint64) * P, np.arange(n, dtype=np.uint64) * W
    wl, lens = np.full(n, W, np.uint32), np.full(n, P, np.uint32)
    nonce = np.arange(3, 3 + n, dtype=np.uint64)
    nonce[530] = nonce[100]  # third workgroup, below the first workgroup's maximum
    nonce[7] = 2             # the session's stored peer nonce
    nonce[590] = 2
    flags = rng.integers(0, 4, n).astype(np.uint8)
    inp = rng.integers(0, 256, n * P, dtype=np.uint8)
    wire = O.encode_batch(O.make_sessions([precom]), sid, nonce, flags, in_off, lens, inp, out_off, n * W)
    dsess = O.make_sessions([precom], enc_prefix=O.SERVER_PREFIX, dec_prefix=O.CLIENT_PREFIX)
    peer = np.array([2], np.uint64)
    rpl, rfl, rst = O.decode_batch(dsess, peer, sid, out_off, wl, wire, in_off, n * P)
    assert [int(rst[k]) for k in (7, 530, 590)] == [C.ERR_INVALID_SEQUENCE] * 3 and (rst != 0).sum() == 3
    dec = _ctx(C, "0")
    dec.session_set(0, precom, O.SERVER_PREFIX, O.CLIENT_PREFIX, False, 2)
    back = torch.full((n * P,), 0xEE, dtype=torch.uint8, device="cuda")
    fl = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    dec.decode_batch(dev(torch, sid), dev(torch, out_off), dev(torch, wl), dev(torch, wire), dev(torch, in_off), back,
                     fl, st, stream_out=stream_out)
    torch.cuda.synchronize()
    gst = host(st, np.int32)
    assert np.array_equal(gst, rst[:n]), np.nonzero(gst != rst[:n])[0][:10]
    assert np.array_equal(host(fl, np.uint8), rfl[:n])
    assert np.array_equal(host(back, np.uint8), rpl[:n * P])
    assert dec.get_peer_nonce(0) == int(peer[0]) == 3 + n - 1
