"""k_frames_seq (variant ZMQG_FRAMES_G=0) against the oracle, byte for byte,
on the paths its lean step and its one-round look-back added:

* uniform and general steps: waves whose 64 frames all run the same windows
  (the specialised step), waves that one shorter or one longer frame makes
  leave the specialised steps early or late, and ragged lengths at unaligned
  offsets -- encode and decode, with and without ZMQG_OPT_STREAM_OUT;
* the look-back over self-validating records: one session, four workgroups
  (the last partial), replays and reorders across workgroups, a nonce jump,
  and three consecutive calls on one context, so that a record of an earlier
  call taken for this call's would pass a frame the oracle rejects;
* a captured graph of three encode+decode steps replayed twice (the call
  epoch of the records lives on the device).  The send counter ends at
  3 + 512 x (steps run); the peer counter holds the last accepted nonce, one
  below that (src/curve_mechanism_base.cpp:104), so the next nonce it
  accepts is 3 + 512 x (steps run)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_parity import dev, host
from tests.test_gpu_timed_path import _ctx

pytestmark = pytest.mark.gpu

N = 320  # two workgroups, five waves
RAGGED = [1, 31, 32, 33, 63, 64, 65, 127, 1024, 4575]


def _layout(case, rng):
    """(lens, in_off, out_off): payload lengths, payload offsets, wire offsets."""
    if case == "ragged":
        lens = np.array([RAGGED[i % len(RAGGED)] for i in rng.permutation(N)], np.uint32)
        gap_in = rng.integers(0, 7, N).astype(np.uint64)
        gap_out = rng.integers(0, 5, N).astype(np.uint64)
        in_off = np.concatenate([[0], np.cumsum(lens.astype(np.uint64) + gap_in)[:-1]]).astype(np.uint64) + 1
        out_off = np.concatenate([[0], np.cumsum(lens.astype(np.uint64) + 33 + gap_out)[:-1]]).astype(np.uint64) + 3
        return lens, in_off, out_off
    lens = np.full(N, 1024, np.uint32)
    if case == "one_shorter":  # one frame per wave ends early: 3, 9, 12, 1 and 16 windows
        lens[[5, 64 + 63, 128, 192 + 31, 256 + 17]] = [100, 500, 700, 0, 1000]
    elif case == "one_longer":  # one frame per wave goes on: up to 72 windows
        lens[[5, 64 + 63, 128, 192 + 31, 256 + 17]] = [1025, 1100, 2000, 4575, 1088]
    else:
        assert case == "uniform"
    slot = np.uint64(4672)  # 64-byte aligned, room for the longest wire frame
    in_off = np.arange(N, dtype=np.uint64) * slot
    out_off = np.arange(N, dtype=np.uint64) * slot
    return lens, in_off, out_off


def _covered(off, lens, size):
    m = np.zeros(size, bool)
    for a, L in zip(off, lens):
        m[int(a):int(a) + int(L)] = True
    return m


@pytest.fixture(scope="module")
def batches():
    """Per case: inputs and the oracle's wire, payloads, flags and statuses (computed once)."""
    out = {}
    for ci, case in enumerate(["uniform", "one_shorter", "one_longer", "ragged"]):
        rng = np.random.default_rng(900 + ci)
        precom = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        lens, in_off, out_off = _layout(case, rng)
        wl = (lens + 33).astype(np.uint32)
        in_size = int(in_off[-1] + lens[-1]) + 16
        w_size = int(out_off[-1] + wl[-1]) + 16
        inp = rng.integers(0, 256, in_size, dtype=np.uint8)
        sid = np.zeros(N, np.uint32)
        nonce = np.arange(3, 3 + N, dtype=np.uint64)
        flags = rng.integers(0, 4, N).astype(np.uint8)
        wire = O.encode_batch(O.make_sessions([precom]), sid, nonce, flags, in_off, lens, inp, out_off, w_size)
        bad = wire.copy()  # decode input: one MAC failure in a long frame's late window, when there is one
        k = int(np.argmax(lens))
        if lens[k] >= 64:
            bad[int(out_off[k]) + 33 + int(lens[k]) - 5] ^= 0x20
        dsess = O.make_sessions([precom], enc_prefix=O.SERVER_PREFIX, dec_prefix=O.CLIENT_PREFIX)
        peer = np.array([2], np.uint64)
        rpl, rfl, rst = O.decode_batch(dsess, peer, sid, out_off, wl, bad, in_off, in_size)
        out[case] = dict(precom=precom, lens=lens, in_off=in_off, out_off=out_off, wl=wl, inp=inp, sid=sid, nonce=nonce,
                         flags=flags, wire=wire, bad=bad, rpl=rpl, rfl=rfl, rst=rst, peer=int(peer[0]),
                         in_size=in_size, w_size=w_size, tampered=k if lens[k] >= 64 else None)
    return out


@pytest.mark.parametrize("stream_out", [False, True])
@pytest.mark.parametrize("case", ["uniform", "one_shorter", "one_longer", "ragged"])
def test_seq_encode_steps(torch_cuda, C, batches, case, stream_out):
    torch, b = torch_cuda, batches[case]
    enc = _ctx(C, "0")
    enc.session_set(0, b["precom"], O.CLIENT_PREFIX, O.SERVER_PREFIX)
    out = torch.full((b["w_size"],), 0xEE, dtype=torch.uint8, device="cuda")
    enc.encode_batch(dev(torch, b["sid"]), dev(torch, b["nonce"]), dev(torch, b["flags"]), dev(torch, b["in_off"]),
                     dev(torch, b["lens"]), dev(torch, b["inp"]), dev(torch, b["out_off"]), out, stream_out=stream_out)
    torch.cuda.synchronize()
    got = host(out, np.uint8)
    cov = _covered(b["out_off"], b["wl"], b["w_size"])
    diff = np.nonzero(got[cov] != b["wire"][cov])[0]
    assert diff.size == 0, f"{diff.size} wire bytes differ"
    assert (got[~cov] == 0xEE).all(), "bytes outside the frames written"


@pytest.mark.parametrize("stream_out", [False, True])
@pytest.mark.parametrize("case", ["uniform", "one_shorter", "one_longer", "ragged"])
def test_seq_decode_steps(torch_cuda, C, batches, case, stream_out):
    torch, b = torch_cuda, batches[case]
    dec = _ctx(C, "0")
    dec.session_set(0, b["precom"], O.SERVER_PREFIX, O.CLIENT_PREFIX, False, 2)
    back = torch.full((b["in_size"],), 0xEE, dtype=torch.uint8, device="cuda")
    fl = torch.full((N,), 0x55, dtype=torch.uint8, device="cuda")
    st = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    dec.decode_batch(dev(torch, b["sid"]), dev(torch, b["out_off"]), dev(torch, b["wl"]), dev(torch, b["bad"]),
                     dev(torch, b["in_off"]), back, fl, st, stream_out=stream_out)
    torch.cuda.synchronize()
    if b["tampered"] is not None:
        assert b["rst"][b["tampered"]] != 0
    assert np.array_equal(host(st, np.int32), b["rst"][:N])
    assert np.array_equal(host(fl, np.uint8), b["rfl"][:N])
    got = host(back, np.uint8)
    cov = _covered(b["in_off"], b["lens"], b["in_size"])
    diff = np.nonzero(got[cov] != b["rpl"][:b["in_size"]][cov])[0]
    assert diff.size == 0, f"{diff.size} payload bytes differ"
    assert (got[~cov] == 0xEE).all(), "bytes outside the payloads written"
    assert dec.get_peer_nonce(0) == b["peer"]


def test_seq_lookback_three_calls(torch_cuda, C):
    """n = 785 (workgroups of 256: four, the last of 17 frames), 100-byte
    payloads, one session, three decode calls on one context."""
    torch = torch_cuda
    n, P = 785, 100
    W = P + 33
    rng = np.random.default_rng(910)
    precom = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    sid = np.zeros(n, np.uint32)
    in_off = np.arange(n, dtype=np.uint64) * P
    out_off = np.arange(n, dtype=np.uint64) * W
    wl = np.full(n, W, np.uint32)
    lens = np.full(n, P, np.uint32)
    sess = O.make_sessions([precom])
    dsess = O.make_sessions([precom], enc_prefix=O.SERVER_PREFIX, dec_prefix=O.CLIENT_PREFIX)
    dec = _ctx(C, "0")
    dec.session_set(0, precom, O.SERVER_PREFIX, O.CLIENT_PREFIX, False, 2)
    peer = np.array([2], np.uint64)
    d_sid, d_in, d_wl, d_out = dev(torch, sid), dev(torch, out_off), dev(torch, wl), dev(torch, in_off)
    base = 3
    for call in range(3):
        nonce = np.arange(base, base + n, dtype=np.uint64)
        if call == 0:
            nonce[600] = nonce[50]                          # replay of a frame two workgroups earlier
            nonce[250], nonce[260] = nonce[260], nonce[250]  # reorder across the seam at 256: 251..260 fail
            nonce[400] = nonce[399]                         # replay of the frame just before
            nonce[770] = base + n + 100                     # jump: the frames after it fail
        elif call == 1:
            nonce[700] = nonce[10]                          # cross-workgroup replay (workgroup 2 <- 0)
            nonce[510], nonce[515] = nonce[515], nonce[510]  # reorder across the seam at 512
            nonce[300] = nonce[299]
            nonce[0] = base - 1                             # below the previous call's jump: rejected by the peer nonce
        else:
            nonce[780] = nonce[3]                           # last, partial workgroup <- workgroup 0
            nonce[520] = nonce[260]                         # workgroup 2 <- 1
            nonce[100] = base + 2 * n                       # early jump: most of the batch fails
            nonce[769:] = np.arange(base + 3 * n, base + 3 * n + n - 769, dtype=np.uint64)  # and recovers above it
        base = int(nonce.max()) + 1
        flags = rng.integers(0, 4, n).astype(np.uint8)
        inp = rng.integers(0, 256, n * P, dtype=np.uint8)
        wire = O.encode_batch(sess, sid, nonce, flags, in_off, lens, inp, out_off, n * W)
        rpl, rfl, rst = O.decode_batch(dsess, peer, sid, out_off, wl, wire, in_off, n * P)
        assert (rst != 0).sum() >= 4 and (rst == 0).sum() >= 20, call
        back = torch.full((n * P,), 0xEE, dtype=torch.uint8, device="cuda")
        fl = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        dec.decode_batch(d_sid, d_in, d_wl, dev(torch, wire), d_out, back, fl, st)
        torch.cuda.synchronize()
        gst = host(st, np.int32)
        assert np.array_equal(gst, rst[:n]), (call, np.nonzero(gst != rst[:n])[0][:10])
        assert np.array_equal(host(fl, np.uint8), rfl[:n]), call
        assert np.array_equal(host(back, np.uint8), rpl[:n * P]), call  # (failed frames zero-filled)
        assert dec.get_peer_nonce(0) == int(peer[0]), call


def test_seq_graph_replay(torch_cuda, C):
    torch = torch_cuda
    n, P, K = 512, 1024, 3
    W = P + 33
    rng = np.random.default_rng(911)
    precom = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    enc = _ctx(C, "0")
    enc.session_set(0, precom, O.CLIENT_PREFIX, O.SERVER_PREFIX)
    enc.set_nonce(0, 3)
    dec = _ctx(C, "0")
    dec.session_set(0, precom, O.SERVER_PREFIX, O.CLIENT_PREFIX, False, 2)
    payload = torch.from_numpy(rng.integers(0, 256, n * P, dtype=np.uint8)).to("cuda")
    flags_np = rng.integers(0, 4, n).astype(np.uint8)
    sid, flags = dev(torch, np.zeros(n, np.uint32)), dev(torch, flags_np)
    in_off, out_off = dev(torch, np.arange(n, dtype=np.uint64) * P), dev(torch, np.arange(n, dtype=np.uint64) * W)
    lens, wl = dev(torch, np.full(n, P, np.uint32)), dev(torch, np.full(n, W, np.uint32))
    wire = torch.zeros(n * W, dtype=torch.uint8, device="cuda")
    back = torch.zeros(n * P, dtype=torch.uint8, device="cuda")
    fl = torch.zeros(n, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")

    def step(s):
        enc.encode_batch(sid, None, flags, in_off, lens, payload, out_off, wire, s, max_len=P, nonce_auto=True)
        dec.decode_batch(sid, out_off, wl, wire, in_off, back, fl, st, s, max_len=W)

    def check(steps_run):
        torch.cuda.synchronize()
        assert int((st != 0).sum()) == 0
        assert torch.equal(back, payload)
        assert np.array_equal(host(fl, np.uint8), flags_np)
        assert enc.get_nonce(0) == 3 + n * steps_run
        assert dec.get_peer_nonce(0) + 1 == 3 + n * steps_run

    step(torch.cuda.current_stream())  # (the workspaces are allocated outside the capture)
    check(1)
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=cap):
        for _ in range(K):
            step(torch.cuda.current_stream())
    torch.cuda.synchronize()
    for r in range(2):
        back.zero_()
        st.fill_(-1)
        graph.replay()
        check(1 + K * (r + 1))
