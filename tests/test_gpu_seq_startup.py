"""k_frames_seq (variant ZMQG_FRAMES_G=0) against the oracle, byte for byte, on
what its start-up (descriptors, session key, window 0) and its first steps
decide: 320 frames unless said otherwise (two workgroups, the last wave
partial), encode and decode, no byte written outside the frames, the send and
peer counters the oracle's.

* frames of unknown sessions (sid >= max_sessions) beside good ones, a
  max_len bound some frames exceed, and decode's out_bytes bound
  (ZMQG_OPT_VERIFY_FIRST);
* decode wire lengths 0, 1, 7, 8, 32, 33, 63, 64: the header failures of
  src/curve_mechanism_base.cpp:80-97 beside the shortest valid frames;
* encode payloads of 0, 1, 31, 32, 33 bytes under each plaintext header
  (1, 2, 8 and 11 bytes: plain flags, SUBSCRIBE / CANCEL with and without
  downgrade_sub);
* every frame start modulo 16, on the payload side and on the wire side;
* 7 frames (one wave, 57 lanes without a frame);
* three sessions with their own keys (several sessions: the replay tables);
* nonces from the device's send counters (ZMQG_OPT_NONCE_AUTO) and explicit;
* step 1 as a uniform step: waves whose shortest frame has 3, 4 or 5 windows
  (payloads 159, 160, 223, 224, 287), uniform and with one shorter lane per
  wave, with and without ZMQG_OPT_STREAM_OUT;
* uniform batches with an odd and an even number of uniform steps (payloads
  1024 and 1088)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_parity import dev, host
from tests.test_gpu_timed_path import _ctx

pytestmark = pytest.mark.gpu

N = 320
FILL = 0xEE


def _offsets(sizes, mods):
    """Frame i at the first place at or after frame i - 1's end that is
    mods[i] modulo 16 (a gap of 0..15 bytes stays between frames)."""
    off, pos = [], 0
    for s, m in zip(sizes, mods):
        pos += (int(m) - pos) % 16
        off.append(pos)
        pos += int(s)
    return np.array(off, np.uint64), pos + 16


def make(seed, lens, flags=None, sid=None, nsess=1, downgrade=False, in_mod=None, out_mod=None, max_len=0):
    """A batch and the oracle's results for it.  Frames whose sid is not a
    session of the context, or whose payload is above max_len, are left out of
    the oracle's run: encode must not touch their wire region."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.uint32)
    n = len(lens)
    flags = rng.integers(0, 4, n).astype(np.uint8) if flags is None else np.asarray(flags, np.uint8)
    sid = np.zeros(n, np.uint32) if sid is None else np.asarray(sid, np.uint32)
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(nsess)]
    wl = np.array([O.wire_size(int(f), downgrade, int(p)) for f, p in zip(flags, lens)], np.uint32)
    in_off, in_size = _offsets(lens, np.zeros(n, int) if in_mod is None else in_mod)
    out_off, w_size = _offsets(wl, np.zeros(n, int) if out_mod is None else out_mod)
    # where decode puts what follows the flags byte (a SUBSCRIBE / CANCEL frame's command name comes with it)
    dec_off, dec_size = _offsets(wl - 33, np.zeros(n, int) if in_mod is None else in_mod)
    inp = rng.integers(0, 256, in_size, dtype=np.uint8)
    known = sid < nsess
    fits = (lens <= max_len) if max_len else np.ones(n, bool)
    good = known & fits
    nonce = np.zeros(n, np.uint64)  # per session 3, 4, ... over the frames that are encoded
    for s in range(nsess):
        k = np.nonzero(good & (sid == s))[0]
        nonce[k] = 3 + np.arange(len(k), dtype=np.uint64)
    g = np.nonzero(good)[0]
    sess = O.make_sessions(precoms, downgrade_sub=downgrade)
    wire = O.encode_batch(sess, sid[g], nonce[g], flags[g], in_off[g], lens[g], inp, out_off[g], w_size)
    return dict(n=n, lens=lens, flags=flags, sid=sid, nsess=nsess, precoms=precoms, downgrade=downgrade, wl=wl,
                in_off=in_off, out_off=out_off, in_size=in_size, w_size=w_size, dec_off=dec_off, dec_size=dec_size,
                inp=inp, nonce=nonce, good=good, known=known, fits=fits, wire=wire, max_len=max_len)


def _covered(off, lens, size, pick):
    m = np.zeros(size, bool)
    for a, L, p in zip(off, lens, pick):
        if p:
            m[int(a):int(a) + int(L)] = True
    return m


def check_encode(torch, C, b, nonce_auto=False, stream_out=False):
    enc = _ctx(C, "0", b["nsess"])
    for s, k in enumerate(b["precoms"]):
        enc.session_set(s, k, O.CLIENT_PREFIX, O.SERVER_PREFIX, b["downgrade"])
        enc.set_nonce(s, 3)
    out = torch.full((b["w_size"],), FILL, dtype=torch.uint8, device="cuda")
    est = torch.full((b["n"],), -1, dtype=torch.int32, device="cuda")
    enc.encode_batch(dev(torch, b["sid"]), None if nonce_auto else dev(torch, b["nonce"]), dev(torch, b["flags"]),
                     dev(torch, b["in_off"]), dev(torch, b["lens"]), dev(torch, b["inp"]), dev(torch, b["out_off"]),
                     out, max_len=b["max_len"], status_out=est, nonce_auto=nonce_auto, stream_out=stream_out)
    torch.cuda.synchronize()
    want = np.where(~b["known"], C.ERR_SESSION, np.where(~b["fits"], C.ERR_BOUND, 0)).astype(np.int32)
    assert np.array_equal(host(est, np.int32), want)
    got = host(out, np.uint8)
    cov = _covered(b["out_off"], b["wl"], b["w_size"], b["good"])
    diff = np.nonzero(got[cov] != b["wire"][cov])[0]
    assert diff.size == 0, f"{diff.size} wire bytes differ"
    assert (got[~cov] == FILL).all(), "bytes outside the encoded frames written"
    if nonce_auto:
        for s in range(b["nsess"]):
            assert enc.get_nonce(s) == 3 + int((b["good"] & (b["sid"] == s)).sum()), s


def check_decode(torch, C, b, wire=None, wl=None, stream_out=False, max_len=0, out_bytes=None):
    """Decode `wire` (default: the oracle's) with the batch's sids.  Expected:
    the oracle over the frames the call may process (known session, within
    max_len, payload inside out_bytes); ZMQG_ERR_SESSION frames zero-filled,
    ZMQG_ERR_BOUND frames untouched."""
    wire = b["wire"] if wire is None else wire
    wl = b["wl"] if wl is None else np.asarray(wl, np.uint32)
    n = b["n"]
    plen = np.where(wl > 33, wl - 33, 0).astype(np.uint32)
    pay_off, size = b["dec_off"], b["dec_size"]
    fits = np.ones(n, bool)
    if max_len:
        fits &= wl <= max_len
    if out_bytes is not None:
        fits &= ~((wl > 33) & (pay_off + plen > out_bytes))
    run = b["known"] & fits
    g = np.nonzero(run)[0]
    dsess = O.make_sessions(b["precoms"], enc_prefix=O.SERVER_PREFIX, dec_prefix=O.CLIENT_PREFIX,
                            downgrade_sub=b["downgrade"])
    peer = np.full(b["nsess"], 2, np.uint64)
    rpl, rfl, rst = O.decode_batch(dsess, peer, b["sid"][g], b["out_off"][g], wl[g], wire, pay_off[g], size)
    want_st = np.where(~b["known"], C.ERR_SESSION, C.ERR_BOUND).astype(np.int32)
    want_fl = np.zeros(n, np.uint8)
    want_st[g], want_fl[g] = rst, rfl
    dec = _ctx(C, "0", b["nsess"])
    for s, k in enumerate(b["precoms"]):
        dec.session_set(s, k, O.SERVER_PREFIX, O.CLIENT_PREFIX, b["downgrade"], 2)
    back = torch.full((size,), FILL, dtype=torch.uint8, device="cuda")
    fl = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    dec.decode_batch(dev(torch, b["sid"]), dev(torch, b["out_off"]), dev(torch, wl), dev(torch, wire),
                     dev(torch, pay_off), back, fl, st, stream_out=stream_out, max_len=max_len,
                     verify_first=out_bytes is not None, out_bytes=out_bytes)
    torch.cuda.synchronize()
    gst = host(st, np.int32)
    assert np.array_equal(gst, want_st), np.nonzero(gst != want_st)[0][:10]
    assert np.array_equal(host(fl, np.uint8), want_fl)
    got = host(back, np.uint8)
    want = np.full(size, FILL, np.uint8)
    for i in range(n):
        a, z = int(pay_off[i]), int(pay_off[i]) + int(plen[i])
        if run[i]:
            want[a:z] = rpl[a:z]  # (a frame that fails is zero-filled by the oracle too)
        elif not b["known"][i]:
            want[a:z] = 0
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, f"{diff.size} payload bytes differ, first at {diff[:5]}"
    for s in range(b["nsess"]):
        assert dec.get_peer_nonce(s) == int(peer[s]), s
    return want_st


# ------------------------------------------------------------------ the start-up
RAGGED = [0, 1, 31, 32, 33, 63, 64, 65, 160, 224, 1024]


def test_unknown_sessions_and_max_len(torch_cuda, C):
    rng = np.random.default_rng(1201)
    lens = np.array([RAGGED[i % len(RAGGED)] for i in rng.permutation(N)], np.uint32)
    sid = np.zeros(N, np.uint32)
    sid[[0, 63, 64, 200, 319]] = [1, 7, 0xffffffff, 2, 1]
    lens[[0, 63, 64, 200, 319]] = [33, 64, 0, 160, 1]  # (inside the bound: one failure each)
    b = make(1202, lens, sid=sid, max_len=224, in_mod=rng.integers(0, 16, N), out_mod=rng.integers(0, 16, N))
    assert (~b["fits"]).sum() > 10 and (~b["known"]).sum() == 5
    check_encode(torch_cuda, C, b)
    # decode: every frame on the wire (the ones encode refused, too), the bound on the wire length
    full = make(1202, lens, in_mod=rng.integers(0, 16, N), out_mod=rng.integers(0, 16, N))
    full["sid"], full["known"] = sid, b["known"]
    st = check_decode(torch_cuda, C, full, max_len=224 + 33)
    assert (st == C.ERR_BOUND).sum() > 10 and (st == C.ERR_SESSION).sum() == 5 and (st == 0).sum() > 200


def test_decode_out_bytes_bound(torch_cuda, C):
    lens = np.full(N, 100, np.uint32)
    lens[::7] = 0
    b = make(1203, lens)
    limit = int(b["dec_off"][250]) + 50  # frame 250 and the payloads behind it reach past the extent
    st = check_decode(torch_cuda, C, b, out_bytes=limit)
    assert (st == C.ERR_BOUND).sum() > 50 and (st[:250] == 0).all()
    assert (st[250:][lens[250:] == 0] == 0).all()  # (an empty payload is inside any extent)


def test_decode_header_failures(torch_cuda, C):
    """Wire lengths 0, 1, 7, 8, 32, 33, 63, 64: valid frames of 33, 63 and 64
    bytes, prefixes of valid frames, and frames with a broken size byte or
    command name, at every alignment."""
    rng = np.random.default_rng(1204)
    kinds = [0, 1, 7, 8, 32, 33, 63, 64]
    want_len = np.array([kinds[i % 8] for i in range(N)], np.uint32)
    lens = np.where(want_len >= 33, want_len - 33, 31).astype(np.uint32)  # (the shorter ones: cut from a 64-byte frame)
    b = make(1205, lens, flags=rng.integers(0, 4, N), in_mod=rng.integers(0, 16, N), out_mod=np.arange(N) % 16)
    wire = b["wire"].copy()
    for i in range(N):
        a = int(b["out_off"][i])
        if i % 16 >= 8 and want_len[i] >= 1:  # half of them: a size byte or a name that is not MESSAGE's
            if i % 3 == 0:
                wire[a] = [0, 6, 8, 200][(i // 16) % 4]
            elif want_len[i] >= 8:
                wire[a + 1 + (i // 16) % 7] ^= 0x20
    st = check_decode(torch_cuda, C, b, wire=wire, wl=want_len)
    for code in (C.ERR_MALFORMED_UNSPECIFIED, C.ERR_UNEXPECTED_COMMAND, C.ERR_MALFORMED_MESSAGE, 0):
        assert (st == code).sum() >= 8, hex(code)


@pytest.mark.parametrize("downgrade", [False, True])
@pytest.mark.parametrize("nonce_auto", [False, True])
def test_encode_headers_and_short_payloads(torch_cuda, C, downgrade, nonce_auto):
    """Payloads 0, 1, 31, 32, 33 under plain flags (1-byte header), SUBSCRIBE
    and CANCEL (11 and 8 bytes, 2 with downgrade_sub), MORE and COMMAND bits
    mixed in; every payload start modulo 16 against every header."""
    pl = [0, 1, 31, 32, 33]
    fl = [0, 1, 2, 3, 12, 13, 16, 17]
    lens = np.array([pl[i % 5] for i in range(N)], np.uint32)
    flags = np.array([fl[(i // 5) % 8] for i in range(N)], np.uint8)
    b = make(1206, lens, flags=flags, downgrade=downgrade, in_mod=(np.arange(N) // 40 * 2 + np.arange(N) % 2) % 16,
             out_mod=(np.arange(N) * 7) % 16)
    hl = b["wl"].astype(int) - 32 - lens.astype(int)
    assert set(hl) == ({1, 2} if downgrade else {1, 8, 11})
    check_encode(torch_cuda, C, b, nonce_auto=nonce_auto)
    check_decode(torch_cuda, C, b)


@pytest.mark.parametrize("stream_out", [False, True])
def test_every_alignment(torch_cuda, C, stream_out):
    """Frame starts 0..15 modulo 16 on both sides, all 256 pairs, 200-byte payloads (four windows)."""
    n = 256
    b = make(1207, np.full(n, 200, np.uint32), in_mod=np.arange(n) % 16, out_mod=np.arange(n) // 16)
    check_encode(torch_cuda, C, b, stream_out=stream_out)
    check_decode(torch_cuda, C, b, stream_out=stream_out)


@pytest.mark.parametrize("nonce_auto", [False, True])
def test_seven_frames(torch_cuda, C, nonce_auto):
    b = make(1208, [1024, 0, 33, 1024, 200, 1, 4000], in_mod=[0, 3, 5, 0, 9, 15, 1], out_mod=[0, 1, 2, 3, 4, 5, 6])
    check_encode(torch_cuda, C, b, nonce_auto=nonce_auto)
    check_decode(torch_cuda, C, b)


@pytest.mark.parametrize("nonce_auto", [False, True])
def test_three_sessions(torch_cuda, C, nonce_auto):
    rng = np.random.default_rng(1209)
    lens = np.array([RAGGED[i % len(RAGGED)] for i in rng.permutation(N)], np.uint32)
    sid = rng.integers(0, 3, N).astype(np.uint32)
    sid[100:164] = 1  # (one wave all on one session)
    b = make(1210, lens, sid=sid, nsess=3, in_mod=rng.integers(0, 16, N), out_mod=rng.integers(0, 16, N))
    check_encode(torch_cuda, C, b, nonce_auto=nonce_auto)
    check_decode(torch_cuda, C, b)


# ------------------------------------------------------------------ the first steps
def _uniform(payload, shorter):
    """Every frame `payload` bytes at 64-byte aligned places; `shorter`: one
    frame per wave with fewer windows (and the last wave partial anyway)."""
    lens = np.full(N, payload, np.uint32)
    if shorter:
        lens[[5, 64 + 63, 128, 192 + 31, 256 + 17]] = [payload - 64, 90, 31, 0, payload - 130]
    slot = (payload + 33 + 63) // 64 * 64
    return lens, np.arange(N, dtype=np.uint64) * slot


@pytest.fixture(scope="module")
def step_batches():
    out = {}
    for payload in (159, 160, 223, 224, 287, 1024, 1088):
        for shorter in (False, True):
            if shorter and payload > 287:
                continue
            lens, off = _uniform(payload, shorter)
            b = make(1300 + payload + int(shorter), lens)
            # (64-byte aligned payloads and wire frames: decode's 64-byte chunks, encode's cooperative stores)
            b2 = dict(b)
            b2["in_off"], b2["out_off"], b2["dec_off"] = off, off, off
            b2["in_size"] = b2["w_size"] = b2["dec_size"] = int(off[-1]) + int(off[1]) + 16
            rng = np.random.default_rng(1400 + payload)
            b2["inp"] = rng.integers(0, 256, b2["in_size"], dtype=np.uint8)
            sess = O.make_sessions(b["precoms"])
            b2["wire"] = O.encode_batch(sess, b["sid"], b["nonce"], b["flags"], off, lens, b2["inp"], off, b2["w_size"])
            out[payload, shorter] = b2
    return out


STEP_CASES = [(p, s) for p in (159, 160, 223, 224, 287) for s in (False, True)] + [(1024, False), (1088, False)]


@pytest.mark.parametrize("stream_out", [False, True])
@pytest.mark.parametrize("payload,shorter", STEP_CASES)
def test_first_steps_encode(torch_cuda, C, step_batches, payload, shorter, stream_out):
    check_encode(torch_cuda, C, step_batches[payload, shorter], nonce_auto=True, stream_out=stream_out)


@pytest.mark.parametrize("stream_out", [False, True])
@pytest.mark.parametrize("payload,shorter", STEP_CASES)
def test_first_steps_decode(torch_cuda, C, step_batches, payload, shorter, stream_out):
    b = step_batches[payload, shorter]
    wire = b["wire"].copy()  # one MAC failure in the last whole window's ciphertext of a full-length frame
    k = 70
    wire[int(b["out_off"][k]) + 33 + int(b["lens"][k]) - 2] ^= 0x04
    st = check_decode(torch_cuda, C, b, wire=wire, stream_out=stream_out)
    assert st[k] == C.ERR_CRYPTOGRAPHIC and (np.delete(st, k) == 0).all()
