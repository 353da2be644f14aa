"""Every device Poly1305 at its reduction edges (tests/poly_steer.py): ciphertexts
solved so that the accumulator, before the final freeze, is 0, 1, 4, p - 1,
p - 5, 2^128 - 1, 2^128, 2^129, 2^26 - 1, -s, -s - 1, -s + 2^129 (mod 2^128) or
2^52 (+ 4) -- values random payloads reach with probability ~2^-100 -- through

* zmqg_decode_batch / zmqg_encode_batch under ZMQG_FRAMES_G = default, 0, 1, 2,
  4, 8 (k_frames_seq, k_frames<1, 2, 4>, k_frames_lds) and the split variants
  18, 20, 24 (steered frames in the one-lane half and in the 2/4/8-lane
  remainder of one launch);
* ZMQG_OPT_VERIFY_FIRST, alone and with ZMQG_OPT_REPLAY_HOST;
* the chunked body kernel (payloads of 4,576 bytes and more);
* zmqg_encode_msg / zmqg_decode_msg (k_msg), zmqg_box_afternm_batch /
  zmqg_box_open_afternm_batch (k_box), and one zmqg_decode_zmtp_multi call.

Decode must accept each frame (status 0, payload = ciphertext XOR keystream,
flags = (ct[0] ^ ks[32]) & 3, the oracle's peer nonce); the same frames with
tag + 1, - 1, + 5, - 5 (tag - 5 is what a missing final subtraction yields)
must fail as ZMQG_ERR_CRYPTOGRAPHIC with zero-filled payload regions; encoding
the matching plaintexts must give the steered wire byte for byte.  The
reference is big-integer Poly1305 (poly_steer.poly1305_int); the oracle supplies
the keystream and a second opinion.  All-0xff and all-zero ciphertexts under the
keys with the largest and smallest words and limbs of r run beside them.

Not steerable: ciphertexts under 16 bytes (no full block), a single block to
T = 0, and which integer (T or T + p) a form holds for a residue."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O
from oracle import zmtp_oracle as Z
from tests import poly_steer as S
from tests.test_gpu_parity import dev, host

pytestmark = pytest.mark.gpu

KEY = S.TEST_KEY
BODY_TARGETS = [0, 3, 5, 9]  # 0, p-1, 2^128-1, -s (indices into poly_steer.targets)
MSG_PAYLOADS = [15, 16, 63, 64, 255, 256, 1024, 2049, 3073, 3935]
BOX_LENGTHS = [16, 17, 64, 65, 200, 4100]


@functools.lru_cache(maxsize=None)
def frame_set():
    """The shared set: FRAME_LENGTHS x targets on one session key, frame i on a
    nonce above frame i - 1's, the free block first / middle / last in rotation."""
    frames, used = S.steered_frames(S.standard_cases(S.FRAME_LENGTHS), np.random.default_rng(20261019))
    print(f"shared steered set: {len(frames)} frames over {used} nonces")
    return frames


@functools.lru_cache(maxsize=None)
def extreme_sets():
    """All-0xff and all-zero ciphertexts of 16, 64, 65 and 1,025 bytes under the
    extreme keys, then the same bases at 65 and 1,025 bytes with one block
    solved for a target (the targets in rotation): one list per (length, base),
    each for a session of its own (the lists share the nonces)."""
    out = []
    for ln in (16, 64, 65, 1025):
        fr = S.extreme_frames(ln)
        out += [[f for f in fr if f.name == b] for b in ("base ff", "base 00")]
    rng = np.random.default_rng(20261024)
    out += [S.extreme_steered(ln, rng, b) for ln in (65, 1025) for b in (0xff, 0x00)]
    return out


def _decode_extreme(torch, C, variant, lists, what):
    frames = [f for fr in lists for f in fr]
    sid = [s for s, fr in enumerate(lists) for _ in fr]
    dec = _decoder(C, variant, len(lists))
    _check_accepted(frames, _decode(torch, dec, [f.wire for f in frames], sid), what)
    assert [dec.get_peer_nonce(s) for s in range(len(lists))] == [fr[-1].nonce for fr in lists]
    return len(frames)


def _ctx(C, variant, sessions=1):
    old = os.environ.pop("ZMQG_FRAMES_G", None)
    try:
        if variant != "default":
            os.environ["ZMQG_FRAMES_G"] = variant
        return C.CurveContext(0, sessions)
    finally:
        os.environ.pop("ZMQG_FRAMES_G", None)
        if old is not None:
            os.environ["ZMQG_FRAMES_G"] = old


def _decoder(C, variant="default", sessions=1):
    ctx = _ctx(C, variant, sessions)
    for s in range(sessions):
        ctx.session_set(s, KEY, O.SERVER_PREFIX, O.CLIENT_PREFIX, False, 2)
    return ctx


def _layout(wires):
    wl = np.array([len(w) for w in wires], np.uint32)
    woff = np.concatenate([[0], np.cumsum(wl.astype(np.uint64))[:-1]]).astype(np.uint64)
    plen = wl.astype(np.int64) - 33
    poff = np.concatenate([[0], np.cumsum(plen)[:-1]]).astype(np.uint64)
    buf = np.frombuffer(b"".join(wires) + bytes(64), np.uint8)
    return wl, woff, plen, poff, buf


def _decode(torch, ctx, wires, sid=None, **kw):
    """Decode `wires` (session sid[i], default 0) into a separate 0xEE-filled
    buffer; returns (out, flags, status, payload offsets, payload lengths)."""
    n = len(wires)
    wl, woff, plen, poff, buf = _layout(wires)
    sid = np.zeros(n, np.uint32) if sid is None else np.asarray(sid, np.uint32)
    out = torch.full((int(plen.sum()) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    fl = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.decode_batch(dev(torch, sid), dev(torch, woff), dev(torch, wl), dev(torch, buf), dev(torch, poff), out, fl, st,
                     **kw)
    torch.cuda.synchronize()
    return host(out, np.uint8), host(fl, np.uint8), host(st, np.int32), poff, plen


def _oracle_peer(wires, sid, sessions):
    wl, woff, plen, poff, buf = _layout(wires)
    peer = np.full(sessions, 2, np.uint64)
    sess = O.make_sessions([KEY] * sessions, dec_prefix=O.CLIENT_PREFIX)
    _, _, st = O.decode_batch(sess, peer, np.asarray(sid, np.uint32), woff, wl, buf, poff, int(plen.sum()) + 64)
    return st, [int(p) for p in peer]


def _check_accepted(frames, res, what):
    out, fl, st, poff, plen = res
    bad = [i for i in range(len(frames)) if st[i] != 0]
    assert not bad, (what, [(frames[i].name, len(frames[i].ct), hex(int(st[i]) & 0xffffffff)) for i in bad[:8]])
    for i, f in enumerate(frames):
        a = int(poff[i])
        assert out[a:a + int(plen[i])].tobytes() == f.payload, (what, f.name, len(f.ct))
        assert fl[i] == f.flags_byte & 3, (what, f.name, len(f.ct))
    assert (out[int(poff[-1]) + int(plen[-1]):] == 0xEE).all()


def _check_rejected(res, what):
    out, fl, st, poff, plen = res
    bad = np.flatnonzero(st != S.ERR_CRYPTOGRAPHIC)
    assert bad.size == 0, (what, bad[:8].tolist(), [hex(int(x) & 0xffffffff) for x in st[bad[:8]]])
    assert (fl == 0).all()
    assert (out[:int(plen.sum())] == 0).all(), what  # no plaintext of a forged frame


def _near_miss_batch(frames):
    """Kind k (tag + 1, - 1, + 5, - 5) of every frame on session k: the four
    share a nonce, and a failed MAC has advanced the peer nonce already."""
    wires, sid = [], []
    for k in range(4):
        wires += [f.near_misses()[k] for f in frames]
        sid += [k] * len(frames)
    return wires, sid


def _encode(torch, ctx, frames, **kw):
    n = len(frames)
    lens = np.array([len(f.payload) for f in frames], np.uint32)
    in_off = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]]).astype(np.uint64)
    inp = np.frombuffer(b"".join(f.payload for f in frames) + bytes(64), np.uint8)
    wl, woff, _, _, want = _layout([f.wire for f in frames])
    flags = np.array([f.flags_byte for f in frames], np.uint8)
    assert (flags < 4).all()
    nonce = np.array([f.nonce for f in frames], np.uint64)
    out = torch.full((len(want),), 0xEE, dtype=torch.uint8, device="cuda")
    ctx.encode_batch(dev(torch, np.zeros(n, np.uint32)), dev(torch, nonce), dev(torch, flags), dev(torch, in_off),
                     dev(torch, lens), dev(torch, inp), dev(torch, woff), out, **kw)
    torch.cuda.synchronize()
    got = host(out, np.uint8)
    total = len(want) - 64
    bad = np.flatnonzero(got[:total] != want[:total])
    if bad.size:
        i = int(np.searchsorted(woff, bad[0], side="right")) - 1
        raise AssertionError(f"encode: {bad.size} wire bytes differ, first in frame {i} ({frames[i].name}, "
                             f"{len(frames[i].ct)} bytes) at +{int(bad[0] - woff[i])}")
    assert (got[total:] == 0xEE).all()


def _encoder(C, variant="default"):
    ctx = _ctx(C, variant)
    ctx.session_set(0, KEY, O.CLIENT_PREFIX, O.SERVER_PREFIX)
    return ctx


def _full_checks(torch, C, variant, frames, what, **kw):
    """Decode, near-miss and peer-nonce checks of one steered list on one path."""
    wires = [f.wire for f in frames]
    dec = _decoder(C, variant)
    _check_accepted(frames, _decode(torch, dec, wires, **kw), what)
    ost, opeer = _oracle_peer(wires, np.zeros(len(wires), np.uint32), 1)
    assert (ost == 0).all()
    assert dec.get_peer_nonce(0) == opeer[0] == frames[-1].nonce
    nw, nsid = _near_miss_batch(frames)
    dec4 = _decoder(C, variant, 4)
    _check_rejected(_decode(torch, dec4, nw, nsid, **kw), what + " near miss")
    ost, opeer = _oracle_peer(nw, nsid, 4)
    assert (ost == S.ERR_CRYPTOGRAPHIC).all()
    assert [dec4.get_peer_nonce(s) for s in range(4)] == opeer == [frames[-1].nonce] * 4


@pytest.mark.parametrize("variant", ["default", "0", "1", "2", "4", "8"])
def test_frame_kernels(torch_cuda, C, variant):
    torch = torch_cuda
    frames = frame_set()
    _full_checks(torch, C, variant, frames, "ZMQG_FRAMES_G=" + variant)
    _encode(torch, _encoder(C, variant), frames)
    ne = _decode_extreme(torch, C, variant, extreme_sets(), "extreme keys, ZMQG_FRAMES_G=" + variant)
    nw, nsid = _near_miss_batch(extreme_sets()[-2])  # 1,025 bytes of 0xff, steered
    _check_rejected(_decode(torch, _decoder(C, variant, 4), nw, nsid), "extreme keys near miss")
    print(f"ZMQG_FRAMES_G={variant}: {len(frames)} steered frames decoded and encoded, {4 * len(frames)} near misses, "
          f"{ne} extreme-key frames")


@functools.lru_cache(maxsize=None)
def split_batch(slots):
    """slots + ~300 frames of one session with increasing nonces: the steered
    one-window frames (ciphertext <= 32 bytes), 0-payload fillers up to index
    `slots`, then every longer steered frame and a few more fillers -- so the
    multi-window frames fall in the multi-lane remainder and steered frames sit
    on both sides of the seam."""
    rng = np.random.default_rng(20261020)
    short = [ln for ln in S.FRAME_LENGTHS if ln <= 32]
    head, used = S.steered_frames(S.standard_cases(short), rng, nonce0=3)
    nfill = slots - len(head) + 7  # seven fillers beyond the seam, then the long frames
    n0 = 3 + used
    fill_nonce = np.arange(n0, n0 + nfill, dtype=np.uint64)
    tail, _ = S.steered_frames(S.standard_cases([ln for ln in S.FRAME_LENGTHS if ln > 32]), rng, nonce0=n0 + nfill)
    more = 300 - 7 - len(tail)
    end_nonce = np.arange(tail[-1].nonce + 1, tail[-1].nonce + 1 + more, dtype=np.uint64)
    z = lambda k, dt: np.zeros(k, dt)

    def fillers(nonce):
        k = len(nonce)
        w = O.encode_batch(O.make_sessions([KEY]), z(k, np.uint32), nonce, z(k, np.uint8), z(k, np.uint64),
                           z(k, np.uint32), z(1, np.uint8), np.arange(k, dtype=np.uint64) * 33, 33 * k)
        return w.tobytes()

    f1, f2 = fillers(fill_nonce), fillers(end_nonce)
    wires = ([f.wire for f in head] + [f1[33 * i:33 * i + 33] for i in range(nfill)] + [f.wire for f in tail]
             + [f2[33 * i:33 * i + 33] for i in range(more)])
    steered = {i: f for i, f in enumerate(head)}
    steered.update({len(head) + nfill + i: f for i, f in enumerate(tail)})
    nonce = np.concatenate([[f.nonce for f in head], fill_nonce, [f.nonce for f in tail], end_nonce]).astype(np.uint64)
    assert len(wires) == slots + 300 and min(steered) < slots < max(steered)
    assert all(len(f.ct) <= 32 for i, f in steered.items() if i < slots)
    return wires, steered, nonce


@pytest.mark.parametrize("variant", ["18", "20", "24"])
def test_split_kernels(torch_cuda, C, variant):
    torch = torch_cuda
    slots = 256 * torch.cuda.get_device_properties(0).multi_processor_count
    wires, steered, nonce = split_batch(slots)
    n = len(wires)
    dec = _decoder(C, variant)
    out, fl, st, poff, plen = _decode(torch, dec, wires)
    assert (st == 0).all(), [(i, hex(int(st[i]) & 0xffffffff)) for i in np.flatnonzero(st != 0)[:8]]
    for i, f in steered.items():
        a = int(poff[i])
        assert out[a:a + int(plen[i])].tobytes() == f.payload, (variant, i, f.name, len(f.ct))
        assert fl[i] == f.flags_byte & 3
    filler = np.ones(n, bool)
    filler[list(steered)] = False
    assert (fl[filler] == 0).all()
    assert dec.get_peer_nonce(0) == int(nonce[-1])
    # encode: every frame's payload is its plaintext (the fillers have none)
    lens = np.maximum(plen, 0).astype(np.uint32)
    pays = [steered[i].payload if i in steered else b"" for i in range(n)]
    flags = np.array([steered[i].flags_byte if i in steered else 0 for i in range(n)], np.uint8)
    in_off = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]]).astype(np.uint64)
    inp = np.frombuffer(b"".join(pays) + bytes(64), np.uint8)
    wl, woff, _, _, want = _layout(wires)
    wire = torch.full((len(want),), 0xEE, dtype=torch.uint8, device="cuda")
    _encoder(C, variant).encode_batch(dev(torch, np.zeros(n, np.uint32)), dev(torch, nonce), dev(torch, flags),
                                      dev(torch, in_off), dev(torch, lens), dev(torch, inp), dev(torch, woff), wire)
    torch.cuda.synchronize()
    got = host(wire, np.uint8)
    bad = np.flatnonzero(got[:-64] != want[:-64])
    assert bad.size == 0, (variant, int(np.searchsorted(woff, bad[0], side="right")) - 1)
    below = sum(i < slots for i in steered)
    print(f"ZMQG_FRAMES_G={variant}: n = {n}, {below} steered frames in the one-lane half, {len(steered) - below} in "
          f"the {int(variant) - 16}-lane remainder")


@pytest.mark.parametrize("replay_host", [False, True])
def test_verify_first(torch_cuda, C, replay_host):
    torch = torch_cuda
    frames = frame_set()
    wires = [f.wire for f in frames]
    dec = _decoder(C)
    kw = dict(verify_first=True)
    if replay_host:
        kw["verdict_in"] = torch.zeros(len(wires), dtype=torch.int32, device="cuda")
    _check_accepted(frames, _decode(torch, dec, wires, **kw), "verify first")
    # (with REPLAY_HOST the host keeps the peer nonces: the device leaves its own alone)
    assert dec.get_peer_nonce(0) == (2 if replay_host else frames[-1].nonce)
    nw, nsid = _near_miss_batch(frames)
    if replay_host:
        kw["verdict_in"] = torch.zeros(len(nw), dtype=torch.int32, device="cuda")
    dec4 = _decoder(C, "default", 4)
    _check_rejected(_decode(torch, dec4, nw, nsid, **kw), "verify first near miss")
    assert [dec4.get_peer_nonce(s) for s in range(4)] == [2 if replay_host else frames[-1].nonce] * 4
    print(f"VERIFY_FIRST{' + REPLAY_HOST' if replay_host else ''}: {len(frames)} steered frames, {len(nw)} near misses")


@functools.lru_cache(maxsize=None)
def body_set():
    """Payloads of 4,576 (the smallest the body kernel takes), 8,200 (8,233
    stream bytes: just over a tile of 64 chunks of 128), 20,000 and 65,551
    bytes x targets 0, p - 1, 2^128 - 1, -s.  The four 4,577-byte ciphertexts
    come first and are packed back to back: 37 chunks each, so two body frames
    share a tile."""
    cases = [(p + 1, ti, ("first", "middle", "last")[(i + k) % 3]) for i, p in enumerate([4576, 8200, 20000, 65551])
             for k, ti in enumerate(BODY_TARGETS)]
    frames, _ = S.steered_frames(cases, np.random.default_rng(20261021))
    assert (32 + 4577 + 127) // 128 == 37
    return frames


def test_body_kernel(torch_cuda, C):
    torch = torch_cuda
    frames = body_set()
    _full_checks(torch, C, "default", frames, "k_body")
    _encode(torch, _encoder(C), frames)
    _full_checks(torch, C, "default", frames, "k_body verify first", verify_first=True)
    # all-0xff and all-zero ciphertexts of 4,577 and 8,233 bytes under the extreme keys
    lists = []
    for ln in (4577, 8233):
        fr = S.extreme_frames(ln)
        lists += [[f for f in fr if f.name == b] for b in ("base ff", "base 00")]
    lists.append(S.extreme_steered(4577, np.random.default_rng(20261025), 0xff))  # and steered, the targets in rotation
    ne = _decode_extreme(torch, C, "default", lists, "k_body extreme keys")
    print(f"k_body: {len(frames)} steered frames decoded (plain and verify-first) and encoded, {4 * len(frames)} "
          f"near misses each, {ne} extreme-key frames")


def test_msg_calls(torch_cuda, C):
    frames, _ = S.steered_frames(S.standard_cases([p + 1 for p in MSG_PAYLOADS]), np.random.default_rng(20261022))
    enc, dec = _encoder(C), _decoder(C)
    for f in frames:
        assert enc.encode_msg(0, f.nonce, f.flags_byte, f.payload) == f.wire, (f.name, len(f.ct))
        got, gfl, gst = dec.decode_msg(0, f.wire)
        assert gst == 0 and got == f.payload and gfl == f.flags_byte & 3, (f.name, len(f.ct), hex(gst))
    assert dec.get_peer_nonce(0) == frames[-1].nonce
    # one near miss per size, the kinds and targets in rotation, on a fresh session
    dec = _decoder(C)
    for j, p in enumerate(MSG_PAYLOADS):
        same = [f for f in frames if len(f.payload) == p]
        f = same[(5 * j) % len(same)]
        got, _, gst = dec.decode_msg(0, f.near_misses()[(j + 3) % 4])
        assert gst == S.ERR_CRYPTOGRAPHIC and got is None, (f.name, len(f.ct), hex(gst))
    print(f"zmqg_encode_msg / zmqg_decode_msg: {len(frames)} steered frames, {len(MSG_PAYLOADS)} near misses")


def test_box_calls(torch_cuda, C):
    from tests.test_box import _open, _seal
    torch = torch_cuda
    rng = np.random.default_rng(20261023)
    names = S.targets(bytes(32))
    items = [S.box_item(rng, ln, ti, (ln // 16 - 1) * ((i + ti) % 2)) for i, ln in enumerate(BOX_LENGTHS)
             for ti in range(len(names)) if not (ln == 16 and names[ti][0] == "0")]
    keys, nonces, msgs, boxes = (list(x) for x in zip(*items))
    got = _seal(torch, C, keys, nonces, msgs, np.random.default_rng(3), 5)
    for i, (g, b) in enumerate(zip(got, boxes)):
        assert g == b, (i, len(msgs[i]))
    back, st = _open(torch, C, keys, nonces, boxes, np.random.default_rng(4), 7)
    assert (st == 0).all() and back == msgs
    for k in range(4):
        forged = [S.near_miss_tags(b[:16])[k] + b[16:] for b in boxes]
        back, st = _open(torch, C, keys, nonces, forged, np.random.default_rng(4), 7)
        assert (st == -1).all(), (k, np.flatnonzero(st != -1)[:8])
        assert back == [bytes(len(m)) for m in msgs]
    print(f"zmqg_box_afternm_batch / _open_: {len(items)} steered boxes, {4 * len(items)} near misses")


def test_zmtp_multi_in_place(torch_cuda, C):
    """Three receive streams of steered frames (thirds of the shared set, each
    on its own session), parsed and decoded in place by one call."""
    torch = torch_cuda
    frames = frame_set()
    k = (len(frames) + 2) // 3
    parts = [frames[0:k], frames[k:2 * k], frames[2 * k:]]
    arena, offs, lens, body = bytearray(b"\x00" * 3), [], [], []
    for part in parts:
        offs.append(len(arena))
        for f in part:
            z = Z.frame(f.wire)
            body.append(len(arena) + len(z) - len(f.wire))
            arena += z
        lens.append(len(arena) - offs[-1])
        arena += b"\x00" * 5
    arena = np.frombuffer(bytes(arena), np.uint8)
    ctx = _decoder(C, "default", 3)
    mf, slots = k, 3 * k
    t = lambda a, dt, vt: torch.from_numpy(np.asarray(a, dt).view(vt)).cuda()
    buf = torch.from_numpy(arena.copy()).cuda()
    foff = torch.full((slots,), -1, dtype=torch.int64, device="cuda")
    flen = torch.full((slots,), -1, dtype=torch.int32, device="cuda")
    poff = torch.full((slots,), -1, dtype=torch.int64, device="cuda")
    fl = torch.full((slots,), 0xEE, dtype=torch.uint8, device="cuda")
    st = torch.full((slots,), -1, dtype=torch.int32, device="cuda")
    res = torch.full((3, 4), -1, dtype=torch.int64, device="cuda")
    ctx.decode_zmtp_multi(t([0, 1, 2], np.uint32, np.int32), t(offs, np.uint64, np.int64), t(lens, np.uint32, np.int32),
                          buf, -1, mf, foff, flen, poff, buf, fl, st, res)
    torch.cuda.synchronize()
    results = ctx.zmtp_results(res)
    got, gfl, gst = buf.cpu().numpy(), fl.cpu().numpy(), st.cpu().numpy()
    gfo, gpo = foff.cpu().numpy(), poff.cpu().numpy()
    i = 0
    for s, part in enumerate(parts):
        assert results[s] == dict(frames=len(part), consumed=lens[s], error=0,
                                  out_bytes=sum(len(f.payload) for f in part))
        for j, f in enumerate(part):
            slot = s * mf + j
            assert gst[slot] == 0, (s, j, f.name, len(f.ct), hex(int(gst[slot]) & 0xffffffff))
            assert gfo[slot] == body[i] and gpo[slot] == body[i]
            assert got[body[i]:body[i] + len(f.payload)].tobytes() == f.payload, (s, j, f.name, len(f.ct))
            assert gfl[slot] == f.flags_byte & 3
            i += 1
        assert ctx.get_peer_nonce(s) == part[-1].nonce
    print(f"zmqg_decode_zmtp_multi: {len(frames)} steered frames in 3 streams, in place")
