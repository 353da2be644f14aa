"""zmqg_decode_ws_multi: the WebSocket receive buffers of many connections
parsed, unmasked and decoded in one call, against tests/ws_model.py (pinned to
the reference's ws_decoder_t by tests/test_ws_model.py) per stream and one
oracle CURVE decode over all slots in slot order, as tests/test_zmtp_multi.py
does for the ZMTP framing.  Bit-exact everywhere: the per-stream results with
the control frame, the descriptor arrays over every slot, statuses, flags, the
payload bytes at the bodies' offsets, an unmasked control payload, every
session's peer nonce, that nothing outside the returned bodies and a control
payload is written, and that `in` stays as it was when out != in."""
import struct

import numpy as np
import pytest

from oracle import oracle as O
from tests import ws_model as W
from tests.test_zmtp_multi import PEER0, _bodies, _precoms

SENT = 0x77
JUNK = b"\x82\x8a\x07MESSAGE\x82\x05" + bytes(range(5))  # what a gap holds: frame-like bytes no stream owns


def _keys(rng, n, masked):
    """Per-frame key values, with the two a rotation cannot tell apart among them."""
    if not masked:
        return [None] * n
    ks = [int(k) for k in rng.integers(0, 2 ** 32, n)]
    for i, k in zip(range(2, n, 5), (0, 0xFFFFFFFF, 0x37FA213D)):
        ks[i] = k
    return ks


def _frames(rng, precom, lens, masked, nonce0=3, wsflags=None, forms=None):
    bodies = _bodies(rng, precom, lens, nonce0)
    keys = _keys(rng, len(bodies), masked)
    return [W.frame(b, k, wsflags[i] if wsflags else 0, form=forms[i] if forms else None)
            for i, (b, k) in enumerate(zip(bodies, keys))]


def _arena(streams, mods=None):
    """Streams packed into one arena behind gaps of frame-like bytes;
    stream s starts at an offset that is mods[s] mod 16 (default: odd ones)."""
    buf, offs = bytearray(), []
    for s, st in enumerate(streams):
        want = mods[s] if mods else (2 * s + 1) % 16
        buf += JUNK[:3 + s % 5]
        while len(buf) % 16 != want:
            buf += b"\x82"
        offs.append(len(buf))
        buf += st
    buf += JUNK
    return np.frombuffer(bytes(buf), np.uint8).copy(), offs


def _oracle(C, arena, offs, lens, sids, precoms, must_mask, max_msg, max_frames):
    S, ns = len(offs), len(precoms)
    slots = S * max_frames
    f_off, f_len = np.zeros(slots, np.uint64), np.zeros(slots, np.uint32)
    mfl, sid = np.zeros(slots, np.uint8), np.zeros(slots, np.uint32)  # (padding: an empty frame on session 0)
    results, plain, body, ctl = [], arena.copy(), np.zeros(len(arena), bool), np.zeros(len(arena), bool)
    put = lambda a, b: plain.__setitem__(slice(a, a + len(b)), np.frombuffer(b, np.uint8))
    for s in range(S):
        r = W.parse(arena[offs[s]:offs[s] + lens[s]].tobytes(), must_mask, max_msg, max_frames)
        fr = r["frames"]
        for j, (fl, boff, size, key) in enumerate(fr):
            k, a = s * max_frames + j, offs[s] + boff
            f_off[k], f_len[k], mfl[k], sid[k] = a, size, W.msg_flags(fl), sids[s]
            body[a:a + size] = True
            if must_mask:
                put(a, W.unmask(arena[a:a + size].tobytes(), key, 1))
        res = dict(frames=len(fr), consumed=r["consumed"], out_bytes=sum(max(f[2] - 33, 0) for f in fr),
                   error=r["error"], ctl_opcode=0, ctl_off=0, ctl_len=0)
        if r["ctl"]:
            op, coff, size, key = r["ctl"]
            a = offs[s] + coff
            res.update(ctl_opcode=op, ctl_off=a, ctl_len=size)
            ctl[a:a + size] = True
            if must_mask:
                put(a, W.unmask(arena[a:a + size].tobytes(), key, 0))
        results.append(res)
    known = sid < ns
    dec = np.concatenate([O.make_sessions([p], dec_prefix=O.CLIENT_PREFIX) for p in precoms])
    peer = np.full(ns, PEER0, np.uint64)
    out, fl, st = O.decode_batch(dec, peer, sid[known], f_off[known], f_len[known], plain, f_off[known], len(arena))
    status, flags = np.full(slots, C.ERR_SESSION, np.int64), np.zeros(slots, np.uint8)
    status[known] = st.astype(np.int64) & 0xffffffff
    flags[known] = [int(a) | int(m) if s_ == 0 else 0 for a, m, s_ in zip(fl, mfl[known], st)]
    return dict(results=results, f_off=f_off, f_len=f_len, sid=sid, status=status, flags=flags, out=out, peer=peer,
                plain=plain, body=body, ctl=ctl)


def _run(torch, C, arena, offs, lens, sids, precoms, must_mask, max_msg, max_frames, in_place):
    dev = torch.device("cuda", 0)
    S, slots = len(offs), len(offs) * max_frames
    ctx = C.CurveContext(0, len(precoms))
    for s, p in enumerate(precoms):
        ctx.session_set(s, p, C.SERVER_PREFIX, C.CLIENT_PREFIX, False, PEER0)
    t = lambda a, dt, vt: torch.from_numpy(np.asarray(a, dt).view(vt)).to(dev)
    d_in = torch.from_numpy(arena.copy()).to(dev)
    d_out = d_in if in_place else torch.full((len(arena),), SENT, dtype=torch.uint8, device=dev)
    d_foff = torch.full((slots,), -1, dtype=torch.int64, device=dev)
    d_flen = torch.full((slots,), -1, dtype=torch.int32, device=dev)
    d_poff = torch.full((slots,), -1, dtype=torch.int64, device=dev)
    d_fl = torch.full((slots,), 0xEE, dtype=torch.uint8, device=dev)
    d_st = torch.full((slots,), -1, dtype=torch.int32, device=dev)
    res = torch.full((S, 6), -1, dtype=torch.int64, device=dev)
    ctx.decode_ws_multi(t(sids, np.uint32, np.int32), t(offs, np.uint64, np.int64), t(lens, np.uint32, np.int32),
                        d_in, must_mask, max_msg, max_frames, d_foff, d_flen, d_poff, d_out, d_fl, d_st, res)
    torch.cuda.synchronize()
    got = dict(results=ctx.ws_results(res), f_off=d_foff.cpu().numpy().view(np.uint64),
               f_len=d_flen.cpu().numpy().view(np.uint32), out_off=d_poff.cpu().numpy().view(np.uint64),
               flags=d_fl.cpu().numpy(), status=d_st.cpu().numpy().astype(np.int64) & 0xffffffff,
               out=d_out.cpu().numpy(), inp=d_in.cpu().numpy(),
               peer=[ctx.get_peer_nonce(s) for s in range(len(precoms))])
    ctx.close()
    return got


def _compare(got, ref, arena, max_frames, in_place):
    for s, (g, r) in enumerate(zip(got["results"], ref["results"])):
        assert g == r, (s, g, r)
    assert (got["f_off"] == ref["f_off"]).all() and (got["f_len"] == ref["f_len"]).all()
    assert (got["out_off"] == ref["f_off"]).all()  # each payload at its body's offset
    bad = np.nonzero(got["status"] != ref["status"])[0]
    assert bad.size == 0, (bad[:8].tolist(), got["status"][bad[:8]].tolist(), ref["status"][bad[:8]].tolist())
    assert (got["flags"] == ref["flags"]).all()
    assert got["peer"] == [int(x) for x in ref["peer"]]
    # the payload regions of the returned frames (a failed frame's is zero-filled)
    payload = np.zeros(len(arena), bool)
    want = np.zeros(len(arena), np.uint8)
    for s, r in enumerate(ref["results"]):
        for k in range(s * max_frames, s * max_frames + r["frames"]):
            a, ln = int(ref["f_off"][k]), max(int(ref["f_len"][k]) - 33, 0)
            want[a:a + ln] = ref["out"][a:a + ln]
            payload[a:a + ln] = True
    assert (got["out"][payload] == want[payload]).all()
    # a control payload, unmasked
    assert (got["out"][ref["ctl"]] == ref["plain"][ref["ctl"]]).all()
    # nothing else is written: outside the returned bodies and the control
    # payloads `out` keeps what it held (in place: headers, keys, flags bytes,
    # the frames that were not returned, the gaps)
    rest = ~(ref["body"] | ref["ctl"])
    assert (got["out"][rest] == (arena[rest] if in_place else SENT)).all()
    if not in_place:
        assert (got["inp"] == arena).all()


def _check(torch, C, streams, sids, precoms, must_mask, max_msg=-1, max_frames=16, in_place=False, mods=None):
    arena, offs = _arena(streams, mods)
    lens = [len(s) for s in streams]
    ref = _oracle(C, arena, offs, lens, sids, precoms, must_mask, max_msg, max_frames)
    got = _run(torch, C, arena, offs, lens, sids, precoms, must_mask, max_msg, max_frames, in_place)
    _compare(got, ref, arena, max_frames, in_place)
    return ref, got, offs


def _ok(ref, s, max_frames, n):
    return ref["results"][s]["frames"] == n and (ref["status"][s * max_frames:s * max_frames + n] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_mixed_streams(torch_cuda, C, masked):
    """16 streams at stream_off % 16 = 0 .. 15, payloads 0 .. 40 and 1,024
    bytes under varying keys: every body alignment against every key rotation.
    In place and into a separate buffer give the same results."""
    rng = np.random.default_rng(11 + masked)
    precoms = _precoms(rng, 16)
    streams = []
    for s in range(16):
        lens = [(3 * s + 7 * i) % 41 for i in range(9)] + [1024, s, 40 - s]
        fl = [int(x) for x in rng.integers(0, 4, len(lens))]
        streams.append(b"".join(_frames(rng, precoms[s], lens, masked, wsflags=fl)))
    runs = []
    for in_place in (False, True):
        ref, got, offs = _check(torch_cuda, C, streams, list(range(16)), precoms, masked, in_place=in_place,
                                mods=list(range(16)))
        assert [o % 16 for o in offs] == list(range(16))
        assert all(_ok(ref, s, 16, 12) and ref["results"][s]["consumed"] == len(streams[s]) for s in range(16))
        assert set(int(x) for x in ref["flags"]) >= {0, 1, 2, 3}
        runs.append(got)
    for k in ("results", "f_off", "f_len", "flags", "status", "peer"):
        assert np.array_equal(np.asarray(runs[0][k]), np.asarray(runs[1][k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_size_forms(torch_cuda, C, masked):
    """Body + 1 = 125, 126, 127, 65,535, 65,536 (the three size forms at
    their bounds), non-minimal 126 / 127 forms, and one frame of 40,000 bytes
    that covers a whole tile and crosses two tile edges."""
    rng = np.random.default_rng(21 + masked)
    precoms = _precoms(rng, 4)
    pay = lambda body_plus_1: body_plus_1 - 1 - 33
    s0 = _frames(rng, precoms[0], [pay(125), pay(126), pay(127), pay(65535), pay(65536), 5], masked)
    hdrs = [W.header_bytes(b - 1, masked) - (4 if masked else 0) - 1 for b in (125, 126, 127, 65535, 65536)]
    assert hdrs == [2, 4, 4, 4, 10]
    s1 = _frames(rng, precoms[1], [0, 5, 64, 200, 7], masked, forms=[126, 127, 127, 127, None])
    s2 = _frames(rng, precoms[2], [100, 40000 - 33, 64], masked)
    s3 = _frames(rng, precoms[3], [64] * 3, masked)
    streams = [b"".join(x) for x in (s0, s1, s2, s3)]
    for in_place in (False, True):
        ref, _, offs = _check(torch_cuda, C, streams, [0, 1, 2, 3], precoms, masked, in_place=in_place,
                              mods=[0, 5, 16 - 9, 3])
        assert _ok(ref, 0, 16, 6) and _ok(ref, 1, 16, 5) and _ok(ref, 2, 16, 3) and _ok(ref, 3, 16, 3)
        a = int(ref["f_off"][2 * 16 + 1]) - offs[2] + offs[2] % 16  # the long body in the kernel's tile coordinates
        assert int(ref["f_len"][2 * 16 + 1]) == 40000 and a < C.WS_MULTI_TILE and a + 40000 > 2 * C.WS_MULTI_TILE


@pytest.mark.gpu
def test_tile_edges(torch_cuda, C):
    """The second frame's header placed so that each of its bytes in turn --
    header, key, flags byte and the 8 signature bytes: 23 for the 14-byte
    masked 127 form, 15 for the 6-byte short one -- is the last byte of the
    kernel's tile.  Stream offsets are multiples of 16, so stream offsets are
    tile coordinates."""
    rng = np.random.default_rng(31)
    T = C.WS_MULTI_TILE
    cases = [(127, d) for d in range(1, 24)] + [(None, d) for d in range(1, 16)] + [(127, 0), (None, 0)]
    precoms = _precoms(rng, len(cases))
    streams = []
    for s, (form, d) in enumerate(cases):
        first = T - d - 15 - 33  # a masked 127-form first frame: 15 bytes in front of its body
        fr = _frames(rng, precoms[s], [first, 40, 5, 64], True, forms=[127, form, None, None])
        assert len(fr[0]) == T - d
        streams.append(b"".join(fr))
    ref, _, offs = _check(torch_cuda, C, streams, list(range(len(cases))), precoms, True, max_frames=8,
                          mods=[0] * len(cases))
    for s, (form, d) in enumerate(cases):
        assert _ok(ref, s, 8, 4) and ref["results"][s]["consumed"] == len(streams[s])
        assert int(ref["f_off"][s * 8 + 1]) - offs[s] == T - d + (15 if form else 7)


def _error_streams(rng, precoms, masked, limit):
    good = lambda s: _frames(rng, precoms[s], [64, 64], masked)
    tail = lambda s: _frames(rng, precoms[s], [64], masked, nonce0=5)[0]
    key = 0x01020304 if masked else None
    S, names = [], []

    def add(name, bad):
        s = len(S)
        S.append(b"".join(good(s)) + bad + tail(s))
        names.append(name)

    body = _bodies(rng, precoms[0], [10])[0]
    f = W.frame(body, key)
    add("good", b"")
    add("fin_clear", bytes([f[0] & 0x7F]) + f[1:])
    for op in (0, 1, 3, 11):
        add("opcode_%d" % op, bytes([0x80 | op]) + f[1:])
    add("wrong_mask_bit", W.frame(body, None if masked else 0x01020304))
    add("binary_size_0", W.header(0, masked) + (W.key_bytes(key) if masked else b""))
    add("binary_at_limit", W.frame(_bodies(rng, precoms[len(S)], [limit - 33], nonce0=5)[0], key))
    add("binary_above_limit", W.frame(_bodies(rng, precoms[len(S)], [limit + 1 - 33], nonce0=5)[0], key))
    add("ping_at_limit", W.frame(bytes(limit), key, opcode=W.OP_PING))
    add("ping_above_limit", W.frame(bytes(limit + 1), key, opcode=W.OP_PING))
    add("size_2_32", W.header(2 ** 32 + 1, masked) + (W.key_bytes(key) if masked else b"") + b"\x00" + bytes(40))
    add("size_2_32_ping", W.header(2 ** 32, masked, W.OP_PING) + (W.key_bytes(key) if masked else b"") + bytes(40))
    add("good_too", b"")
    return S, names


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("max_msg", [120, -1])
def test_errors(torch_cuda, C, masked, max_msg):
    """One stream per error, each behind two good frames and in front of a
    third, beside good streams: FIN clear, opcodes 0 / 1 / 3 / 11, a wrong
    MASK bit, a binary frame of size 0, a size at and above max_msg_size for a
    binary and a control frame, a size of 2^32."""
    rng = np.random.default_rng(41 + masked)
    precoms = _precoms(rng, 20)
    streams, names = _error_streams(rng, precoms, masked, 120)
    ref, got, _ = _check(torch_cuda, C, streams, list(range(len(streams))), precoms, masked, max_msg=max_msg,
                         max_frames=8, in_place=masked)
    R = dict(zip(names, ref["results"]))
    two = len(streams[0]) - len(_frames(rng, precoms[0], [64], masked)[0])  # two good frames' bytes
    for name in names:
        r = R[name]
        if name in ("good", "good_too"):
            assert r["frames"] == 3 and r["error"] == 0 and r["consumed"] == len(streams[0])
        elif name in ("fin_clear", "wrong_mask_bit", "binary_size_0") or name.startswith("opcode"):
            assert (r["frames"], r["error"], r["consumed"], r["ctl_opcode"]) == (2, W.EPROTO, two, 0), name
        elif name.startswith("size_2_32"):
            assert (r["frames"], r["error"], r["consumed"]) == (2, W.EMSGSIZE, two), name
        elif name.endswith("above_limit") and max_msg >= 0:
            assert (r["frames"], r["error"], r["consumed"], r["ctl_opcode"]) == (2, W.EMSGSIZE, two, 0), name
        elif name.startswith("ping"):
            assert (r["frames"], r["error"], r["ctl_opcode"]) == (2, 0, W.OP_PING), name
        else:
            assert (r["frames"], r["error"]) == (4, 0), name


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_truncation(torch_cuda, C, masked):
    """A good frame followed by every proper prefix of a second frame, as the
    streams of one batch: consumed stays at the second frame's first byte.
    Then a lone 0x02 (FIN clear: an error already) and a lone 0x82."""
    rng = np.random.default_rng(51 + masked)
    precom = _precoms(rng, 1)
    f = _frames(rng, precom[0], [64, 200], masked)
    assert f[1][1] & 0x7F == 126
    streams = [f[0] + f[1][:cut] for cut in range(len(f[1]))] + [f[0] + b"\x02", f[0] + b"\x82", b"\x02", b"\x82",
                                                                 f[0] + f[1]]
    S = len(streams)
    ref, _, _ = _check(torch_cuda, C, streams, [0] * S, precom * 1, masked, max_frames=4, in_place=masked)
    for s in range(len(f[1])):
        assert ref["results"][s] == dict(frames=1, consumed=len(f[0]), out_bytes=64, error=0, ctl_opcode=0,
                                         ctl_off=0, ctl_len=0), s
    assert [ref["results"][s]["error"] for s in range(S - 5, S)] == [W.EPROTO, 0, W.EPROTO, 0, 0]
    assert [ref["results"][s]["consumed"] for s in range(S - 5, S)] == [len(f[0]), len(f[0]), 0, 0, len(streams[-1])]
    assert ref["results"][S - 1]["frames"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("in_place", [False, True])
def test_control_frames(torch_cuda, C, masked, in_place):
    """Ping, pong and close with payloads of 0, 2 and 125 bytes behind two
    good frames: ctl_*, the unmasked payload in `out`, consumed behind the
    control frame, the frames after it not returned; and a control frame that
    arrives when the stream already has max_frames frames."""
    rng = np.random.default_rng(61 + masked)
    cases = [(op, n) for op in (W.OP_PING, W.OP_PONG, W.OP_CLOSE) for n in (0, 2, 125)]
    precoms = _precoms(rng, len(cases) + 2)
    streams, want = [], []
    for s, (op, n) in enumerate(cases):
        fr = _frames(rng, precoms[s], [64, 5, 100, 64], masked)
        c = W.frame(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), 0xA1B2C3D4 + s if masked else None, opcode=op)
        streams.append(fr[0] + fr[1] + c + fr[2] + fr[3])
        want.append((2, len(fr[0]) + len(fr[1]) + len(c), op, n))
    fr = _frames(rng, precoms[-2], [64, 5, 100, 64], masked)
    ping = W.frame(b"late", 7 if masked else None, opcode=W.OP_PING)
    streams.append(fr[0] + fr[1] + fr[2] + ping + fr[3])  # max_frames = 3 reached: the ping is the next call's
    streams.append(ping + fr[0])                         # first in its stream
    ref, _, _ = _check(torch_cuda, C, streams, list(range(len(streams))), precoms, masked, max_frames=3,
                       in_place=in_place)
    for s, (frames, consumed, op, n) in enumerate(want):
        r = ref["results"][s]
        assert (r["frames"], r["consumed"], r["ctl_opcode"], r["ctl_len"], r["error"]) == (frames, consumed, op, n, 0)
    r = ref["results"][-2]
    assert (r["frames"], r["ctl_opcode"], r["consumed"]) == (3, 0, len(fr[0]) + len(fr[1]) + len(fr[2]))
    r = ref["results"][-1]
    assert (r["frames"], r["ctl_opcode"], r["consumed"], r["ctl_len"]) == (0, W.OP_PING, len(ping), 4)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_non_message_and_misuse(torch_cuda, C, masked):
    """A binary frame that is not a MESSAGE command and an empty binary body,
    each returned as its stream's last frame; signatures and WebSocket headers
    planted inside bodies; a tampered tag; a replayed nonce; two streams on
    one session; a session the ctx does not have; more frames than
    max_frames."""
    rng = np.random.default_rng(71 + masked)
    precoms = _precoms(rng, 8)
    key = 0x0BADF00D if masked else None
    fr = lambda s, lens, **kw: _frames(rng, precoms[s], lens, masked, **kw)
    streams = []
    add = lambda b: streams.append(bytes(b))
    f0 = fr(0, [64] * 4)
    add(f0[0] + f0[1] + W.frame(b"\x04PING\x00\x00\x00", key) + f0[2] + f0[3])    # 0: not a MESSAGE command
    f1 = fr(1, [64] * 3)
    add(f1[0] + W.frame(b"", key, flags=1) + f1[1])                                # 1: an empty body (size 1)
    s2 = b""                                                                       # 2: planted patterns
    for i, b in enumerate(_bodies(rng, precoms[2], [200, 300, 1024, 64])):
        b = bytearray(b)
        if i in (1, 2):
            pat = (b"\x82\x8a\x07MESSAGE\x82\x05\x89\x00\x88\x00" + bytes(2)) * ((len(b) - 49) // 16)
            b[33:33 + len(pat)] = pat
        s2 += W.frame(b, None if key is None else key + i)
    add(s2)
    b3 = [bytearray(b) for b in _bodies(rng, precoms[3], [100] * 5)]                # 3: a tag byte flipped in frame 2
    b3[2][16 + 5] ^= 0x10
    add(b"".join(W.frame(b, key) for b in b3))
    f4 = fr(4, [64, 5, 100])
    add(f4[0] + f4[1] + f4[1] + f4[2])                                             # 4: frame 1 replayed
    add(b"".join(fr(5, [100, 64])))                                                # 5: session 5 ...
    add(b"".join(fr(5, [64, 5, 300, 7])))                                          # 6: ... again: nonces 3, 4, 5 replayed, 6 new
    add(b"".join(fr(6, [64, 64])))                                                 # 7: a session the ctx does not have
    add(b"".join(fr(7, [0] * 12)))                                                 # 8: more than max_frames frames
    sids, mf = [0, 1, 2, 3, 4, 5, 5, 99, 7], 8
    ref, got, _ = _check(torch_cuda, C, streams, sids, precoms, masked, max_frames=mf, in_place=masked)
    R, st = ref["results"], ref["status"].reshape(len(streams), mf)
    assert R[0]["frames"] == 3 and [int(x) for x in st[0, :3]] == [0, 0, C.ERR_UNEXPECTED_COMMAND]
    assert R[0]["consumed"] == len(f0[0]) + len(f0[1]) + W.header_bytes(8, masked) + 8
    assert R[1]["frames"] == 2 and st[1, 0] == 0 and st[1, 1] != 0 and int(ref["f_len"][mf + 1]) == 0
    assert [int(x) for x in st[2, :4]] == [0, C.ERR_CRYPTOGRAPHIC, C.ERR_CRYPTOGRAPHIC, 0] and R[2]["frames"] == 4
    assert [int(x) for x in st[3, :5]] == [0, 0, C.ERR_CRYPTOGRAPHIC, 0, 0]
    assert [int(x) for x in st[4, :4]] == [0, 0, C.ERR_INVALID_SEQUENCE, 0]
    assert (st[5, :2] == 0).all() and [int(x) for x in st[6, :4]] == [C.ERR_INVALID_SEQUENCE] * 2 + [0, 0]
    assert (st[7, :2] == C.ERR_SESSION).all() and R[7]["frames"] == 2
    assert R[8]["frames"] == mf and R[8]["consumed"] == mf * len(streams[8]) // 12 and (st[8] == 0).all()
    assert int(ref["peer"][5]) == PEER0 + 4


@pytest.mark.gpu
def test_arguments(torch_cuda, C):
    """-EINVAL for more than 2^31 - 1 slots and for a missing ctx / results;
    max_frames == 0 zero-fills the results; n_streams == 0 does nothing."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    ctx = C.CurveContext(0, 2)
    S = 3
    z32 = torch.zeros(S, dtype=torch.int32, device=dev)
    z64 = torch.zeros(S, dtype=torch.int64, device=dev)
    buf = torch.zeros(64, dtype=torch.uint8, device=dev)
    res = torch.full((S, 6), -1, dtype=torch.int64, device=dev)
    call = lambda sid, mf, r: C._lib.zmqg_decode_ws_multi(
        ctx._ctx, int(sid.numel()), C._ptr(sid), C._ptr(z64), C._ptr(z32), C._ptr(buf), 1, -1, mf, C._ptr(z64),
        C._ptr(z32), C._ptr(z64), C._ptr(buf), C._ptr(buf), C._ptr(z32), None if r is None else C._ptr(r),
        C._stream_handle(None))
    assert call(z32, (2 ** 31 - 1) // S + 1, res) == -22
    assert call(z32, 2 ** 31, res) == -22
    assert call(z32, 4, None) == -22
    assert C._lib.zmqg_decode_ws_multi(None, 0, *([None] * 4), 1, -1, 4, *([None] * 8)) == -22
    torch.cuda.synchronize()
    assert bool((res == -1).all())
    assert call(z32[:0], 4, res) == 0
    torch.cuda.synchronize()
    assert bool((res == -1).all())
    ctx.decode_ws_multi(z32, z64, z32, buf, True, -1, 0, z64, z32, z64, buf, buf, z32, res)
    torch.cuda.synchronize()
    assert ctx.ws_results(res) == [dict(frames=0, consumed=0, out_bytes=0, error=0, ctl_opcode=0, ctl_off=0,
                                        ctl_len=0)] * S
    ctx.close()
