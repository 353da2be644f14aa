"""zmqg_decode_zmtp_multi: the receive buffers of many connections parsed and
decoded in one call, against oracle/zmtp_oracle.py (the reference's decoder
loop, src/v2_decoder.cpp:35-140) per stream and one oracle CURVE decode over
all slots in slot order (the empty padding slots included: they fail in the
header checks and touch no peer nonce).  Compared everywhere: the per-stream
results, the four descriptor arrays over every slot, statuses, flags, the
payload bytes at the bodies' offsets, every session's peer nonce, and -- with
out != in -- that nothing but the returned frames' payload regions is written."""
import functools
import struct

import numpy as np
import pytest

from oracle import oracle as O
from oracle import zmtp_oracle as Z
from tests.helpers import pack, wire_layout

PEER0 = 2  # every session's peer nonce before the call
SIZES = [0, 5, 100, 222, 223, 1024, 3000]  # the `clean` recipe of tests/test_zmtp.py


def _precoms(rng, n):
    return [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]


def _bodies(rng, precom, lens, nonce0=3):
    """MESSAGE commands (ZMTP frame bodies) of one connection: payloads of
    `lens` bytes, nonces nonce0, nonce0 + 1, ..."""
    n = len(lens)
    if n == 0:
        return []
    lens = np.asarray(lens, np.uint32)
    flags = rng.choice([0, 1, 2], n).astype(np.uint8)
    pays = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in lens]
    inp, in_off = pack(pays)
    sid = np.zeros(n, np.uint32)
    out_off, wl, total = wire_layout(flags, lens, [False], sid)
    wire = O.encode_batch(O.make_sessions([precom]), sid, np.arange(nonce0, nonce0 + n, dtype=np.uint64), flags, in_off,
                          lens, inp, out_off, total)
    return [wire[int(o):int(o) + int(w)].tobytes() for o, w in zip(out_off, wl)]


def _frames(rng, precom, lens, nonce0=3):
    return [Z.frame(b) for b in _bodies(rng, precom, lens, nonce0)]


def _large(body):
    return bytes([Z.LARGE]) + struct.pack(">Q", len(body)) + bytes(body)


JUNK = b"\x00\x10\x07MESSAGE" + bytes(range(6))  # what a gap holds: frame-like bytes no stream owns


def _arena(streams, odd=True, align=None, gaps=None):
    """Streams packed into one arena that ends with the last stream's last
    byte; odd: every offset odd and not a multiple of 16; align: every offset
    a multiple of it; gaps[s]: the bytes in front of stream s."""
    buf, offs = bytearray(), []
    for s, st in enumerate(streams):
        if gaps and gaps.get(s):
            buf += gaps[s]
        elif odd:
            buf += JUNK[:3 + 2 * (s % 5)]
            while len(buf) % 2 == 0 or len(buf) % 16 == 0:
                buf += b"\x00"
        elif align:
            buf += JUNK
            buf += bytes(-len(buf) % align)
        offs.append(len(buf))
        buf += st
    assert len(streams[-1]) > 0 and offs[-1] + len(streams[-1]) == len(buf)
    return np.frombuffer(bytes(buf), np.uint8).copy(), offs


def _oracle(C, arena, offs, lens, sids, precoms, max_msg, max_frames):
    S, ns = len(offs), len(precoms)
    slots = S * max_frames
    f_off, f_len = np.zeros(slots, np.uint64), np.zeros(slots, np.uint32)
    zfl, sid = np.zeros(slots, np.uint8), np.zeros(slots, np.uint32)  # (padding: an empty frame on session 0)
    results = []
    for s in range(S):
        r = Z.parse(arena[offs[s]:offs[s] + lens[s]].tobytes(), max_msg, max_frames)
        fr = r["frames"]
        for j, (f, body, size) in enumerate(fr):
            k = s * max_frames + j
            f_off[k], f_len[k], zfl[k], sid[k] = offs[s] + body, size, f, sids[s]
        results.append(dict(frames=len(fr), consumed=r["consumed"], error=r["error"],
                            out_bytes=sum(max(f[2] - 33, 0) for f in fr)))
    # curve_encoding_t::decode over all slots in slot order; a session the ctx
    # does not know is the library's own code (ZMQG_ERR_SESSION: not processed)
    known = sid < ns
    dec = np.concatenate([O.make_sessions([p], dec_prefix=O.CLIENT_PREFIX) for p in precoms])
    peer = np.full(ns, PEER0, np.uint64)
    out, fl, st = O.decode_batch(dec, peer, sid[known], f_off[known], f_len[known], arena, f_off[known], len(arena))
    status, flags = np.full(slots, C.ERR_SESSION, np.int64), np.zeros(slots, np.uint8)
    status[known] = st.astype(np.int64) & 0xffffffff
    flags[known] = [int(a) | Z.msg_flags(int(z)) if s_ == 0 else 0 for a, z, s_ in zip(fl, zfl[known], st)]
    return dict(results=results, f_off=f_off, f_len=f_len, zfl=zfl, sid=sid, status=status, flags=flags, out=out,
                peer=peer)


def _run(torch, C, arena, offs, lens, sids, precoms, max_msg, max_frames, in_place=False):
    dev = torch.device("cuda", 0)
    S, slots = len(offs), len(offs) * max_frames
    ctx = C.CurveContext(0, len(precoms))
    for s, p in enumerate(precoms):
        ctx.session_set(s, p, C.SERVER_PREFIX, C.CLIENT_PREFIX, False, PEER0)
    t = lambda a, dt, vt: torch.from_numpy(np.asarray(a, dt).view(vt)).to(dev)
    d_in = torch.from_numpy(arena.copy()).to(dev)
    d_out = d_in if in_place else torch.full((len(arena),), 0x77, dtype=torch.uint8, device=dev)
    d_foff = torch.full((slots,), -1, dtype=torch.int64, device=dev)
    d_flen = torch.full((slots,), -1, dtype=torch.int32, device=dev)
    d_poff = torch.full((slots,), -1, dtype=torch.int64, device=dev)
    d_fl = torch.full((slots,), 0xEE, dtype=torch.uint8, device=dev)
    d_st = torch.full((slots,), -1, dtype=torch.int32, device=dev)
    res = torch.full((S, 4), -1, dtype=torch.int64, device=dev)
    ctx.decode_zmtp_multi(t(sids, np.uint32, np.int32), t(offs, np.uint64, np.int64), t(lens, np.uint32, np.int32),
                          d_in, max_msg, max_frames, d_foff, d_flen, d_poff, d_out, d_fl, d_st, res)
    torch.cuda.synchronize()
    got = dict(results=ctx.zmtp_results(res), f_off=d_foff.cpu().numpy().view(np.uint64),
               f_len=d_flen.cpu().numpy().view(np.uint32), out_off=d_poff.cpu().numpy().view(np.uint64),
               flags=d_fl.cpu().numpy(), status=d_st.cpu().numpy().astype(np.int64) & 0xffffffff,
               out=d_out.cpu().numpy(), peer=[ctx.get_peer_nonce(s) for s in range(len(precoms))])
    ctx.close()
    return got


def _compare(got, ref, arena, max_frames, in_place=False):
    assert got["results"] == ref["results"]
    assert (got["f_off"] == ref["f_off"]).all() and (got["f_len"] == ref["f_len"]).all()
    assert (got["out_off"] == ref["f_off"]).all()  # each payload at its body's offset
    bad = np.nonzero(got["status"] != ref["status"])[0]
    assert bad.size == 0, (bad[:8].tolist(), got["status"][bad[:8]].tolist(), ref["status"][bad[:8]].tolist())
    assert (got["flags"] == ref["flags"]).all()
    assert got["peer"] == [int(x) for x in ref["peer"]]
    # the payload regions of the returned frames (a failed frame's is zero-filled), nothing else
    want = arena.copy() if in_place else np.full(len(arena), 0x77, np.uint8)
    region = np.zeros(len(arena), bool)
    for s, r in enumerate(ref["results"]):
        for k in range(s * max_frames, s * max_frames + r["frames"]):
            a, ln = int(ref["f_off"][k]), max(int(ref["f_len"][k]) - 33, 0)
            want[a:a + ln] = ref["out"][a:a + ln]
            region[a:a + ln] = True
    assert (got["out"][region] == want[region]).all()
    if not in_place:
        assert (got["out"][~region] == 0x77).all()


@pytest.mark.gpu
def test_one_stream_equals_decode_zmtp(torch_cuda, C):
    """S = 1 at offset 0: the oracle, and zmqg_decode_zmtp's own outputs."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(101)
    precom = _precoms(rng, 1)[0]
    stream = b"".join(_frames(rng, precom, rng.choice(SIZES, 400)))
    arena, max_frames = np.frombuffer(stream, np.uint8).copy(), 1000
    ref = _oracle(C, arena, [0], [len(arena)], [0], [precom], -1, max_frames)
    assert ref["results"][0]["frames"] == 400 and (ref["status"][:400] == 0).all()
    got = _run(torch, C, arena, [0], [len(arena)], [0], [precom], -1, max_frames)
    _compare(got, ref, arena, max_frames)
    ctx = C.CurveContext(0, 1)
    ctx.session_set(0, precom, C.SERVER_PREFIX, C.CLIENT_PREFIX, False, PEER0)
    d = dict(fo=torch.zeros(max_frames, dtype=torch.int64, device=dev),
             fl=torch.zeros(max_frames, dtype=torch.int32, device=dev),
             po=torch.zeros(max_frames, dtype=torch.int64, device=dev),
             out=torch.full((len(arena),), 0x77, dtype=torch.uint8, device=dev),
             mf=torch.zeros(max_frames, dtype=torch.uint8, device=dev),
             st=torch.full((max_frames,), -1, dtype=torch.int32, device=dev))
    r = ctx.decode_zmtp(0, torch.from_numpy(arena).to(dev), len(arena), -1, max_frames, d["fo"], d["fl"], d["po"],
                        d["out"], d["mf"], d["st"])
    assert [r] == got["results"] and ctx.get_peer_nonce(0) == got["peer"][0]
    assert (d["fo"].cpu().numpy().view(np.uint64) == got["f_off"]).all()
    assert (d["fl"].cpu().numpy().view(np.uint32) == got["f_len"]).all()
    assert (d["po"].cpu().numpy().view(np.uint64) == got["out_off"]).all()
    assert (d["st"].cpu().numpy().astype(np.int64) & 0xffffffff == got["status"]).all()
    assert (d["mf"].cpu().numpy() == got["flags"]).all()
    assert (d["out"].cpu().numpy() == got["out"]).all()
    ctx.close()


@functools.lru_cache(maxsize=None)
def _mixed_case():
    """About 40 streams, one session each; see test_mixed_streams."""
    from libzmq_amd import curve as C
    rng = np.random.default_rng(202)
    n_streams, max_frames = 40, 64
    precoms = _precoms(rng, n_streams)
    fr = lambda s, lens: _frames(rng, precoms[s], lens)
    streams = []
    add = lambda b: streams.append(bytes(b))
    add(b"")                                                      # 0: length 0
    add(b"".join(fr(1, [100]))[:1])                               # 1: length 1
    add(b"".join(fr(2, [64] * 5)))                                # 2: an exact multiple of frames
    add(b"".join(fr(3, [64, 5, 100, 7]))[:-(7 + 33 + 1)])         # 3: cut inside a short header (1 of 2 bytes)
    add(b"".join(fr(4, [64, 5, 400]))[:-(400 + 33 + 4)])          # 4: cut inside a LARGE header (5 of 9 bytes)
    add(b"".join(fr(5, [64, 1024, 100]))[:-50])                   # 5: cut inside a body
    f6 = fr(6, [64] * 6)
    add(b"".join(f6[:3]) + Z.frame(b"\x04PING\x00\x00\x00") + b"".join(f6[3:]))  # 6: a PING, the rest not returned
    add(b"".join(fr(7, [221, 222, 223, 224])))                    # 7: bodies of 254 .. 257 bytes
    add(b"".join(_large(b) if i % 2 else Z.frame(b) for i, b in enumerate(_bodies(rng, precoms[8], [0, 5, 64, 100]))))
    s9 = bytearray()                                              # 9: MORE / COMMAND header bits
    for i, f in enumerate(fr(9, [10, 300, 20, 30, 500])):
        s9 += bytes([f[0] | [Z.MORE, Z.COMMAND, Z.MORE | Z.COMMAND, 0, Z.MORE][i]]) + f[1:]
    add(s9)
    s10 = b""                                                     # 10: frame-like patterns inside ciphertext
    for i, b in enumerate(_bodies(rng, precoms[10], [200, 300, 1024, 100, 64])):
        b = bytearray(b)
        if i in (1, 2):
            pat = (b"\x00\x10\x07MESSAGE" + bytes(6)) * ((len(b) - 49) // 16)
            b[33:33 + len(pat)] = pat
        s10 += Z.frame(b)
    add(s10)
    add(b"".join(fr(11, [0] * 70)))                               # 11: more than max_frames frames
    s12 = bytearray(b"".join(fr(12, [100] * 6)))                  # 12: a ciphertext byte flipped in frame 2
    s12[2 * 135 + 2 + 33 + 40] ^= 0x10
    add(s12)
    add(b"".join(fr(13, [70000, 64, 5, 100])))                    # 13: tiles wholly inside a body
    add(b"".join(fr(14, [100, 70000, 64, 40000, 5])))             # 14: the same, entered mid-tile
    while len(streams) < n_streams:                               # random mixes, half of them cut
        s = len(streams)
        st = b"".join(fr(s, rng.choice(SIZES, int(rng.integers(1, 30)))))
        add(st[:int(rng.integers(1, len(st)))] if s % 2 else st)
    arena, offs = _arena(streams)
    assert all(o % 2 == 1 and o % 16 for o in offs)
    lens, sids = [len(s) for s in streams], list(range(n_streams))
    ref = _oracle(C, arena, offs, lens, sids, precoms, -1, max_frames)
    # the classes are really there
    R, st = ref["results"], ref["status"].reshape(n_streams, max_frames)
    assert R[0]["frames"] == 0 and R[1]["frames"] == 0 and R[0]["consumed"] == 0
    assert R[2] == dict(frames=5, consumed=lens[2], error=0, out_bytes=320) and (st[2, :5] == 0).all()
    assert R[3]["frames"] == 3 and R[3]["consumed"] == lens[3] - 1
    assert R[4]["frames"] == 2 and R[4]["consumed"] == lens[4] - 5
    assert R[5]["frames"] == 2 and R[5]["consumed"] < lens[5] - 50
    assert R[6]["frames"] == 4 and (st[6, :3] == 0).all() and st[6, 3] == C.ERR_UNEXPECTED_COMMAND
    assert R[6]["consumed"] == 3 * 99 + 10
    assert [int(x) for x in ref["f_len"][7 * max_frames:7 * max_frames + 4]] == [254, 255, 256, 257]
    assert (st[7, :4] == 0).all() and (st[8, :4] == 0).all() and (st[9, :5] == 0).all()
    assert [int(x) for x in ref["flags"][9 * max_frames:9 * max_frames + 5] & 2] == [0, 2, 2, 0, 0]
    assert [int(x) for x in st[10, :5]] == [0, C.ERR_CRYPTOGRAPHIC, C.ERR_CRYPTOGRAPHIC, 0, 0]
    assert R[11]["frames"] == 64 and R[11]["consumed"] == 64 * 35 and (st[11] == 0).all()
    assert [int(x) for x in st[12, :6]] == [0, 0, C.ERR_CRYPTOGRAPHIC, 0, 0, 0] and ref["peer"][12] == PEER0 + 6
    assert R[13]["frames"] == 4 and R[14]["frames"] == 5 and (st[13, :4] == 0).all() and (st[14, :5] == 0).all()
    pad = set(int(x) for s in range(n_streams) for x in st[s, R[s]["frames"]:])
    assert pad == {C.ERR_MALFORMED_UNSPECIFIED}
    return arena, offs, lens, sids, precoms, max_frames, ref


@pytest.mark.gpu
@pytest.mark.parametrize("frames_g", [None, "0"])
def test_mixed_streams(torch_cuda, C, frames_g, monkeypatch):
    """Streams at odd offsets in an arena that ends with the last one: length
    0 and 1, exact, cut inside a header / a LARGE header / a body, a PING
    mid-stream, the 255 / 256-byte boundary, LARGE with a small size, MORE /
    COMMAND bits, planted signatures, more than max_frames frames, a flipped
    ciphertext byte, bodies that cover whole tiles.  "0": the decode's
    one-lane-per-frame kernels (ZMQG_FRAMES_G=0), which OR the ZMTP flag bits
    themselves."""
    if frames_g is not None:
        monkeypatch.setenv("ZMQG_FRAMES_G", frames_g)
    arena, offs, lens, sids, precoms, max_frames, ref = _mixed_case()
    got = _run(torch_cuda, C, arena, offs, lens, sids, precoms, -1, max_frames)
    _compare(got, ref, arena, max_frames)


@pytest.mark.gpu
def test_emsgsize_and_max_len(torch_cuda, C):
    """max_msg_size = 2000 (within the frame kernel's range: the decode runs
    with max_len): a larger frame first, in the middle, at the bound, or none."""
    rng = np.random.default_rng(303)
    precoms = _precoms(rng, 5)
    lens_of = [[3000, 64, 100], [64, 100, 1024, 3000, 64, 5], [64, 1024, 1967, 5], [64, 1968, 5], [1024] * 7]
    streams = [b"".join(_frames(rng, precoms[s], l)) for s, l in enumerate(lens_of)]
    arena, offs = _arena(streams)
    lens, sids, max_frames = [len(s) for s in streams], list(range(5)), 16
    ref = _oracle(C, arena, offs, lens, sids, precoms, 2000, max_frames)
    assert [(r["frames"], r["error"]) for r in ref["results"]] == [(0, Z.EMSGSIZE), (3, Z.EMSGSIZE), (4, 0),
                                                                  (1, Z.EMSGSIZE), (7, 0)]
    assert ref["results"][1]["consumed"] == 99 + 135 + 1024 + 33 + 9
    got = _run(torch_cuda, C, arena, offs, lens, sids, precoms, 2000, max_frames)
    _compare(got, ref, arena, max_frames)


@pytest.mark.gpu
def test_tile_edges(torch_cuda, C):
    """The second frame's header at B + d for every power-of-two tile size B
    a kernel could use and d = -12 .. +2 (a header, a LARGE size field or a
    signature across the edge, or the frame right behind it), LARGE and short
    second frames alternating; all streams in one call.  Offsets are multiples
    of 16 so that B + d is the distance from the kernel's tile edge too (its
    tiles are cut in 16-byte-aligned address space)."""
    rng = np.random.default_rng(404)
    edges = sorted({4096, 8192, 16384, 32768, 65536, C.ZMTP_MULTI_TILE})
    cases = [(B, d) for B in edges for d in range(-12, 3)]
    precoms = _precoms(rng, len(cases))
    streams = []
    for s, (B, d) in enumerate(cases):
        first = B + d - 9 - 33  # a LARGE first frame: 9 + 33 + payload bytes in front of the second header
        streams.append(b"".join(_frames(rng, precoms[s], [first, 300 if s % 2 else 40, 5, 64, 100])))
    arena, offs = _arena(streams, odd=False, align=16)
    lens, sids, max_frames = [len(s) for s in streams], list(range(len(cases))), 8
    ref = _oracle(C, arena, offs, lens, sids, precoms, -1, max_frames)
    for s, (B, d) in enumerate(cases):
        k = s * max_frames
        assert ref["results"][s]["frames"] == 5 and ref["results"][s]["consumed"] == lens[s]
        assert int(ref["f_off"][k + 1]) - offs[s] == B + d + (9 if s % 2 else 2) and (ref["status"][k:k + 5] == 0).all()
    got = _run(torch_cuda, C, arena, offs, lens, sids, precoms, -1, max_frames)
    _compare(got, ref, arena, max_frames)


@pytest.mark.gpu
def test_isolation(torch_cuda, C):
    """A stream cut inside a frame, the rest of that frame and more valid
    frames in the gap behind it (bytes no stream owns): the frame is reported
    incomplete, and nothing in the gap is parsed or written."""
    rng = np.random.default_rng(505)
    precoms = _precoms(rng, 3)
    f1 = _frames(rng, precoms[1], [100, 64, 1024, 64, 100, 5])
    full = b"".join(f1)
    cut = len(f1[0]) + len(f1[1]) + 500  # inside the third frame
    streams = [b"".join(_frames(rng, precoms[0], [64, 100])), full[:cut], b"".join(_frames(rng, precoms[2], [5, 222]))]
    arena, offs = _arena(streams, gaps={2: full[cut:]})
    assert arena[offs[1]:offs[1] + len(full)].tobytes() == full and offs[2] == offs[1] + len(full)
    lens, sids, max_frames = [len(s) for s in streams], [0, 1, 2], 8
    ref = _oracle(C, arena, offs, lens, sids, precoms, -1, max_frames)
    assert ref["results"][1] == dict(frames=2, consumed=len(f1[0]) + len(f1[1]), error=0, out_bytes=164)
    assert ref["peer"][1] == PEER0 + 2 and ref["results"][2]["frames"] == 2
    got = _run(torch_cuda, C, arena, offs, lens, sids, precoms, -1, max_frames)
    _compare(got, ref, arena, max_frames)


@pytest.mark.gpu
def test_shared_session_in_place(torch_cuda, C):
    """Streams 0 and 2 on one session with the same nonces (the later one
    fails the replay rule, in slot order), a stream on a session the ctx does
    not have (ZMQG_ERR_SESSION), decoded in place (out = in)."""
    rng = np.random.default_rng(606)
    precoms = _precoms(rng, 2)
    streams = [b"".join(_frames(rng, precoms[0], [64, 100, 5])), b"".join(_frames(rng, precoms[1], [222, 223, 64, 0])),
               b"".join(_frames(rng, precoms[0], [100, 64, 300, 5])), b"".join(_frames(rng, precoms[1], [64, 64]))]
    arena, offs = _arena(streams)
    lens, sids, max_frames = [len(s) for s in streams], [0, 1, 0, 2], 8
    ref = _oracle(C, arena, offs, lens, sids, precoms, -1, max_frames)
    st = ref["status"].reshape(4, max_frames)
    assert (st[0, :3] == 0).all() and (st[1, :4] == 0).all()
    # nonces 3, 4, 5 again, then 6
    assert [int(x) for x in st[2, :4]] == [C.ERR_INVALID_SEQUENCE] * 3 + [0]
    assert (st[3, :2] == C.ERR_SESSION).all() and st[3, 2] == C.ERR_MALFORMED_UNSPECIFIED
    assert [int(x) for x in ref["peer"]] == [PEER0 + 4, PEER0 + 4]
    got = _run(torch_cuda, C, arena, offs, lens, sids, precoms, -1, max_frames, in_place=True)
    _compare(got, ref, arena, max_frames, in_place=True)
    assert got["results"][3]["frames"] == 2


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
    res = torch.full((S, 4), -1, dtype=torch.int64, device=dev)
    call = lambda sid, mf, r: C._lib.zmqg_decode_zmtp_multi(
        ctx._ctx, int(sid.numel()), C._ptr(sid), C._ptr(z64), C._ptr(z32), C._ptr(buf), -1, mf, C._ptr(z64),
        C._ptr(z32), C._ptr(z64), C._ptr(buf), C._ptr(buf), C._ptr(z32), None if r is None else C._ptr(r),
        C._stream_handle(None))
    assert call(z32, (2 ** 31 - 1) // S + 1, res) == -22
    assert call(z32, 2 ** 31, res) == -22
    assert call(z32, 4, None) == -22
    assert C._lib.zmqg_decode_zmtp_multi(None, 0, *([None] * 4), -1, 4, *([None] * 8)) == -22
    torch.cuda.synchronize()
    assert bool((res == -1).all())
    assert call(z32[:0], 4, res) == 0
    torch.cuda.synchronize()
    assert bool((res == -1).all())
    ctx.decode_zmtp_multi(z32, z64, z32, buf, -1, 0, z64, z32, z64, buf, buf, z32, res)
    torch.cuda.synchronize()
    assert ctx.zmtp_results(res) == [dict(frames=0, consumed=0, out_bytes=0, error=0)] * S
    ctx.close()
