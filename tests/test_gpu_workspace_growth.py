"""The context's device buffers growing between calls (curve_ctx.hpp: the
Workspace and ZmtpWs groups, DevBuf / DevArena): every case runs its calls on
one context and one stream, small - large - small, so that the buffers grow at
the middle call only and the grown ones then serve a small batch again.  Every
call's results are compared with the oracle, which carries the sessions' peer
nonces (or send counters) from call to call as the context does.

The group each case grows is named in its docstring; the batch sizes are the
smallest that cross the groups' floors (1024 frames, 1024 candidates, 64
workgroup lists of 16 KiB)."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import zmtp_oracle as Z
from tests import zmtp_send_model as M
from tests.helpers import pack
from tests.test_gpu_boundary import _ctxs, _expected, _keys, _wire_batch, host, t
from tests import test_zmtp_multi as ZM
from tests import test_zmtp_send_multi as ZS

pytestmark = pytest.mark.gpu

COUNTS = [8, 1025, 8]


def _decode_calls(torch, C, n_sessions, counts, seed, verify_first=False):
    """decode_batch over `counts` frames per call on one context: frames of
    0-200 bytes on random sessions, nonces that rise with gaps and replays,
    some forged headers; statuses, flags, payloads (a failed frame's region is
    zero-filled) and every session's peer nonce against the oracle's
    sequential decode, call after call."""
    rng = np.random.default_rng(seed)
    keys = _keys(rng, n_sessions)
    _, dec = _ctxs(C, keys)
    peer = np.full(n_sessions, 2, np.uint64)
    base = 0
    for call, n in enumerate(counts):
        sizes = rng.integers(0, 201, n)
        sid = rng.integers(0, n_sessions, n).astype(np.uint32)
        nonce = np.uint64(base) + rng.integers(3, 12, n).astype(np.uint64) + np.arange(n, dtype=np.uint64) // 3
        base = int(nonce.max())
        flags = rng.choice([0, 1, 3], n).astype(np.uint8)
        wire, woff, wl, _ = _wire_batch(torch, C, rng, keys, sizes, sid, nonce, flags)
        for i in rng.choice(n, max(n // 40, 1), replace=False):
            wire[int(woff[i]) + 2] ^= 1
        ref_pay, ref_fl, ref_st = _expected(keys, peer, sid, woff, wl, wire)  # (advances `peer`)
        assert (ref_st == 0).any() and (ref_st != 0).any()
        if n > 1000:
            assert (ref_st == C.ERR_INVALID_SEQUENCE).sum() > n // 50
        pout = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
        out = torch.full((int(sizes.sum()) + 1,), 0x33, dtype=torch.uint8, device="cuda")
        fl = torch.zeros(n, dtype=torch.uint8, device="cuda")
        st = torch.zeros(n, dtype=torch.int32, device="cuda")
        dec.decode_batch(t(torch, sid), t(torch, woff), t(torch, wl), t(torch, wire), t(torch, pout), out, fl, st,
                         verify_first=verify_first)
        torch.cuda.synchronize()
        assert np.array_equal(host(st, np.int32), ref_st), call
        assert np.array_equal(host(fl, np.uint8), ref_fl), call
        got = host(out, np.uint8)
        for i in range(n):
            a = int(pout[i])
            if ref_st[i] == 0:
                assert np.array_equal(got[a:a + int(sizes[i])], ref_pay[i]), (call, i)
            else:
                assert not got[a:a + int(sizes[i])].any(), (call, i)
        assert got[-1] == 0x33
        assert [dec.get_peer_nonce(s) for s in range(n_sessions)] == [int(x) for x in peer], call
    dec.close()


@pytest.mark.parametrize("n_sessions", [1, 2])
def test_decode_batch_grows(torch_cuda, C, n_sessions):
    """ws.cap 1024 -> 2048 at the second call (the look-back state is
    initialised again); with two sessions the replay tables (ws.rt) grow too."""
    _decode_calls(torch_cuda, C, n_sessions, COUNTS, 500 + n_sessions)


def test_decode_verify_first_grows(torch_cuda, C):
    """ZMQG_OPT_VERIFY_FIRST: the staging area (ws.stage) is sized by each
    call's `out`, so the second call allocates it anew."""
    _decode_calls(torch_cuda, C, 1, COUNTS[:2], 510, verify_first=True)


def test_encode_nonce_auto_grows(torch_cuda, C):
    """ZMQG_OPT_NONCE_AUTO over two sessions: the nonce tables share ws.rt.
    The wire bytes equal the oracle's encode with the nonces the reference's
    get_and_inc_nonce would have given, and the send counters end where its do."""
    torch = torch_cuda
    rng = np.random.default_rng(520)
    keys = _keys(rng, 2)
    enc, _ = _ctxs(C, keys)
    sess = np.concatenate([O.make_sessions([k]) for k in keys])
    ctr = np.array([(1 << 32) - 500, 7], np.uint64)  # (session 0 crosses 2^32 in the second call)
    for s in range(2):
        enc.set_nonce(s, int(ctr[s]))
    for call, n in enumerate(COUNTS):
        sid = rng.integers(0, 2, n).astype(np.uint32)
        sizes = rng.integers(0, 201, n).astype(np.uint32)
        flags = rng.choice([0, 1], n).astype(np.uint8)
        inp, in_off = pack([rng.integers(0, 256, int(s), dtype=np.uint8).tobytes() for s in sizes])
        wl = np.array([O.wire_size(int(f), 0, int(s)) for f, s in zip(flags, sizes)], np.uint32)
        _, woff = pack([b"\0" * int(w) for w in wl])
        total = int(woff[-1]) + int(wl[-1]) + 16
        nonce = np.zeros(n, np.uint64)
        for i in range(n):
            nonce[i] = ctr[sid[i]]
            ctr[sid[i]] += np.uint64(1)
        ref = O.encode_batch(sess, sid, nonce, flags, in_off, sizes, inp, woff, total)
        out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        enc.encode_batch(t(torch, sid), None, t(torch, flags), t(torch, in_off), t(torch, sizes), t(torch, inp),
                         t(torch, woff), out, nonce_auto=True)
        torch.cuda.synchronize()
        bad = np.flatnonzero(host(out, np.uint8) != ref)
        assert bad.size == 0, (call, bad[:4])
        assert [enc.get_nonce(s) for s in range(2)] == [int(x) for x in ctr], call
    enc.close()


def _decode_zmtp_calls(torch, C, lens_per_call, seed):
    """decode_zmtp over one stream per call on one context, every frame
    returned (max_frames = the frame count + 100): the call's result, the
    descriptors, statuses, flags, payloads and the peer nonce against
    Z.parse and the oracle's decode."""
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(seed)
    precom = _keys(rng, 1)[0]
    ctx = C.CurveContext(0, 1)
    ctx.session_set(0, precom, C.SERVER_PREFIX, C.CLIENT_PREFIX, False, 2)
    dec = O.make_sessions([precom], dec_prefix=O.CLIENT_PREFIX)
    peer = np.array([2], np.uint64)
    nonce0, stream_bytes = 3, []
    for call, lens in enumerate(lens_per_call):
        stream = b"".join(ZM._frames(rng, precom, lens, nonce0))
        nonce0 += len(lens)
        max_frames = len(lens) + 100
        ref = Z.parse(stream, -1, max_frames)
        fr = ref["frames"]
        nf = len(fr)
        assert nf == len(lens) and ref["consumed"] == len(stream)
        f_off = np.array([f[1] for f in fr], np.uint64)
        f_len = np.array([f[2] for f in fr], np.uint32)
        plen = np.maximum(f_len.astype(np.int64) - 33, 0)
        p_off = np.concatenate([[0], np.cumsum(plen)[:-1]]).astype(np.uint64)
        inp = np.frombuffer(stream, np.uint8)
        pl, fl, st = O.decode_batch(dec, peer, np.zeros(nf, np.uint32), f_off, f_len, inp, p_off, int(plen.sum()))
        assert (st == 0).all()
        fl = np.array([int(fl[i]) | Z.msg_flags(fr[i][0]) for i in range(nf)], np.uint8)
        d_foff = torch.zeros(max_frames, dtype=torch.int64, device=dev)
        d_flen = torch.zeros(max_frames, dtype=torch.int32, device=dev)
        d_poff = torch.zeros(max_frames, dtype=torch.int64, device=dev)
        d_out = torch.full((len(stream) + 1,), 0x77, dtype=torch.uint8, device=dev)
        d_fl = torch.zeros(max_frames, dtype=torch.uint8, device=dev)
        d_st = torch.full((max_frames,), -1, dtype=torch.int32, device=dev)
        r = ctx.decode_zmtp(0, torch.from_numpy(inp.copy()).to(dev), len(stream), -1, max_frames, d_foff, d_flen,
                            d_poff, d_out, d_fl, d_st)
        assert r == dict(frames=nf, consumed=len(stream), out_bytes=int(plen.sum()), error=0), (call, r)
        assert (d_foff[:nf].cpu().numpy().view(np.uint64) == f_off).all(), call
        assert (d_flen[:nf].cpu().numpy().view(np.uint32) == f_len).all(), call
        assert (d_poff[:nf].cpu().numpy().view(np.uint64) == f_off).all(), call
        assert (d_st[:nf].cpu().numpy() == st).all(), call
        assert (d_fl[:nf].cpu().numpy() == fl).all(), call
        got = d_out.cpu().numpy()
        for i in range(nf):
            a, p0, ln = int(f_off[i]), int(p_off[i]), int(plen[i])
            assert got[a:a + ln].tobytes() == pl[p0:p0 + ln].tobytes(), (call, i)
        assert ctx.get_peer_nonce(0) == int(peer[0]) == nonce0 - 1, call
        stream_bytes.append(len(stream))
    ctx.close()
    return stream_bytes


def test_decode_zmtp_grows_candidates_and_frames(torch_cuda, C):
    """1100 frames of about 10 payload bytes: more than 1024 candidates (c_cap)
    and more than 1024 frames (f_cap), between two streams of 8 frames."""
    rng = np.random.default_rng(530)
    nbytes = _decode_zmtp_calls(torch_cuda, C, [rng.integers(0, 21, n) for n in (8, 1100, 8)], 531)
    assert nbytes[0] // 8 + 2 <= 1024 < 1100 < nbytes[1] // 8 + 2  # (the candidate bound of each call)


def test_decode_zmtp_grows_workgroup_lists(torch_cuda, C):
    """A stream just over 1 MiB: 65 scan workgroups of 16 KiB (g_cap 64 -> 128)."""
    nbytes = _decode_zmtp_calls(torch_cuda, C, [[5] * 8, [3000] * 346, [5] * 8], 540)
    assert nbytes[0] <= 16384 and 64 * 16384 < nbytes[1] <= 65 * 16384


def test_encode_zmtp_multi_grows(torch_cuda, C):
    """3 streams over 2 sessions, 8 - 1025 - 8 frames: s_cap 1024 -> 2048 (and
    s_tab, the workspace of the encode behind it), against the send model."""
    rng = np.random.default_rng(550)
    precoms, down, stream_sid = ZS._precoms(rng, 2), [False, True], [0, 1, 1]
    ctx = ZS._ctx(C, precoms, down)
    for n in COUNTS:
        b = M.make_batch(rng, n, 3, [0, 1, 100, 221, 222, 223, 300])
        args = (precoms, down, stream_sid, b["frame_stream"], b["nonce"], b["flags"], b["lens"], b["payloads"])
        total = ZS._total(M.model(*args, 2 ** 62, 0, encode=False))
        ref = M.model(*args, total, total + ZS.PAD)
        assert all(ref["fit"])
        got = ZS._run(torch_cuda, C, precoms, down, stream_sid, b, total, total + ZS.PAD, ctx=ctx)
        ZS._compare(got, ref, total)
    ctx.close()


def test_decode_zmtp_multi_grows(torch_cuda, C):
    """3 streams, max_frames 8 then 400: the per-frame buffers are sized by
    n_streams * max_frames, 24 slots then 1200 (f_cap 1024 -> 2048).  The
    second call's nonces lie above the first's, so the oracle's decode from
    the sessions' first peer nonce gives this call's statuses and final peer
    nonces."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(560)
    precoms = ZM._precoms(rng, 3)
    ctx = C.CurveContext(0, 3)
    for s, p in enumerate(precoms):
        ctx.session_set(s, p, C.SERVER_PREFIX, C.CLIENT_PREFIX, False, ZM.PEER0)
    tt = lambda a, dt, vt: torch.from_numpy(np.asarray(a, dt).view(vt)).to(dev)
    for max_frames, counts, nonce0 in ((8, (5, 8, 3), 3), (400, (300, 400, 17), 1000)):
        streams = [b"".join(ZM._frames(rng, precoms[s], rng.integers(0, 60, counts[s]), nonce0)) for s in range(3)]
        arena, offs = ZM._arena(streams)
        lens, sids = [len(s) for s in streams], [0, 1, 2]
        ref = ZM._oracle(C, arena, offs, lens, sids, precoms, -1, max_frames)
        assert [r["frames"] for r in ref["results"]] == list(counts)
        slots = 3 * max_frames
        d_in = torch.from_numpy(arena.copy()).to(dev)
        d_out = torch.full((len(arena),), 0x77, dtype=torch.uint8, device=dev)
        d_foff = torch.full((slots,), -1, dtype=torch.int64, device=dev)
        d_flen = torch.full((slots,), -1, dtype=torch.int32, device=dev)
        d_poff = torch.full((slots,), -1, dtype=torch.int64, device=dev)
        d_fl = torch.full((slots,), 0xEE, dtype=torch.uint8, device=dev)
        d_st = torch.full((slots,), -1, dtype=torch.int32, device=dev)
        res = torch.full((3, 4), -1, dtype=torch.int64, device=dev)
        ctx.decode_zmtp_multi(tt(sids, np.uint32, np.int32), tt(offs, np.uint64, np.int64),
                              tt(lens, np.uint32, np.int32), d_in, -1, max_frames, d_foff, d_flen, d_poff, d_out, d_fl,
                              d_st, res)
        torch.cuda.synchronize()
        got = dict(results=ctx.zmtp_results(res), f_off=d_foff.cpu().numpy().view(np.uint64),
                   f_len=d_flen.cpu().numpy().view(np.uint32), out_off=d_poff.cpu().numpy().view(np.uint64),
                   flags=d_fl.cpu().numpy(), status=d_st.cpu().numpy().astype(np.int64) & 0xffffffff,
                   out=d_out.cpu().numpy(), peer=[ctx.get_peer_nonce(s) for s in range(3)])
        ZM._compare(got, ref, arena, max_frames)
    ctx.close()
