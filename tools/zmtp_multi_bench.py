#!/usr/bin/env python3
"""Device ZMTP decode of many connections' receive buffers (an I/O thread's
shape): S connections, each with one receive buffer of up to 8,192 bytes
(in_batch_size, reference src/options.cpp:221) cut from a valid framed stream
of its own session, so the last frame is usually incomplete.  `full`: every
buffer holds 8,192 bytes (no slot is padding: max_frames is the buffer's worst
case for the payload size); `random`: each buffer holds 0 .. 8,192 bytes, so
about half the slots are padding.  Microseconds, per payload size and S, of
  multi     one zmqg_decode_zmtp_multi call over the S buffers;
  S calls   the same buffers through S zmqg_decode_zmtp_async calls on one
            stream (the only device parse before the multi call: the baseline);
  floor     zmqg_decode_batch on the known descriptors of the same frames, no
            padding slots: what the parse and the padding cost on top.
Each figure is the host clock around the enqueue and the stream's
synchronisation, the sessions' peer nonces reset before it (outside the
window); the C ABI is called directly with arguments built once."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libzmq_amd import curve as C  # noqa: E402

BUF = 8192


def case(S, P, reps, fill):
    dev = torch.device("cuda", 0)
    W = C.wire_size(0, 0, P)
    F = W + (9 if W > 255 else 2)
    hdr = F - W
    fpb = BUF // F          # complete frames in a full buffer = max_frames
    nf = fpb + 1            # frames encoded per connection: at least BUF bytes
    n = S * nf
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev)
    g = torch.Generator(device=dev).manual_seed(S + P)
    pay = torch.randint(0, 256, (n * P,), dtype=torch.uint8, device=dev, generator=g)
    precom = torch.randint(0, 256, (S, 32), dtype=torch.uint8, device=dev, generator=g)
    sids = np.arange(S, dtype=np.uint32)
    enc = C.CurveContext(0, S)
    enc.session_set_batch(sids, precom, C.CLIENT_PREFIX, C.SERVER_PREFIX)
    framed = torch.zeros(n * F, dtype=torch.uint8, device=dev)
    foff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    enc.encode_zmtp(i32(np.repeat(sids, nf)), i64(np.tile(np.arange(3, 3 + nf, dtype=np.uint64), S)),
                    torch.zeros(n, dtype=torch.uint8, device=dev), i64(np.arange(n, dtype=np.uint64) * P),
                    i32(np.full(n, P, np.uint32)), pay, framed, foff)
    torch.cuda.synchronize()
    assert int(foff[n].item()) == n * F
    enc.close()
    # connection s's frames are framed[s * nf * F ..); its receive buffer, the
    # first lens[s] bytes of them, is in slot s (BUF bytes) of the arena
    arena = framed.view(S, nf * F)[:, :BUF].contiguous().view(-1)
    lens = np.full(S, BUF) if fill == "full" else np.random.default_rng(S + P).integers(0, BUF + 1, S)
    cnt = lens // F         # complete frames of each buffer
    real = int(cnt.sum())
    want = [dict(frames=int(c), consumed=int(c) * F, out_bytes=int(c) * P, error=0) for c in cnt]

    dec = C.CurveContext(0, S)
    peer0 = np.full(S, 2, np.uint64)
    reset = lambda: dec.session_set_batch(sids, precom, C.SERVER_PREFIX, C.CLIENT_PREFIX, peer_nonce=peer0)
    slots = S * fpb
    s_sid, s_off, s_len = i32(sids), i64(sids.astype(np.uint64) * BUF), i32(lens)
    d_foff = torch.zeros(slots, dtype=torch.int64, device=dev)
    d_flen = torch.zeros(slots, dtype=torch.int32, device=dev)
    d_poff = torch.zeros(slots, dtype=torch.int64, device=dev)
    d_fl = torch.zeros(slots, dtype=torch.uint8, device=dev)
    d_st = torch.zeros(slots, dtype=torch.int32, device=dev)
    out = torch.zeros(S * BUF, dtype=torch.uint8, device=dev)
    res = torch.zeros((S, 4), dtype=torch.int64, device=dev)
    is_real = (torch.arange(fpb, device=dev)[None, :] < torch.from_numpy(cnt).to(dev)[:, None]).reshape(-1)
    body = (torch.arange(S, device=dev)[:, None] * BUF + torch.arange(fpb, device=dev)[None, :] * F + hdr).reshape(-1)
    lib, st = C._lib, C._stream_handle(None)
    p = lambda t, off=0: C.ctypes.c_void_p(t.data_ptr() + off)

    def timed(fn, check):
        ts = []
        for _ in range(reps + 1):
            reset()
            d_st.fill_(-1)
            res.fill_(-1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            check()
        ts = sorted(ts[1:])  # (the first call grows the workspaces)
        return ts[0] * 1e6, ts[len(ts) // 2] * 1e6

    def check_results():
        assert dec.zmtp_results(res) == want
        assert int((d_st[is_real] != 0).sum()) == 0

    a_multi = (dec._ctx, S, p(s_sid), p(s_off), p(s_len), p(arena), -1, fpb, p(d_foff), p(d_flen), p(d_poff), p(out),
               p(d_fl), p(d_st), p(res), st)

    def multi():
        rc = lib.zmqg_decode_zmtp_multi(*a_multi)
        assert rc == 0, rc

    t_multi = timed(multi, check_results)
    # the descriptors, the padding, and every payload where its body is
    assert torch.equal(d_foff[is_real], body[is_real]) and torch.equal(d_poff, d_foff)
    assert bool((d_flen[is_real] == W).all()) and bool((d_flen[~is_real] == 0).all())
    assert bool((d_st[~is_real] == C.ERR_MALFORMED_UNSPECIFIED).all())
    src = (torch.arange(S, device=dev)[:, None] * nf + torch.arange(fpb, device=dev)[None, :]).reshape(-1) * P
    probe = torch.nonzero(is_real).reshape(-1)[::max(real // 512, 1)]
    idx = torch.arange(P, device=dev)[None, :]
    assert torch.equal(out[body[probe][:, None] + idx], pay[src[probe][:, None] + idx])

    # S single-stream calls: stream s's arrays are its slots of the same tensors
    # (its offsets are then relative to its own buffer)
    a_one = [(dec._ctx, s, p(arena, s * BUF), int(lens[s]), -1, fpb, p(d_foff, 8 * s * fpb), p(d_flen, 4 * s * fpb),
              p(d_poff, 8 * s * fpb), p(out, s * BUF), p(d_fl, s * fpb), p(d_st, 4 * s * fpb), p(res, 32 * s), st)
             for s in range(S)]

    def calls():
        f = lib.zmqg_decode_zmtp_async
        for a in a_one:
            rc = f(*a)
            assert rc == 0, rc

    t_calls = timed(calls, check_results)

    # the floor: the same frames' descriptors, known to the caller
    f_sid, f_off = i32(np.repeat(sids, cnt)), body[is_real].contiguous()
    f_len = i32(np.full(real, W, np.uint32))
    a_floor = (dec._ctx, real, p(f_sid), p(f_off), p(f_len), p(arena), p(f_off), p(out), p(d_fl), p(d_st), st)

    def floor():
        rc = lib.zmqg_decode_batch(*a_floor)
        assert rc == 0, rc

    t_floor = timed(floor, lambda: None)
    assert int((d_st[:real] != 0).sum()) == 0
    dec.close()
    return fpb, real, slots, t_multi, t_calls, t_floor


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    print(f"{'payload':>7} {'buffers':>7} {'S':>5} {'max_frames':>10} {'frames/slots':>15} {'multi us':>17} "
          f"{'S calls us':>21} {'floor us':>17}   (min / median of {reps})")
    for P in (64, 1024):
        for fill in ("full", "random"):
            for S in (16, 256, 4096):
                fpb, real, slots, m, c, f = case(S, P, reps, fill)
                print(f"{P:7d} {fill:>7} {S:5d} {fpb:10d} {real:7d}/{slots:7d} {m[0]:8.1f}/{m[1]:8.1f} "
                      f"{c[0]:10.1f}/{c[1]:10.1f} {f[0]:8.1f}/{f[1]:8.1f}", flush=True)


if __name__ == "__main__":
    main()
