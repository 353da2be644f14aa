#!/usr/bin/env python3
"""Device ZMTP encode of many connections' send buffers (an I/O thread's
shape): S connections, each with about 8,192 bytes of wire to send
(out_batch_size, reference src/options.cpp:222), the frames arriving
interleaved round-robin over the connections (A1 B1 C1 ... A2 B2 C2 ...), one
session per connection, explicit nonces.  Microseconds, per payload size and S:
  multi      one zmqg_encode_zmtp_multi call over the batch as it arrived;
  multi+up   the same, with the upload of its six descriptor arrays (unsorted,
             from pageable host memory) inside the window;
  S calls    (a) one zmqg_encode_zmtp call per connection on one stream, each
             over that connection's frames (grouped beforehand, outside the
             window) into that connection's region;
  sort+call  (b) a stable argsort of the frames by connection on the host, the
             five descriptor arrays permuted there and uploaded, and one
             zmqg_encode_zmtp call: the sort and the upload are in the window;
  call       (b) without the sort and the upload: zmqg_encode_zmtp alone on the
             sorted arrays already on the device.
(a) and (b) are what a caller had before the multi call; they still need a read
back of frame_off to find each connection's run, which no figure includes.
Each figure is the host clock around the enqueue and the stream's
synchronisation; the variants alternate inside every repetition; all of them
must produce byte-identical output.  The C ABI is called directly with
arguments built once.
usage: zmtp_send_multi_bench.py [repetitions [S,S,...]]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libzmq_amd import curve as C  # noqa: E402

BUF = 8192
WARMUP = 2


def case(S, P, reps):
    dev = torch.device("cuda", 0)
    W = C.wire_size(0, 0, P)
    F = W + (9 if W > 255 else 2)
    per = BUF // F  # frames per connection
    n = S * per
    total = n * F
    up = lambda a, dt, vt: torch.from_numpy(np.ascontiguousarray(a, dt).view(vt)).to(dev)
    g = torch.Generator(device=dev).manual_seed(S + P)
    pay = torch.randint(0, 256, (n * P,), dtype=torch.uint8, device=dev, generator=g)
    precom = torch.randint(0, 256, (S, 32), dtype=torch.uint8, device=dev, generator=g)
    sids = np.arange(S, dtype=np.uint32)
    ctx = C.CurveContext(0, S)
    ctx.session_set_batch(sids, precom, C.CLIENT_PREFIX, C.SERVER_PREFIX)
    # the batch in arrival order (host arrays, as an I/O thread has them)
    h = dict(fs=np.tile(sids, per), nonce=3 + np.arange(n, dtype=np.uint64) // S, flags=np.zeros(n, np.uint8),
             in_off=np.arange(n, dtype=np.uint64) * P, len=np.full(n, P, np.uint32))
    kinds = dict(fs=(np.uint32, np.int32), nonce=(np.uint64, np.int64), flags=(np.uint8, np.uint8),
                 in_off=(np.uint64, np.int64), len=(np.uint32, np.int32))
    d = {k: up(v, *kinds[k]) for k, v in h.items()}
    d_ssid = up(sids, np.uint32, np.int32)
    outs = {k: torch.zeros(total, dtype=torch.uint8, device=dev) for k in ("multi", "calls", "sorted")}
    foff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    foff_s = torch.zeros(S * (per + 1), dtype=torch.int64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    res = torch.zeros((S, 4), dtype=torch.int64, device=dev)
    lib, st = C._lib, C._stream_handle(None)
    p = lambda t, off=0: C.ctypes.c_void_p(t.data_ptr() + off)

    def multi_args(dd):
        return (ctx._ctx, S, p(d_ssid), n, p(dd["fs"]), p(dd["nonce"]), p(dd["flags"]), p(dd["in_off"]), p(dd["len"]),
                p(pay), p(outs["multi"]), total, p(foff), p(status), p(res), st)

    a_multi = multi_args(d)

    def multi():
        rc = lib.zmqg_encode_zmtp_multi(*a_multi)
        assert rc == 0, rc

    def multi_up():
        dd = {k: up(v, *kinds[k]) for k, v in h.items()}
        rc = lib.zmqg_encode_zmtp_multi(*multi_args(dd))
        assert rc == 0, rc
        return dd  # (kept alive until the synchronisation)

    # (a) connection s's frames, grouped: slot s (per entries) of the sorted arrays
    order = np.argsort(h["fs"], kind="stable")
    g_sid = up(h["fs"][order], np.uint32, np.int32)  # (session = connection here)
    gs = {k: up(h[k][order], *kinds[k]) for k in ("nonce", "flags", "in_off", "len")}
    width = dict(nonce=8, flags=1, in_off=8, len=4)
    a_one = [(ctx._ctx, per, p(g_sid, 4 * s * per), *(p(gs[k], width[k] * s * per) for k in ("nonce", "flags", "in_off",
                                                                                              "len")),
              p(pay), p(outs["calls"], s * per * F), p(foff_s, 8 * s * (per + 1)), st) for s in range(S)]

    def calls():
        f = lib.zmqg_encode_zmtp
        for a in a_one:
            rc = f(*a)
            assert rc == 0, rc

    # (b) the sort on the host, then one call
    def sort_call():
        o = np.argsort(h["fs"], kind="stable")
        dd = dict(sid=up(sids[h["fs"][o]], np.uint32, np.int32))
        dd.update({k: up(h[k][o], *kinds[k]) for k in ("nonce", "flags", "in_off", "len")})
        rc = lib.zmqg_encode_zmtp(ctx._ctx, n, p(dd["sid"]), p(dd["nonce"]), p(dd["flags"]), p(dd["in_off"]),
                                  p(dd["len"]), p(pay), p(outs["sorted"]), p(foff), st)
        assert rc == 0, rc
        return dd

    a_call = (ctx._ctx, n, p(g_sid), p(gs["nonce"]), p(gs["flags"]), p(gs["in_off"]), p(gs["len"]), p(pay),
              p(outs["sorted"]), p(foff), st)

    def call():
        rc = lib.zmqg_encode_zmtp(*a_call)
        assert rc == 0, rc

    variants = [("multi", multi), ("multi+up", multi_up), ("S calls", calls), ("sort+call", sort_call), ("call", call)]
    ts = {k: [] for k, _ in variants}
    for r in range(WARMUP + reps):
        for k, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = fn()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            del keep
            if r >= WARMUP:
                ts[k].append((t1 - t0) * 1e6)
    # every variant wrote the same bytes; the multi call's results
    assert int(foff[n].item()) == total
    assert torch.equal(outs["multi"], outs["sorted"]) and torch.equal(outs["multi"], outs["calls"])
    assert int((status != 0).sum()) == 0
    assert ctx.zmtp_send_results(res) == [dict(frames=per, out_off=s * per * F, out_bytes=per * F, error=0)
                                          for s in range(S)]
    ctx.close()
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))
    return per, n, total, {k: stat(v) for k, v in ts.items()}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    streams = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [16, 256, 4096]
    print("build", " ".join(C.build_id()), "device", torch.cuda.get_device_name(0))
    names = ("multi", "multi+up", "S calls", "sort+call", "call")
    print(f"{'payload':>7} {'S':>5} {'frames':>7} {'wire KiB':>9}  " + "  ".join(f"{k + ' us':>24}" for k in names)
          + f"   (median [min-max] of {reps}, after {WARMUP} warm-up rounds)")
    for P in (1024, 64):
        for S in streams:
            per, n, total, t = case(S, P, reps)
            print(f"{P:7d} {S:5d} {n:7d} {total / 1024:9.0f}  "
                  + "  ".join(f"{t[k][0]:9.1f} [{t[k][1]:.1f}-{t[k][2]:.1f}]".rjust(24) for k in names), flush=True)


if __name__ == "__main__":
    main()
