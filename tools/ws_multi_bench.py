#!/usr/bin/env python3
"""The WebSocket calls beside the ZMTP multi calls on the same payloads, in one
run (tools/zmtp_multi_bench.py's shapes): S connections, each with nf messages
of P bytes -- a little more than 8,192 bytes of wire (in_batch_size /
out_batch_size, reference src/options.cpp:221-222).  Microseconds, per payload
size and S, of
  send   zmqg_encode_zmtp_multi, zmqg_encode_ws_multi without and with masking
         keys, over the S * nf messages in round-robin order;
  recv   zmqg_decode_zmtp_multi, zmqg_decode_ws_multi with must_mask 0 and 1,
         over the first 8,192 bytes of every connection's region of the
         matching send output (the last frame is cut), into a separate `out`.
The ZMTP calls are the ones the library had before the WebSocket calls and
stand for it.  Each figure is the host clock around the enqueue and the
stream's synchronisation, min / median of `reps` after one untimed call; the
receive side's peer nonces are reset before each call (outside the window).
Every call's results and statuses are checked.

    python tools/ws_multi_bench.py [reps [S,...]]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libzmq_amd import curve as C  # noqa: E402

BUF = 8192
FRAMINGS = ("zmtp", "ws", "ws masked")


def frame_bytes(W, framing):
    if framing == "zmtp":
        return W + (9 if W > 255 else 2)
    size = W + 1
    return 2 + (0 if size <= 125 else 2 if size <= 0xFFFF else 8) + (4 if framing == "ws masked" else 0) + size


def timed(fn, reps, before=lambda: None, check=lambda: None):
    ts = []
    for _ in range(reps + 1):
        before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        check()
    ts = sorted(ts[1:])  # (the first call grows the workspaces)
    return ts[0] * 1e6, ts[len(ts) // 2] * 1e6


def case(S, P, reps):
    dev = torch.device("cuda", 0)
    W = C.wire_size(0, 0, P)
    nf = BUF // frame_bytes(W, "zmtp") + 1  # messages per connection: more than BUF bytes in every framing
    n = S * nf
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev)
    g = torch.Generator(device=dev).manual_seed(S + P)
    pay = torch.randint(0, 256, (n * P,), dtype=torch.uint8, device=dev, generator=g)
    precom = torch.randint(0, 256, (S, 32), dtype=torch.uint8, device=dev, generator=g)
    sids = np.arange(S, dtype=np.uint32)
    # round robin: message i belongs to connection i % S, with nonce 3 + i // S
    i = np.arange(n, dtype=np.uint64)
    a_fs, a_nonce = i32(i % S), i64(3 + i // S)
    a_flags, a_off, a_len = torch.zeros(n, dtype=torch.uint8, device=dev), i64(i * P), i32(np.full(n, P, np.uint32))
    a_mask = i32(np.random.default_rng(S + P).integers(0, 2 ** 32, n))
    # (named: the calls get raw pointers, so the tensors must outlive them)
    s_sid, s_off, s_len = i32(sids), i64(sids.astype(np.uint64) * BUF), i32(np.full(S, BUF, np.uint32))
    lib, st = C._lib, C._stream_handle(None)
    p = lambda t: None if t is None else C.ctypes.c_void_p(t.data_ptr())

    enc = C.CurveContext(0, S)
    enc.session_set_batch(sids, precom, C.CLIENT_PREFIX, C.SERVER_PREFIX)
    dec = C.CurveContext(0, S)
    peer0 = np.full(S, 2, np.uint64)
    reset = lambda: dec.session_set_batch(sids, precom, C.SERVER_PREFIX, C.CLIENT_PREFIX, peer_nonce=peer0)
    send, recv = {}, {}
    for framing in FRAMINGS:
        F = frame_bytes(W, framing)
        assert nf * F >= BUF
        wire = torch.zeros(n * F, dtype=torch.uint8, device=dev)
        foff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        e_st = torch.zeros(n, dtype=torch.int32, device=dev)
        e_res = torch.zeros((S, 4), dtype=torch.int64, device=dev)
        head = (enc._ctx, S, p(s_sid), n, p(a_fs), p(a_nonce), p(a_flags), p(a_off), p(a_len), p(pay))
        tail = (p(wire), n * F, p(foff), p(e_st), p(e_res), st)
        if framing == "zmtp":
            encode = lambda: lib.zmqg_encode_zmtp_multi(*head, *tail)
        else:
            mask = p(a_mask) if framing == "ws masked" else None
            encode = lambda: lib.zmqg_encode_ws_multi(*head, mask, *tail)

        def run_encode():
            rc = encode()
            assert rc == 0, rc

        def check_encode():
            assert int(foff[n].item()) == n * F and int((e_st != 0).sum()) == 0
            assert enc.zmtp_send_results(e_res) == [dict(frames=nf, out_off=s * nf * F, out_bytes=nf * F, error=0)
                                                    for s in range(S)]

        send[framing] = timed(run_encode, reps, check=check_encode)

        # connection s's receive buffer: the first BUF bytes of its region
        arena = wire.view(S, nf * F)[:, :BUF].contiguous().view(-1)
        fpb = BUF // F
        slots = S * fpb
        d_foff = torch.zeros(slots, dtype=torch.int64, device=dev)
        d_flen = torch.zeros(slots, dtype=torch.int32, device=dev)
        d_poff = torch.zeros(slots, dtype=torch.int64, device=dev)
        d_fl = torch.zeros(slots, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(slots, dtype=torch.int32, device=dev)
        out = torch.zeros(S * BUF, dtype=torch.uint8, device=dev)
        ws = framing != "zmtp"
        res = torch.zeros((S, 6 if ws else 4), dtype=torch.int64, device=dev)
        front = (dec._ctx, S, p(s_sid), p(s_off), p(s_len), p(arena))
        back = (-1, fpb, p(d_foff), p(d_flen), p(d_poff), p(out), p(d_fl), p(d_st), p(res), st)
        if ws:
            decode = lambda: lib.zmqg_decode_ws_multi(*front, int(framing == "ws masked"), *back)
        else:
            decode = lambda: lib.zmqg_decode_zmtp_multi(*front, *back)

        def run_decode():
            rc = decode()
            assert rc == 0, rc

        def before_decode():
            reset()
            d_st.fill_(-1)
            res.fill_(-1)

        def check_decode():
            got = dec.ws_results(res) if ws else dec.zmtp_results(res)
            assert all((r["frames"], r["consumed"], r["out_bytes"], r["error"]) == (fpb, fpb * F, fpb * P, 0)
                       for r in got)
            assert int((d_st != 0).sum()) == 0

        recv[framing] = timed(run_decode, reps, before_decode, check_decode)
        # a sample of payloads, where their bodies are
        k = torch.arange(0, slots, max(slots // 512, 1), device=dev)
        src = ((k % fpb) * S + k // fpb) * P  # slot (s, j) holds message j * S + s
        idx = torch.arange(P, device=dev)[None, :]
        assert torch.equal(out[d_poff[k][:, None] + idx], pay[src[:, None] + idx])
    enc.close()
    dec.close()
    return nf, send, recv


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    Ss = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [16, 256, 4096]
    print("build", *C.build_id())
    cols = "".join(f"{'send ' + f + ' us':>22}" for f in FRAMINGS) + "".join(f"{'recv ' + f + ' us':>22}" for f in FRAMINGS)
    print(f"{'payload':>7} {'S':>5} {'msgs':>7}{cols}   (min / median of {reps})")
    for P in (64, 1024):
        for S in Ss:
            nf, send, recv = case(S, P, reps)
            row = "".join(f"{send[f][0]:12.1f}/{send[f][1]:9.1f}" for f in FRAMINGS)
            row += "".join(f"{recv[f][0]:12.1f}/{recv[f][1]:9.1f}" for f in FRAMINGS)
            print(f"{P:7d} {S:5d} {S * nf:7d}{row}", flush=True)


if __name__ == "__main__":
    main()
