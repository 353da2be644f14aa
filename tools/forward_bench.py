#!/usr/bin/env python3
"""A broker's round on one MI355X, measured two ways (a measurement, not a
gate): 256 source connections with 16 frames of 1 KiB each, forwarded to 16
destinations, every source to one of them.

  (a) forward    zmqg_forward_zmtp_multi: receive buffers to send buffers in
                 one asynchronous call
  (b) two_call   zmqg_decode_zmtp_multi, a stream synchronisation, the
                 statuses / flags / results / offsets / lengths read back, the
                 encode descriptors built on the host (numpy, the same rule)
                 and uploaded, zmqg_encode_zmtp_multi

Each round is bracketed by stream events; before the first event of a round
the sessions are installed again, peer nonces and send counters at their start
(the same receive buffers are decoded again).  --warmup rounds of each, then --rounds timed ones, alternating.
Prints one JSON line: the two medians and minima in microseconds, the shape,
the device and the library's source id; --out also writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libzmq_amd import curve as C  # noqa: E402
from tests import forward_model as F  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--payload", type=int, default=1024)
    ap.add_argument("--dst", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    o = ap.parse_args()
    S, K, L, D = o.streams, o.frames, o.payload, o.dst
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(S + D)]
    parts = [(0, rng.integers(0, 256, L, dtype=np.uint8).tobytes()) for _ in range(K)]
    streams = [b"".join(F.source_frames(precoms[s], parts)) for s in range(S)]
    arena, offs = F.arena_of(streams)
    route = np.arange(S, dtype=np.uint32) % D

    def t(a, dt, vt):
        return torch.from_numpy(np.ascontiguousarray(a, dt).view(vt)).to(dev)

    ctx = C.CurveContext(0, S + D)
    sid_all = np.arange(S + D, dtype=np.uint32)
    d_precom = torch.from_numpy(np.frombuffer(b"".join(precoms), np.uint8).copy()).to(dev)
    reset = lambda: ctx.session_set_batch(sid_all, d_precom, C.SERVER_PREFIX, C.CLIENT_PREFIX,
                                          peer_nonce=np.full(S + D, 2, np.uint64))
    slots, N = S * K, S * K
    d_sid, d_off = t(np.arange(S), np.uint32, np.int32), t(offs, np.uint64, np.int64)
    d_len, d_in = t([len(x) for x in streams], np.uint32, np.int32), torch.from_numpy(arena).to(dev)
    d_plain = torch.zeros(len(arena), dtype=torch.uint8, device=dev)
    d_foff, d_poff = (torch.zeros(slots, dtype=torch.int64, device=dev) for _ in range(2))
    d_flen, d_st = (torch.zeros(slots, dtype=torch.int32, device=dev) for _ in range(2))
    d_fl = torch.zeros(slots, dtype=torch.uint8, device=dev)
    d_res = torch.zeros((S, 4), dtype=torch.int64, device=dev)
    d_dst = t(S + np.arange(D), np.uint32, np.int32)
    out_bytes = N * (L + 33 + 9)
    d_out = torch.zeros(out_bytes, dtype=torch.uint8, device=dev)
    d_pair_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    d_pair_st = torch.zeros(N, dtype=torch.int32, device=dev)
    d_dres = torch.zeros((D, 4), dtype=torch.int64, device=dev)
    d_fwd = torch.zeros((S, 4), dtype=torch.int64, device=dev)
    route_idx = np.arange(S + 1, dtype=np.uint32)

    def forward():
        ctx.forward_zmtp_multi(d_sid, d_off, d_len, d_in, -1, K, d_foff, d_flen, d_poff, d_plain, d_fl, d_st, d_res,
                               d_dst, route_idx, route, d_out, d_pair_off, d_pair_st, d_dres, d_fwd)

    j = np.arange(K)[None, :]

    def two_call():
        ctx.decode_zmtp_multi(d_sid, d_off, d_len, d_in, -1, K, d_foff, d_flen, d_poff, d_plain, d_fl, d_st, d_res)
        torch.cuda.synchronize()
        frames = d_res.cpu().numpy()[:, 0:1]
        st, fl = d_st.cpu().numpy().reshape(S, K), d_fl.cpu().numpy().reshape(S, K)
        poff, flen = d_poff.cpu().numpy().reshape(S, K), d_flen.cpu().numpy().reshape(S, K)
        valid = j < frames
        bad = valid & (st != 0)
        first_bad = np.where(bad.any(1), bad.argmax(1), frames[:, 0])[:, None]
        part = valid & (j < first_bad) & ((fl & C.COMMAND) == 0)
        last = part & ((fl & C.MORE) == 0)
        end = np.where(last.any(1), K - 1 - last[:, ::-1].argmax(1), -1)[:, None]
        s_idx, k_idx = np.nonzero(part & (j <= end))
        ctx.encode_zmtp_multi(d_dst, t(route[s_idx], np.uint32, np.int32), None,
                              t(fl[s_idx, k_idx] & C.MORE, np.uint8, np.uint8), t(poff[s_idx, k_idx], np.int64, np.int64),
                              t(flen[s_idx, k_idx] - 33, np.int32, np.int32), d_plain, d_out, d_pair_off, d_pair_st,
                              d_dres)
        return len(s_idx)

    def timed(fn):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    fns = dict(forward=forward, two_call=two_call)
    for _ in range(o.warmup):
        for fn in fns.values():
            timed(fn)
    us = {k: [] for k in fns}
    for _ in range(o.rounds):
        for k, fn in fns.items():
            us[k].append(timed(fn))
    # both forms forwarded everything
    reset()
    assert two_call() == N
    torch.cuda.synchronize()
    two = d_out.cpu().numpy().copy()
    reset()  # (the send counters too: both forms seal with the same nonces)
    forward()
    torch.cuda.synchronize()
    assert [f["forwarded"] for f in ctx.forward_results(d_fwd)] == [K] * S and (d_out.cpu().numpy() == two).all()
    sid, commit = C.build_id()
    line = dict(tool="forward_bench", shape=dict(streams=S, frames=K, payload=L, dst=D, fan_out=1, pairs=N,
                                                 in_bytes=int(sum(len(x) for x in streams))),
                rounds=o.rounds, warmup=o.warmup,
                forward_us=dict(median=float(np.median(us["forward"])), min=float(min(us["forward"]))),
                two_call_us=dict(median=float(np.median(us["two_call"])), min=float(min(us["two_call"]))),
                device=torch.cuda.get_device_name(0), hip=torch.version.hip, source_id=sid, commit=commit)
    print(json.dumps(line))
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
