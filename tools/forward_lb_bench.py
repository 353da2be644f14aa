#!/usr/bin/env python3
"""A load-balanced broker's round on one MI355X, measured two ways (a
measurement, not a gate): 256 source connections with 16 single-part messages
of 1 KiB each and 16 destinations.

  (a) static   zmqg_forward_zmtp_multi, each source routed to one destination
               by the host (per connection and per call: all the host can do
               without reading the decode back)
  (b) lb       zmqg_forward_zmtp_lb_multi with one group of the 16
               destinations: every message takes the next destination in turn,
               chosen on the device; the same frames on both sides

Every destination gets the same number of messages either way, so both forms
write the same number of bytes per destination; the tool asserts the totals of
dst_results and the ring's order.  Each round is bracketed by stream events;
before the first event of a round the sessions are installed again, peer
nonces and send counters at their start, and the cursor is set to 0.  --warmup
rounds of each, then --rounds timed ones, alternating.  Prints one JSON line:
the two medians and minima in microseconds, the shape, the device and the
library's source id; --out also writes it to a file.  --once FORM runs one
round of one form and nothing else (for a kernel trace)."""
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
    ap.add_argument("--once", choices=["static", "lb"])
    ap.add_argument("--out")
    o = ap.parse_args()
    S, K, L, D = o.streams, o.frames, o.payload, o.dst
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(S + D)]
    route = np.arange(S, dtype=np.uint32) % D
    body = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for _ in range(K)]
    streams = [b"".join(F.source_frames(precoms[s], [(0, b) for b in body])) for s in range(S)]

    def t(a, dt, vt):
        return torch.from_numpy(np.ascontiguousarray(a, dt).view(vt)).to(dev)

    ctx = C.CurveContext(0, S + D)
    sid_all = np.arange(S + D, dtype=np.uint32)
    d_precom = torch.from_numpy(np.frombuffer(b"".join(precoms), np.uint8).copy()).to(dev)
    d_cur = torch.zeros(1, dtype=torch.int32, device=dev)

    def reset():
        ctx.session_set_batch(sid_all, d_precom, C.SERVER_PREFIX, C.CLIENT_PREFIX,
                              peer_nonce=np.full(S + D, 2, np.uint64))
        d_cur.zero_()

    arena, offs = F.arena_of(streams)
    slots = S * K
    r = dict(sid=t(np.arange(S), np.uint32, np.int32), off=t(offs, np.uint64, np.int64),
             len=t([len(x) for x in streams], np.uint32, np.int32), inp=torch.from_numpy(arena).to(dev),
             plain=torch.zeros(len(arena), dtype=torch.uint8, device=dev),
             foff=torch.zeros(slots, dtype=torch.int64, device=dev), poff=torch.zeros(slots, dtype=torch.int64, device=dev),
             flen=torch.zeros(slots, dtype=torch.int32, device=dev), st=torch.zeros(slots, dtype=torch.int32, device=dev),
             fl=torch.zeros(slots, dtype=torch.uint8, device=dev), res=torch.zeros((S, 4), dtype=torch.int64, device=dev),
             pair_off=torch.zeros(slots + 1, dtype=torch.int64, device=dev),
             pair_st=torch.zeros(slots, dtype=torch.int32, device=dev))
    d_dst = t(S + np.arange(D), np.uint32, np.int32)
    d_out = torch.zeros(slots * (L + 33 + 9), dtype=torch.uint8, device=dev)
    d_dres = torch.zeros((D, 4), dtype=torch.int64, device=dev)
    d_fwd = torch.zeros((S, 4), dtype=torch.int64, device=dev)
    idx_a = np.arange(S + 1, dtype=np.uint32)
    d_dest = torch.zeros(slots, dtype=torch.int32, device=dev)
    group = np.zeros(S, np.uint32)
    d_gidx = t([0, D], np.uint32, np.int32)
    d_ring = t(np.arange(D), np.uint32, np.int32)

    def static():
        ctx.forward_zmtp_multi(r["sid"], r["off"], r["len"], r["inp"], -1, K, r["foff"], r["flen"], r["poff"],
                               r["plain"], r["fl"], r["st"], r["res"], d_dst, idx_a, route, d_out, r["pair_off"],
                               r["pair_st"], d_dres, d_fwd)

    def balanced():
        ctx.forward_zmtp_lb_multi(r["sid"], r["off"], r["len"], r["inp"], -1, K, r["foff"], r["flen"], r["poff"],
                                  r["plain"], r["fl"], r["st"], r["res"], d_dst, d_out, r["pair_off"], r["pair_st"],
                                  d_dres, d_fwd, 0, group, d_gidx, d_ring, d_cur, dest_out=d_dest)

    def timed(fn):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    fns = dict(static=static, lb=balanced)
    if o.once:
        timed(fns[o.once])
        ctx.close()
        return
    for _ in range(o.warmup):
        for fn in fns.values():
            timed(fn)
    us = {k: [] for k in fns}
    for _ in range(o.rounds):
        for k, fn in fns.items():
            us[k].append(timed(fn))
    # both forms forwarded every message, and the same bytes to every destination
    reset()
    static()
    torch.cuda.synchronize()
    res_a = ctx.zmtp_send_results(d_dres)
    assert [f["forwarded"] for f in ctx.forward_results(d_fwd)] == [K] * S
    reset()
    balanced()
    torch.cuda.synchronize()
    res_b = ctx.zmtp_send_results(d_dres)
    assert [f["forwarded"] for f in ctx.forward_results(d_fwd)] == [K] * S
    assert all(x["error"] == 0 for x in res_a + res_b)
    assert sum(x["out_bytes"] for x in res_a) == sum(x["out_bytes"] for x in res_b)
    assert sum(x["frames"] for x in res_a) == sum(x["frames"] for x in res_b) == slots
    dest = d_dest.cpu().numpy().view(np.uint32)
    assert (dest == np.arange(slots, dtype=np.uint32) % D).all() and int(d_cur.cpu()[0]) == slots % D
    sid, commit = C.build_id()
    line = dict(tool="forward_lb_bench",
                shape=dict(streams=S, frames=K, payload=L, dst=D, groups=1, pairs=slots, live_pairs=slots,
                           in_bytes=int(sum(len(x) for x in streams)),
                           out_bytes=int(sum(x["out_bytes"] for x in res_b))),
                rounds=o.rounds, warmup=o.warmup,
                static_us=dict(median=float(np.median(us["static"])), min=float(min(us["static"]))),
                lb_us=dict(median=float(np.median(us["lb"])), min=float(min(us["lb"]))),
                device=torch.cuda.get_device_name(0), hip=torch.version.hip, source_id=sid, commit=commit)
    print(json.dumps(line))
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
