#!/usr/bin/env python3
"""A request/reply broker's round on one MI355X, measured two ways (a
measurement, not a gate): 256 source connections with 16 messages of 1 KiB
each and 16 destinations; every message is for one destination.

  (a) static   zmqg_forward_zmtp_multi, single-part messages, each source
               routed to its one destination (the host has made the decision)
  (b) route    zmqg_forward_zmtp_router_multi with ZMQG_ROUTER_ROUTE: every
               message carries a 5-byte address part in front (the
               reference's auto-generated routing id form), looked up on the
               device in a table of 16 ids and consumed; twice the frames on
               the receive side, the same frames on the send side

The nonces fall in the same order, so both forms write the same `out` and
dst_results; the tool asserts it.  Each round is bracketed by stream events;
before the first event of a round the sessions are installed again, peer
nonces and send counters at their start.  --warmup rounds of each, then
--rounds timed ones, alternating.  Prints one JSON line: the two medians and
minima in microseconds, the shape, the device and the library's source id;
--out also writes it to a file."""
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
    ap.add_argument("--ids", type=int, default=16, help="entries of the id table (at least --dst)")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    o = ap.parse_args()
    S, K, L, D, I = o.streams, o.frames, o.payload, o.dst, max(o.ids, o.dst)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(S + D)]
    route = np.arange(S, dtype=np.uint32) % D
    rid = lambda j: b"\x00" + int(0x10000 + 37 * j).to_bytes(4, "big")  # (a 0 byte, then BE32: src/router.cpp:456-457)
    body = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for _ in range(K)]
    plain_parts = [(0, b) for b in body]
    streams_a = [b"".join(F.source_frames(precoms[s], plain_parts)) for s in range(S)]
    streams_b = [b"".join(F.source_frames(precoms[s], [x for b in body for x in ((F.MORE, rid(int(route[s]))), (0, b))]))
                 for s in range(S)]
    # id j names destination j for j < D; the others name nobody's address here
    table = C.CurveContext.forward_router_table([(rid(j), j % D) for j in range(I)])

    def t(a, dt, vt):
        return torch.from_numpy(np.ascontiguousarray(a, dt).view(vt)).to(dev)

    ctx = C.CurveContext(0, S + D)
    sid_all = np.arange(S + D, dtype=np.uint32)
    d_precom = torch.from_numpy(np.frombuffer(b"".join(precoms), np.uint8).copy()).to(dev)
    reset = lambda: ctx.session_set_batch(sid_all, d_precom, C.SERVER_PREFIX, C.CLIENT_PREFIX,
                                          peer_nonce=np.full(S + D, 2, np.uint64))

    def receive_side(streams, max_frames):
        arena, offs = F.arena_of(streams)
        slots = S * max_frames
        return dict(sid=t(np.arange(S), np.uint32, np.int32), off=t(offs, np.uint64, np.int64),
                    len=t([len(x) for x in streams], np.uint32, np.int32), inp=torch.from_numpy(arena).to(dev),
                    plain=torch.zeros(len(arena), dtype=torch.uint8, device=dev),
                    foff=torch.zeros(slots, dtype=torch.int64, device=dev),
                    poff=torch.zeros(slots, dtype=torch.int64, device=dev),
                    flen=torch.zeros(slots, dtype=torch.int32, device=dev),
                    st=torch.zeros(slots, dtype=torch.int32, device=dev),
                    fl=torch.zeros(slots, dtype=torch.uint8, device=dev),
                    res=torch.zeros((S, 4), dtype=torch.int64, device=dev),
                    pair_off=torch.zeros(slots + 1, dtype=torch.int64, device=dev),
                    pair_st=torch.zeros(slots, dtype=torch.int32, device=dev), in_bytes=int(sum(len(x) for x in streams)))

    ra, rb = receive_side(streams_a, K), receive_side(streams_b, 2 * K)
    live = S * K
    d_dst = t(S + np.arange(D), np.uint32, np.int32)
    d_out = torch.zeros(live * (L + 33 + 9), dtype=torch.uint8, device=dev)
    d_dres = torch.zeros((D, 4), dtype=torch.int64, device=dev)
    d_fwd = torch.zeros((S, 4), dtype=torch.int64, device=dev)
    idx_a = np.arange(S + 1, dtype=np.uint32)
    d_dest = torch.zeros(S * 2 * K, dtype=torch.int32, device=dev)
    i_off, i_len = t(table[0], np.uint64, np.int64), t(table[1], np.uint32, np.int32)
    i_dst, i_raw = t(table[2], np.uint32, np.int32), t(table[3], np.uint8, np.uint8)

    def static():
        r = ra
        ctx.forward_zmtp_multi(r["sid"], r["off"], r["len"], r["inp"], -1, K, r["foff"], r["flen"], r["poff"],
                               r["plain"], r["fl"], r["st"], r["res"], d_dst, idx_a, route, d_out, r["pair_off"],
                               r["pair_st"], d_dres, d_fwd)

    def routed():
        r = rb
        ctx.forward_zmtp_router_multi(r["sid"], r["off"], r["len"], r["inp"], -1, 2 * K, r["foff"], r["flen"],
                                      r["poff"], r["plain"], r["fl"], r["st"], r["res"], d_dst, None, None, d_out,
                                      r["pair_off"], r["pair_st"], d_dres, d_fwd, C.ROUTER_ROUTE, id_off=i_off,
                                      id_len=i_len, id_dst=i_dst, id_bytes=i_raw, dest_out=d_dest)

    def timed(fn):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    fns = dict(static=static, route=routed)
    for _ in range(o.warmup):
        for fn in fns.values():
            timed(fn)
    us = {k: [] for k in fns}
    for _ in range(o.rounds):
        for k, fn in fns.items():
            us[k].append(timed(fn))
    # both forms forwarded every payload part, to the same destinations, into the same bytes
    reset()
    static()
    torch.cuda.synchronize()
    one = d_out.cpu().numpy().copy()
    res_a = ctx.zmtp_send_results(d_dres)
    assert [f["forwarded"] for f in ctx.forward_results(d_fwd)] == [K] * S
    d_out.zero_()
    reset()  # (the send counters too: both forms seal with the same nonces)
    routed()
    torch.cuda.synchronize()
    assert [f["forwarded"] for f in ctx.forward_results(d_fwd)] == [2 * K] * S
    dest = d_dest.cpu().numpy().view(np.uint32).reshape(S, K, 2)
    assert (dest[:, :, 0] == C.ROUTE_ADDRESS).all() and (dest[:, :, 1] == route[:, None]).all()
    assert ctx.zmtp_send_results(d_dres) == res_a and (d_out.cpu().numpy() == one).all()
    sid, commit = C.build_id()
    line = dict(tool="forward_router_bench",
                shape=dict(streams=S, frames=K, payload=L, dst=D, ids=I, address_bytes=5, pairs_static=S * K,
                           pairs_route=S * 2 * K, live_pairs=live, in_bytes_static=ra["in_bytes"],
                           in_bytes_route=rb["in_bytes"]),
                rounds=o.rounds, warmup=o.warmup,
                static_us=dict(median=float(np.median(us["static"])), min=float(min(us["static"]))),
                route_us=dict(median=float(np.median(us["route"])), min=float(min(us["route"]))),
                device=torch.cuda.get_device_name(0), hip=torch.version.hip, source_id=sid, commit=commit)
    print(json.dumps(line))
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
