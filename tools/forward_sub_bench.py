#!/usr/bin/env python3
"""A pub/sub broker's round on one MI355X, measured two ways (a measurement,
not a gate): 256 source connections with 16 single-part messages of 1 KiB
each and 16 destinations; every message is for one destination.

  (a) static   zmqg_forward_zmtp_multi, each source routed to its one
               destination (the host has made the decision)
  (b) subs     zmqg_forward_zmtp_sub_multi, every source routed to all 16
               destinations, a table of 16 prefixes per destination under
               which exactly that one destination matches each message (the
               device makes the decision: 16 times the pairs, one in 16 live)

Both forms write the same `out`; the tool compares them.  Each round is
bracketed by stream events; before the first event of a round the sessions are
installed again, peer nonces and send counters at their start.  --warmup
rounds of each, then --rounds timed ones, alternating.  Prints one JSON line:
the two medians and minima in microseconds, the shape, the device and the
library's source id; --out also writes it to a file."""
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
    ap.add_argument("--prefixes", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    o = ap.parse_args()
    S, K, L, D, P = o.streams, o.frames, o.payload, o.dst, o.prefixes
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(S + D)]
    route = np.arange(S, dtype=np.uint32) % D
    topic = lambda d: b"feed/%04d/" % d
    body = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for _ in range(K)]
    parts = [[(0, (topic(d) + b)[:L]) for b in body] for d in range(D)]  # every message starts with its topic
    streams = [b"".join(F.source_frames(precoms[s], parts[int(route[s])])) for s in range(S)]
    arena, offs = F.arena_of(streams)
    # destination d: its own topic last, behind P - 1 prefixes that share the topic's start and match nothing
    table = C.CurveContext.forward_subs_table([[b"feed/%04d/" % (1000 + 100 * d + i) for i in range(P - 1)] + [topic(d)]
                                               for d in range(D)])

    def t(a, dt, vt):
        return torch.from_numpy(np.ascontiguousarray(a, dt).view(vt)).to(dev)

    ctx = C.CurveContext(0, S + D)
    sid_all = np.arange(S + D, dtype=np.uint32)
    d_precom = torch.from_numpy(np.frombuffer(b"".join(precoms), np.uint8).copy()).to(dev)
    reset = lambda: ctx.session_set_batch(sid_all, d_precom, C.SERVER_PREFIX, C.CLIENT_PREFIX,
                                          peer_nonce=np.full(S + D, 2, np.uint64))
    slots, live = S * K, S * K
    d_sid, d_off = t(np.arange(S), np.uint32, np.int32), t(offs, np.uint64, np.int64)
    d_len, d_in = t([len(x) for x in streams], np.uint32, np.int32), torch.from_numpy(arena).to(dev)
    d_plain = torch.zeros(len(arena), dtype=torch.uint8, device=dev)
    d_foff, d_poff = (torch.zeros(slots, dtype=torch.int64, device=dev) for _ in range(2))
    d_flen, d_st = (torch.zeros(slots, dtype=torch.int32, device=dev) for _ in range(2))
    d_fl = torch.zeros(slots, dtype=torch.uint8, device=dev)
    d_res = torch.zeros((S, 4), dtype=torch.int64, device=dev)
    d_dst = t(S + np.arange(D), np.uint32, np.int32)
    out_bytes = live * (L + 33 + 9)
    d_out = torch.zeros(out_bytes, dtype=torch.uint8, device=dev)
    d_dres = torch.zeros((D, 4), dtype=torch.int64, device=dev)
    d_fwd = torch.zeros((S, 4), dtype=torch.int64, device=dev)
    # (a): one route a source
    idx_a, N_a = np.arange(S + 1, dtype=np.uint32), S * K
    poff_a = torch.zeros(N_a + 1, dtype=torch.int64, device=dev)
    pst_a = torch.zeros(N_a, dtype=torch.int32, device=dev)
    # (b): every destination a source, and the table on the device
    idx_b, dst_b, N_b = np.arange(S + 1, dtype=np.uint32) * D, np.tile(np.arange(D, dtype=np.uint32), S), S * K * D
    poff_b = torch.zeros(N_b + 1, dtype=torch.int64, device=dev)
    pst_b = torch.zeros(N_b, dtype=torch.int32, device=dev)
    d_match = torch.zeros(N_b, dtype=torch.uint8, device=dev)
    s_idx, s_off = t(table[0], np.uint32, np.int32), t(table[1], np.uint64, np.int64)
    s_len, s_raw = t(table[2], np.uint32, np.int32), t(table[3], np.uint8, np.uint8)

    def static():
        ctx.forward_zmtp_multi(d_sid, d_off, d_len, d_in, -1, K, d_foff, d_flen, d_poff, d_plain, d_fl, d_st, d_res,
                               d_dst, idx_a, route, d_out, poff_a, pst_a, d_dres, d_fwd)

    def subs():
        ctx.forward_zmtp_sub_multi(d_sid, d_off, d_len, d_in, -1, K, d_foff, d_flen, d_poff, d_plain, d_fl, d_st,
                                   d_res, d_dst, idx_b, dst_b, d_out, poff_b, pst_b, d_dres, d_fwd, s_idx, s_off,
                                   s_len, s_raw, match_out=d_match)

    def timed(fn):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    fns = dict(static=static, subs=subs)
    for _ in range(o.warmup):
        for fn in fns.values():
            timed(fn)
    us = {k: [] for k in fns}
    for _ in range(o.rounds):
        for k, fn in fns.items():
            us[k].append(timed(fn))
    # both forms forwarded everything, to the same destinations, into the same bytes
    reset()
    static()
    torch.cuda.synchronize()
    one = d_out.cpu().numpy().copy()
    res_a = ctx.zmtp_send_results(d_dres)
    assert [f["forwarded"] for f in ctx.forward_results(d_fwd)] == [K] * S
    d_out.zero_()
    reset()  # (the send counters too: both forms seal with the same nonces)
    subs()
    torch.cuda.synchronize()
    assert [f["forwarded"] for f in ctx.forward_results(d_fwd)] == [K] * S
    m = d_match.cpu().numpy().reshape(S, K, D)
    assert int(m.sum()) == live and (m.argmax(2) == route[:, None]).all()
    assert ctx.zmtp_send_results(d_dres) == res_a and (d_out.cpu().numpy() == one).all()
    sid, commit = C.build_id()
    line = dict(tool="forward_sub_bench",
                shape=dict(streams=S, frames=K, payload=L, dst=D, prefixes_per_dst=P, pairs_static=N_a, pairs_subs=N_b,
                           live_pairs=live, in_bytes=int(sum(len(x) for x in streams))),
                rounds=o.rounds, warmup=o.warmup,
                static_us=dict(median=float(np.median(us["static"])), min=float(min(us["static"]))),
                subs_us=dict(median=float(np.median(us["subs"])), min=float(min(us["subs"]))),
                device=torch.cuda.get_device_name(0), hip=torch.version.hip, source_id=sid, commit=commit)
    print(json.dumps(line))
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
