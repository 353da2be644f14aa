#!/usr/bin/env python3
"""What the per-destination high-water marks cost on one MI355X (a measurement,
not a gate), on tools/forward_sub_bench.py's subscription workload: 256 source
connections with 16 single-part messages of 1 KiB each, every source routed to
all 16 destinations, a table of 16 prefixes per destination under which exactly
one destination matches each message (65,536 pairs, one in 16 live).

  (a) framed     zmqg_forward_framed_multi, ZMQG_FWD_SUB, ZMTP on both sides
                 (the call without high-water marks, unchanged)
  (b) unlimited  zmqg_forward_credit_multi on the same input with every credit
                 ZMQG_CREDIT_UNLIMITED: the pass runs and clears nothing
  (c) half       the same with destination 0's credit at half of its
                 deliveries: the pass clears the other half

(a) and (b) write the same `out`; the tool compares them, and checks (c)'s
counts.  Each round is bracketed by stream events; before the first event of a
round the sessions are installed again, peer nonces and send counters at their
start.  --warmup rounds of each, then --rounds timed ones, alternating.  Prints
one JSON line: the medians and minima in microseconds, the shape, the device and
the library's source id; --out also writes it to a file."""
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
    d_out = torch.zeros(live * (L + 33 + 9), dtype=torch.uint8, device=dev)
    d_dres = torch.zeros((D, 4), dtype=torch.int64, device=dev)
    d_fwd = torch.zeros((S, 4), dtype=torch.int64, device=dev)
    idx, dst, N = np.arange(S + 1, dtype=np.uint32) * D, np.tile(np.arange(D, dtype=np.uint32), S), S * K * D
    pair_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    pair_st = torch.zeros(N, dtype=torch.int32, device=dev)
    d_match = torch.zeros(N, dtype=torch.uint8, device=dev)
    plan = dict(sub_idx=t(table[0], np.uint32, np.int32), sub_off=t(table[1], np.uint64, np.int64),
                sub_len=t(table[2], np.uint32, np.int32), sub_bytes=t(table[3], np.uint8, np.uint8), match_out=d_match)
    per_dst = [int((route == d).sum()) * K for d in range(D)]  # deliveries of every destination
    half = [per_dst[0] // 2] + [C.CREDIT_UNLIMITED] * (D - 1)
    cr_unl = t([C.CREDIT_UNLIMITED] * D, np.uint32, np.int32)
    cr_half = t(half, np.uint32, np.int32)
    d_taken, d_dropped = (torch.zeros(D, dtype=torch.int32, device=dev) for _ in range(2))
    common = (d_sid, d_off, d_len, d_in, -1, K, d_foff, d_flen, d_poff, d_plain, d_fl, d_st, d_res, d_dst, idx, dst,
              d_out, pair_off, pair_st, d_dres, d_fwd)
    fr = (C.FRAMING_ZMTP, C.FRAMING_ZMTP, C.FWD_SUB)

    def framed():
        ctx.forward_framed_multi(*fr, *common, **plan)

    def unlimited():
        ctx.forward_credit_multi(*fr, cr_unl, d_taken, d_dropped, *common, **plan)

    def halved():
        ctx.forward_credit_multi(*fr, cr_half, d_taken, d_dropped, *common, **plan)

    def timed(fn):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    fns = dict(framed=framed, unlimited=unlimited, half=halved)
    for _ in range(o.warmup):
        for fn in fns.values():
            timed(fn)
    us = {k: [] for k in fns}
    for _ in range(o.rounds):
        for k, fn in fns.items():
            us[k].append(timed(fn))
    # (a) and (b): the same bytes, results, statuses; (c): destination 0 got half
    u32 = lambda x: [int(v) for v in x.cpu().numpy().view(np.uint32)]
    reset()
    framed()
    torch.cuda.synchronize()
    one, res_a, st_a = d_out.cpu().numpy().copy(), ctx.zmtp_send_results(d_dres), pair_st.cpu().numpy().copy()
    assert [f["forwarded"] for f in ctx.forward_results(d_fwd)] == [K] * S
    d_out.zero_()
    reset()
    unlimited()
    torch.cuda.synchronize()
    assert ctx.zmtp_send_results(d_dres) == res_a and (d_out.cpu().numpy() == one).all()
    assert (pair_st.cpu().numpy() == st_a).all() and u32(d_taken) == per_dst and u32(d_dropped) == [0] * D
    reset()
    halved()
    torch.cuda.synchronize()
    assert u32(d_taken) == [half[0]] + per_dst[1:] and u32(d_dropped) == [per_dst[0] - half[0]] + [0] * (D - 1)
    assert int((pair_st.cpu().numpy().view(np.uint32) == C.ERR_HWM).sum()) == per_dst[0] - half[0]
    assert ctx.zmtp_send_results(d_dres)[0]["frames"] == half[0] and u32(cr_half) == half
    sid, commit = C.build_id()
    stat = lambda k: dict(median=float(np.median(us[k])), min=float(min(us[k])))
    line = dict(tool="forward_credit_bench",
                shape=dict(streams=S, frames=K, payload=L, dst=D, prefixes_per_dst=P, pairs=N, live_pairs=live,
                           deliveries_dst0=per_dst[0], credit_dst0=half[0], in_bytes=int(sum(len(x) for x in streams))),
                rounds=o.rounds, warmup=o.warmup, framed_us=stat("framed"), unlimited_us=stat("unlimited"),
                half_us=stat("half"), device=torch.cuda.get_device_name(0), hip=torch.version.hip, source_id=sid,
                commit=commit)
    print(json.dumps(line))
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
