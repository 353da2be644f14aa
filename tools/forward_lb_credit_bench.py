#!/usr/bin/env python3
"""What high-water marks cost the load balancer on one MI355X (a measurement,
not a gate), on tools/forward_bench.py's workload: 256 source connections with
16 single-part messages of 1 KiB each, one group of 16 destinations (4,096
pairs, all live).

  (a) framed     zmqg_forward_framed_multi, ZMQG_FWD_LB, ZMTP on both sides
                 (the call without high-water marks, unchanged)
  (b) unlimited  zmqg_forward_lb_credit_multi on the same input with every
                 credit ZMQG_CREDIT_UNLIMITED: one epoch, nothing deactivated
  (c) half       the same with eight of the destinations at half of their
                 even share: they run out halfway, one after the other, and
                 the other eight take the rest (nine epochs)

(a) and (b) write the same `out`; the tool compares them, and checks (c)'s
counts.  Each round is bracketed by stream events; before the first event of a
round the sessions are installed again, peer nonces and send counters at their
start, and the cursor is set to 0.  --warmup rounds of each, then --rounds timed
ones, alternating.  Prints one JSON line: the medians and minima in
microseconds, the shape, the device and the library's source id; --out also
writes it to a file.  --once FORM runs one round of one form and nothing else
(for a kernel trace)."""
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
    ap.add_argument("--once", choices=["framed", "unlimited", "half"])
    ap.add_argument("--out")
    o = ap.parse_args()
    S, K, L, D = o.streams, o.frames, o.payload, o.dst
    assert D % 2 == 0 and (S * K) % (2 * D) == 0
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(S + D)]
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
    d_sid, d_off = t(np.arange(S), np.uint32, np.int32), t(offs, np.uint64, np.int64)
    d_len, d_in = t([len(x) for x in streams], np.uint32, np.int32), torch.from_numpy(arena).to(dev)
    d_plain = torch.zeros(len(arena), dtype=torch.uint8, device=dev)
    d_foff, d_poff = (torch.zeros(slots, dtype=torch.int64, device=dev) for _ in range(2))
    d_flen, d_st = (torch.zeros(slots, dtype=torch.int32, device=dev) for _ in range(2))
    d_fl = torch.zeros(slots, dtype=torch.uint8, device=dev)
    d_res = torch.zeros((S, 4), dtype=torch.int64, device=dev)
    d_dst = t(S + np.arange(D), np.uint32, np.int32)
    d_out = torch.zeros(slots * (L + 33 + 9), dtype=torch.uint8, device=dev)
    d_dres = torch.zeros((D, 4), dtype=torch.int64, device=dev)
    d_fwd = torch.zeros((S, 4), dtype=torch.int64, device=dev)
    pair_off = torch.zeros(slots + 1, dtype=torch.int64, device=dev)
    pair_st = torch.zeros(slots, dtype=torch.int32, device=dev)
    d_dest = torch.zeros(slots, dtype=torch.int32, device=dev)
    plan = dict(flags=0, stream_group=np.zeros(S, np.uint32), grp_idx=t([0, D], np.uint32, np.int32),
                lb_dst=t(np.arange(D), np.uint32, np.int32), lb_cur=d_cur, dest_out=d_dest)
    share = slots // D
    half = [share // 2 if d % 2 else C.CREDIT_UNLIMITED for d in range(D)]  # the odd destinations run out
    want = [share // 2 if d % 2 else share + share // 2 for d in range(D)]
    cr_unl = t([C.CREDIT_UNLIMITED] * D, np.uint32, np.int32)
    cr_half = t(half, np.uint32, np.int32)
    d_taken, d_dropped = (torch.zeros(D, dtype=torch.int32, device=dev) for _ in range(2))
    common = (d_sid, d_off, d_len, d_in, -1, K, d_foff, d_flen, d_poff, d_plain, d_fl, d_st, d_res, d_dst)
    outs = (d_out, pair_off, pair_st, d_dres, d_fwd)
    fr = (C.FRAMING_ZMTP, C.FRAMING_ZMTP)

    def framed():
        ctx.forward_framed_multi(*fr, C.FWD_LB, *common, None, None, *outs, **plan)

    def unlimited():
        ctx.forward_lb_credit_multi(*fr, cr_unl, d_taken, d_dropped, *common, *outs, **plan)

    def halved():
        ctx.forward_lb_credit_multi(*fr, cr_half, d_taken, d_dropped, *common, *outs, **plan)

    def timed(fn):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    fns = dict(framed=framed, unlimited=unlimited, half=halved)
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
    # (a) and (b): the same bytes, results, statuses, choices and cursor; (c): the counts
    u32 = lambda x: [int(v) for v in x.cpu().numpy().view(np.uint32)]
    reset()
    framed()
    torch.cuda.synchronize()
    one, res_a, st_a = d_out.cpu().numpy().copy(), ctx.zmtp_send_results(d_dres), pair_st.cpu().numpy().copy()
    dest_a, cur_a = u32(d_dest), u32(d_cur)
    assert [f["forwarded"] for f in ctx.forward_results(d_fwd)] == [K] * S
    assert dest_a == [p % D for p in range(slots)] and cur_a == [slots % D]
    d_out.zero_()
    reset()
    unlimited()
    torch.cuda.synchronize()
    assert ctx.zmtp_send_results(d_dres) == res_a and (d_out.cpu().numpy() == one).all()
    assert (pair_st.cpu().numpy() == st_a).all() and u32(d_dest) == dest_a and u32(d_cur) == cur_a
    assert u32(d_taken) == [share] * D and u32(d_dropped) == [0] * D
    reset()
    halved()
    torch.cuda.synchronize()
    assert u32(d_taken) == want and u32(d_dropped) == [0] * D and u32(cr_half) == half
    assert [x["frames"] for x in ctx.zmtp_send_results(d_dres)] == want
    assert int((pair_st.cpu().numpy() != 0).sum()) == 0
    sid, commit = C.build_id()
    stat = lambda k: dict(median=float(np.median(us[k])), min=float(min(us[k])))
    line = dict(tool="forward_lb_credit_bench",
                shape=dict(streams=S, frames=K, payload=L, dst=D, groups=1, pairs=slots, live_pairs=slots,
                           finite_destinations=D // 2, credit_each=share // 2,
                           in_bytes=int(sum(len(x) for x in streams))),
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
