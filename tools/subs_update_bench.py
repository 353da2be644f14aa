#!/usr/bin/env python3
"""zmqg_subs_update_multi on one MI355X (a measurement, not a gate), two parts.

  (1) update   one round of the call: a store of 1024 destinations x cap 64 x
               slot_bytes 64 with 16 prefixes held each; 256 streams of 4
               commands (a new subscription, a cancel of a held prefix, a
               duplicate, a cancel of a prefix nobody holds).  Before the first
               event of a round the store is copied back from its start state.
  (2) forward  tools/forward_sub_bench.py's subscription workload (256 sources
               x 16 messages of 1 KiB, every source routed to all 16
               destinations, 16 prefixes a destination), once with the table
               the host builds and once with the view this call has published
               from a store it filled from SUBSCRIBE commands.  Both write the
               same `out`; the tool compares every output.

Each round is bracketed by stream events; --warmup rounds, then --rounds timed
ones (part 2 alternating).  Prints one JSON line: medians and minima in
microseconds, the shapes, the device and the library's source id; --out also
writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libzmq_amd import curve as C  # noqa: E402
from tests import forward_model as F  # noqa: E402
from tests import subs_update_model as U  # noqa: E402

dev = torch.device("cuda", 0)


def t(a, dt, vt):
    return torch.from_numpy(np.ascontiguousarray(a, dt).view(vt)).to(dev)


def timed(fn, before):
    before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def stats(us):
    return dict(median=float(np.median(us)), min=float(min(us)))


def update_inputs(streams, MF):
    """The decode call's outputs for hand-made subscription traffic, and this call's per-slot outputs."""
    recv = U.craft(streams, MF)
    S, n = len(streams), len(streams) * MF
    res = np.array([[r["frames"], 0, 0, 0] for r in recv["results"]], np.uint64)
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=dev)
    return [t(res, np.uint64, np.int64), t(recv["f_len"], np.uint32, np.int32), t(recv["f_off"], np.uint64, np.int64),
            t(recv["flags"], np.uint8, np.uint8), t(recv["status"].astype(np.uint32), np.uint32, np.int32),
            t(recv["out"], np.uint8, np.uint8), z(n, torch.int32), z(n, torch.int64), z(n, torch.int32),
            z(n, torch.uint8), z(n, torch.int32), torch.zeros((S, 4), dtype=torch.int64, device=dev)]


def part_update(ctx, o):
    D, cap, sb, held, S = o.store_dst, o.cap, o.slot_bytes, o.held, o.update_streams
    name = lambda d, i: b"feed/%05d/%03d/" % (d, i)
    start = U.store_of([[name(d, i) for i in range(held)] for d in range(D)], cap, sb)
    store = C.CurveContext.subs_store(D, cap, sb, dev)
    first = {k: t(start[k], dt, vt) for k, dt, vt in (("cnt", np.uint32, np.int32), ("slot_len", np.uint32, np.int32),
                                                       ("bytes", np.uint8, np.uint8))}
    sub, can = (lambda p: (0, b"\x01" + p, 0)), (lambda p: (C.COMMAND, b"\x06CANCEL" + p, 0))
    dst = (np.arange(S, dtype=np.uint32) * 3) % D  # (distinct: D is no multiple of 3)
    streams = [[sub(name(d, held)), can(name(d, 0)), sub(name(d, held - 1)), can(name(d, 999))] for d in dst]
    args = update_inputs(streams, 4)

    def reset():
        for k, v in first.items():
            store[k].copy_(v)

    fn = lambda: ctx.subs_update_multi(store, dst, 4, *args)
    for _ in range(o.warmup):
        timed(fn, reset)
    us = [timed(fn, reset) for _ in range(o.rounds)]
    torch.cuda.synchronize()
    assert C.CurveContext.subs_results(args[-1]) == [dict(seen=4, changed=2, notes=3, rejected=0)] * S
    assert list(args[6].cpu().numpy()[:4]) == [C.SUB_ADDED, C.SUB_REMOVED, C.SUB_DUPLICATE, C.SUB_NOT_FOUND]
    idx = store["sub_idx"].cpu().numpy()
    assert int(idx[-1]) == D * held and (np.diff(idx) == held).all()
    return dict(shape=dict(dst=D, cap=cap, slot_bytes=sb, held_per_dst=held, streams=S, commands_per_stream=4),
                us=stats(us))


def part_forward(ctx_of, o):
    S, K, L, D, P = o.streams, o.frames, o.payload, o.dst, o.prefixes
    rng = np.random.default_rng(11)
    precoms = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(S + D)]
    route = np.arange(S, dtype=np.uint32) % D
    topic = lambda d: b"feed/%04d/" % d
    body = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for _ in range(K)]
    parts = [[(0, (topic(d) + b)[:L]) for b in body] for d in range(D)]
    streams = [b"".join(F.source_frames(precoms[s], parts[int(route[s])])) for s in range(S)]
    arena, offs = F.arena_of(streams)
    prefixes = [[b"feed/%04d/" % (1000 + 100 * d + i) for i in range(P - 1)] + [topic(d)] for d in range(D)]
    ctx = ctx_of(S + D)
    # the host-built table, and the view published from a store that SUBSCRIBE commands have filled
    table = C.CurveContext.forward_subs_table(prefixes)
    host = (t(table[0], np.uint32, np.int32), t(table[1], np.uint64, np.int64), t(table[2], np.uint32, np.int32),
            t(table[3], np.uint8, np.uint8), len(table[1]), len(table[3]))
    store = C.CurveContext.subs_store(D, P, 16, dev)
    ctx.subs_update_multi(store, np.arange(D), P, *update_inputs(
        [[(C.COMMAND, b"\x09SUBSCRIBE" + p, 0) for p in d] for d in prefixes], P))
    torch.cuda.synchronize()
    assert [sorted(d) for d in C.CurveContext.subs_store_view(store, view=True)] == [sorted(d) for d in prefixes]
    view = (store["sub_idx"], store["sub_off"], store["sub_len"], store["bytes"], D * P, D * P * 16)

    sid_all = np.arange(S + D, dtype=np.uint32)
    d_precom = torch.from_numpy(np.frombuffer(b"".join(precoms), np.uint8).copy()).to(dev)
    reset = lambda: ctx.session_set_batch(sid_all, d_precom, C.SERVER_PREFIX, C.CLIENT_PREFIX,
                                          peer_nonce=np.full(S + D, 2, np.uint64))
    slots, N = S * K, S * K * D
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=dev)
    d_sid, d_off = t(np.arange(S), np.uint32, np.int32), t(offs, np.uint64, np.int64)
    d_len, d_in = t([len(x) for x in streams], np.uint32, np.int32), torch.from_numpy(arena).to(dev)
    d_plain, d_foff, d_poff = z(len(arena), torch.uint8), z(slots, torch.int64), z(slots, torch.int64)
    d_flen, d_st, d_fl = z(slots, torch.int32), z(slots, torch.int32), z(slots, torch.uint8)
    d_res, d_dres, d_fwd = z((S, 4), torch.int64), z((D, 4), torch.int64), z((S, 4), torch.int64)
    d_dst, d_out = t(S + np.arange(D), np.uint32, np.int32), z(slots * (L + 33 + 9), torch.uint8)
    idx, dst = np.arange(S + 1, dtype=np.uint32) * D, np.tile(np.arange(D, dtype=np.uint32), S)
    poff, pst, d_match = z(N + 1, torch.int64), z(N, torch.int32), z(N, torch.uint8)

    def forward(tab):
        return lambda: ctx.forward_zmtp_sub_multi(d_sid, d_off, d_len, d_in, -1, K, d_foff, d_flen, d_poff, d_plain,
                                                  d_fl, d_st, d_res, d_dst, idx, dst, d_out, poff, pst, d_dres, d_fwd,
                                                  tab[0], tab[1], tab[2], tab[3], n_subs=tab[4], sub_bytes_len=tab[5],
                                                  match_out=d_match)

    fns = dict(host_table=forward(host), published_view=forward(view))
    for _ in range(o.warmup):
        for fn in fns.values():
            timed(fn, reset)
    us = {k: [] for k in fns}
    for _ in range(o.rounds):
        for k, fn in fns.items():
            us[k].append(timed(fn, reset))
    outs = {}
    for k, fn in fns.items():
        d_out.zero_()
        reset()  # (the send counters too: both seal with the same nonces)
        fn()
        torch.cuda.synchronize()
        assert [f["forwarded"] for f in ctx.forward_results(d_fwd)] == [K] * S
        outs[k] = [x.cpu().numpy().copy() for x in (d_out, poff, pst, d_match, d_dres, d_fwd, d_plain)]
    assert int(outs["host_table"][3].sum()) == slots
    assert all((a == b).all() for a, b in zip(outs["host_table"], outs["published_view"]))
    ctx.close()
    return dict(shape=dict(streams=S, frames=K, payload=L, dst=D, prefixes_per_dst=P, pairs=N, live_pairs=slots),
                host_table_us=stats(us["host_table"]), published_view_us=stats(us["published_view"]),
                outputs_equal=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store-dst", type=int, default=1024)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--slot-bytes", type=int, default=64)
    ap.add_argument("--held", type=int, default=16)
    ap.add_argument("--update-streams", type=int, default=256)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--payload", type=int, default=1024)
    ap.add_argument("--dst", type=int, default=16)
    ap.add_argument("--prefixes", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    o = ap.parse_args()
    ctx = C.CurveContext(0, 1)
    update = part_update(ctx, o)
    ctx.close()
    forward = part_forward(lambda n: C.CurveContext(0, n), o)
    sid, commit = C.build_id()
    line = dict(tool="subs_update_bench", rounds=o.rounds, warmup=o.warmup, update=update, forward=forward,
                device=torch.cuda.get_device_name(0), hip=torch.version.hip, source_id=sid, commit=commit)
    print(json.dumps(line))
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
