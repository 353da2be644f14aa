// curve_fwd_lb.hpp -- zmqg_forward_zmtp_lb_multi's part of the plan: what lb_t
// does for a DEALER or a PUSH socket (lb_t::sendpipe, src/lb.cpp:56-131, reached
// from dealer_t::sendpipe, src/dealer.cpp:110-113, and push_t::xsend,
// src/push.cpp:45-48).  Every whole message goes to _pipes[_current], and
// ++_current wraps at _active after its last part (src/lb.cpp:118-124).
//
// A load balancer is a group: a range of lb_dst (its active pipes) and a cursor
// lb_cur[g] that lives on the device across calls.  The messages of a group are
// the forwarded messages of its streams, by rising stream, then rising element;
// the i-th of them takes ring position (cur0 + i) mod A.
//
//   k_fwd_heads<true>  (curve_fwd_match.hpp) the heads, with every message's
//                    rank within its stream and the stream's messages
//   k_fwd_lb_groups  one wave per group, 64 of its streams a step: a wave
//                    exclusive sum of the message counts -> each stream's ring
//                    position first[s], and the group's new cursor
//   k_fwd_pairs_lb   one lane per pair (the router pair space with d' = 1): its
//                    element or id slot, (first[s] + rank) mod A, a bounded read
//                    of lb_dst, the encode's frame and dest_out
//
// The host cannot validate the table, so fwd_lb_range, fwd_lb_cur0, fwd_lb_at
// and fwd_lb_pick bound every read of it; they also compile for the host
// (tests/host/test_fwd_lb.cpp).
#pragma once
#include "curve_fwd_common.hpp"

namespace zmqg {

constexpr uint32_t kFwdLbNone = ZMQG_LB_NONE, kFwdLbNoPeer = ZMQG_LB_NO_PEER, kFwdLbNoGroup = ZMQG_LB_NO_GROUP;

// Group g's active destinations lb_dst[lo .. lo + A): grp_idx entries above n_lb
// clamped to it, a falling pair an empty range.
struct FwdLbRange {
    uint32_t lo, A;
};

ZMQG_FWD_FN FwdLbRange fwd_lb_range(uint32_t idx_lo, uint32_t idx_hi, uint32_t n_lb)
{
    const uint32_t lo = idx_lo < n_lb ? idx_lo : n_lb;
    const uint32_t hi = idx_hi < n_lb ? idx_hi : n_lb;
    FwdLbRange r;
    r.lo = lo;
    r.A = hi < lo ? 0u : hi - lo;
    return r;
}

// lb_t's _current of a cursor the host may have left anywhere (the range was
// edited without reading it): cur mod A, 0 for an empty range.
ZMQG_FWD_FN uint32_t fwd_lb_cur0(uint32_t cur, uint32_t A)
{
    return A ? cur % A : 0u;
}

// The ring position `add` messages after pos (pos < A <= 2^31 - 1, add below
// 2^62: a sum of per-stream counts), in 64-bit arithmetic; 0 for an empty range.
ZMQG_FWD_FN uint32_t fwd_lb_at(uint32_t pos, uint64_t add, uint32_t A)
{
    return A ? (uint32_t) (((uint64_t) pos + add) % A) : 0u;
}

// The destination at ring position pos (< A) of the range, or kFwdLbNoPeer for
// an entry that names none (>= n_dst).  The read is lb_dst[lo + pos] with lo +
// pos < lo + A <= n_lb.
ZMQG_FWD_FN uint32_t fwd_lb_pick(const uint32_t *lb_dst, const FwdLbRange &r, uint32_t pos, uint64_t n_dst)
{
    const uint32_t t = lb_dst[(uint64_t) r.lo + pos];
    return t < n_dst ? t : kFwdLbNoPeer;
}

#if defined(__HIPCC__)

constexpr uint32_t kFwdLbPrepend = ZMQG_LB_PREPEND;

// One wave per group.  gstr[gidx[g] .. gidx[g + 1]) are the group's streams,
// rising.  first[s] = (cur0 + the group's messages before stream s) mod A, and
// lb_cur[g] = (cur0 + all of them) mod A: written for every group, so that a
// cursor is clamped whether or not the group had streams.  msgs == nullptr (a
// call without pairs): every count is 0 and first is not written.
__global__ __launch_bounds__(kFwdThreads) void k_fwd_lb_groups(uint32_t n_groups, const uint32_t *__restrict__ gidx,
                                                              const uint32_t *__restrict__ gstr,
                                                              const uint32_t *__restrict__ msgs,
                                                              const uint32_t *__restrict__ grp_idx, uint32_t n_lb,
                                                              uint32_t *__restrict__ lb_cur,
                                                              uint32_t *__restrict__ first)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * (kFwdThreads / 64u) + (threadIdx.x >> 6);
    if (g >= n_groups)
        return; // (the whole wave)
    const FwdLbRange r = fwd_lb_range(grp_idx[g], grp_idx[g + 1], n_lb);
    const uint32_t cur0 = fwd_lb_cur0(lb_cur[g], r.A);
    const uint32_t end = gidx[g + 1];
    uint64_t before = 0; // the group's messages before this step
    for (uint32_t i0 = gidx[g]; msgs && i0 < end; i0 += 64u) {
        const uint32_t i = i0 + lane;
        const bool in = i < end;
        const uint32_t s = in ? gstr[i] : 0u;
        const uint64_t cnt = in ? msgs[s] : 0u;
        const uint64_t incl = wave_incl_sum_u64(cnt, lane); // (each at most 2^31 - 1)
        if (in)
            first[s] = fwd_lb_at(cur0, before + (incl - cnt), r.A);
        before += (uint64_t) __shfl((unsigned long long) incl, 63, 64);
    }
    if (lane == 0)
        lb_cur[g] = fwd_lb_at(cur0, before, r.A);
}

// One lane per pair: one route slot a stream, id slots with prepend.  sgrp[s] is
// the stream's group (below n_groups, checked on the host) or kFwdLbNoGroup.
// Destination rule: the ring position of the element's message in its stream's
// group, an id part only in front of a head.
__global__ __launch_bounds__(256) void k_fwd_pairs_lb(
    uint32_t n, FwdSrc src, FwdTab tab, uint32_t prepend, const uint32_t *__restrict__ sgrp,
    const uint32_t *__restrict__ head, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ first,
    const uint32_t *__restrict__ grp_idx, uint32_t n_lb, const uint32_t *__restrict__ lb_dst, uint64_t n_dst,
    const uint64_t *__restrict__ src_id_off, const uint32_t *__restrict__ src_id_len, FwdPairsOut out,
    uint32_t *__restrict__ dest_out)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n)
        return;
    const uint32_t s = fwd_stream_of(tab.base, src.n_streams, p);
    const FwdSlot sl = fwd_slot(p - tab.base[s], prepend);
    const FwdElem el = fwd_elem(src, s, sl.q);
    const bool forwarded = sl.q < src.fwd[s].held_first && !(el.flags & ZMQG_MSG_COMMAND);
    // (head[] and rank[] are written for forwarded elements only)
    const uint32_t e = tab.ebase[s] + sl.q;
    uint32_t dest = kFwdLbNone;
    if (forwarded && (!sl.id_slot || head[e] == sl.q)) {
        dest = kFwdLbNoPeer;
        const uint32_t g = sgrp[s];
        if (g != kFwdLbNoGroup) {
            const FwdLbRange r = fwd_lb_range(grp_idx[g], grp_idx[g + 1], n_lb);
            if (r.A)
                dest = fwd_lb_pick(lb_dst, r, fwd_lb_at(first[s], rank[e], r.A), n_dst);
        }
    }
    fwd_store_pair(out, p, dest < kFwdLbNoPeer, dest, sl.id_slot ? fwd_id_part(src_id_off, src_id_len, s) : el);
    if (dest_out)
        dest_out[p] = dest;
}

#endif // __HIPCC__

} // namespace zmqg
