// curve_fwd_lb_credit.hpp -- zmqg_forward_lb_credit_multi's part of the plan:
// lb_t::sendpipe (src/lb.cpp:56-131) with pipes that can be full.  A pipe whose
// check_write fails (pipe_t::check_hwm, src/pipe.cpp:535-541) is not dropped
// for: it is swapped out of the active range and the message goes to the next
// one (src/lb.cpp:103-107).  The choice of every later message moves with it, so
// the choice is made per group, in order, before the pairs are laid out.
//
// Not message by message.  Between two deactivations the ring is plain
// round-robin, so a group is a short run of epochs.  In an epoch with ring size
// A and cursor cur, position j has distance d = (j - cur) mod A and is found
// full at epoch-message index i_j = d + w[j] * A, its (w[j] + 1)-th visit; the
// i_j are distinct.  L = min i_j over the finite entries.  With rem <= L
// messages left they all go round-robin and the group is done (rem == L too:
// the full entry is only found by a later send).  Else L messages go that way,
// every finite entry loses its visits, position (cur + L) mod A is deactivated
// by the swap rule, and the next epoch starts there.  Every epoch finishes the
// group or shrinks A: at most A0 + 1 epochs on any table.
//
//   k_fwd_heads<true>      (curve_fwd_match.hpp) heads, ranks, messages a stream
//   k_fwd_lb_credit_groups one workgroup per group: the exclusive message counts
//                          of its streams; the working ring (orig, w) in LDS,
//                          or, above kFwdLbcRing entries, in ctx scratch at the
//                          group's absolute ring positions; the epochs.  In each the workgroup strides over the
//                          epoch's messages, finds (stream, rank) by a search of
//                          the exclusive counts and writes the destination, or
//                          the refused mark, at pick[ebase[s] + rank]; it strides
//                          over the ring for the visits: X(t) += visits (one
//                          atomic per entry and epoch), w -= visits.  lb_cur[g]
//                          at the end.
//   k_fwd_pairs_lb_credit  k_fwd_pairs_lb reading that slot; the byte per pair
//                          that k_fwd_credit_status turns into ZMQG_ERR_HWM
//   k_fwd_credit_totals    (curve_fwd_credit.hpp) taken, dropped, the write-back
//
// Steps per group, K deactivations, M messages, S_g streams:
// O((K + 1) * A / 256 + M * log S_g / 256).
//
// The device trusts neither the table nor, where a grp_idx that does not rise
// makes two groups' ranges overlap, its own scratch: every orig value is
// bounded before it indexes lb_dst, and the loop's trip count depends on A
// alone.  The per-entry arithmetic (fwd_lbc_*) also compiles for the host
// (tests/host/test_fwd_lb_credit.cpp).
#pragma once
#include "curve_fwd_credit.hpp"
#include "curve_fwd_lb.hpp"

namespace zmqg {

constexpr uint32_t kFwdLbRefused = 0xfffffffcu; // pick[]: every entry of the ring was deactivated
constexpr uint64_t kFwdLbNever = ~0ull;         // the full-at index of an entry that never runs out

// The distance of ring position j from the cursor (j, cur < A <= 2^31 - 1)
ZMQG_FWD_FN uint32_t fwd_lbc_dist(uint32_t j, uint32_t cur, uint32_t A)
{
    return j >= cur ? j - cur : j + (A - cur);
}

// The epoch-message index at which the entry at distance d with credit w is
// found full: its (w + 1)-th visit.  Below 2^63: w <= 2^32 - 2, A <= 2^31 - 1.
ZMQG_FWD_FN uint64_t fwd_lbc_full_at(uint32_t d, uint32_t w, uint32_t A)
{
    return w == kFwdCreditUnlimited ? kFwdLbNever : d + (uint64_t) w * A;
}

// Of an epoch's first n messages, those that go to the entry at distance d:
// indices d, d + A, ...  (n at most the entry's own full-at index, or at most
// 2^32 - 1 for an entry that never runs out: the count fits.)
ZMQG_FWD_FN uint32_t fwd_lbc_visits(uint64_t n, uint32_t d, uint32_t A)
{
    if (n <= d)
        return 0u;
    const uint64_t x = n - d - 1u;
    return (x >> 32 ? (uint32_t) (x / A) : (uint32_t) x / A) + 1u;
}

// The credit after `visits` messages (visits <= w for a finite entry)
ZMQG_FWD_FN uint32_t fwd_lbc_left(uint32_t w, uint32_t visits)
{
    return w == kFwdCreditUnlimited ? w : w - visits;
}

// lb_t's _active and _current
struct FwdLbRing {
    uint32_t A, cur;
};

// The entry at position j (< A) refused a message (src/lb.cpp:103-107):
// _active--, and when j is still below it the entries j and _active change
// places (true: the caller swaps them, R and w together) and the cursor stays on
// j, which now holds another entry; else _current = 0.
ZMQG_FWD_FN bool fwd_lbc_deactivate(FwdLbRing &r, uint32_t j)
{
    r.A -= 1u;
    if (j < r.A) {
        r.cur = j;
        return true;
    }
    r.cur = 0u;
    return false;
}

// A working ring entry's original position, bounded for the read of lb_dst
// (scratch that two overlapping groups wrote may hold anything)
ZMQG_FWD_FN uint32_t fwd_lbc_orig(uint32_t o, uint32_t A0)
{
    return o < A0 ? o : 0u;
}

#if defined(__HIPCC__)

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t x)
{
    for (uint32_t o = 32; o; o >>= 1) {
        const uint64_t y = __shfl_xor((unsigned long long) x, o, 64);
        x = y < x ? y : x;
    }
    return x;
}

constexpr uint32_t kFwdLbcRing = 512;     // ring entries a workgroup keeps in LDS; a larger ring works in ctx scratch
constexpr uint32_t kFwdLbcStreams = 1024; // streams of a group whose counts are searched in LDS; more: in memory

// One workgroup per group.  gstr[gidx[g] .. gidx[g + 1]) are the group's
// streams, rising; each one's exclusive message count and the base of its
// slots go to LDS when the group has at most kFwdLbcStreams streams, else the
// counts to excl[] (indexed like gstr).  The working ring -- every entry's
// original position, working credit and destination -- lives in LDS up to
// kFwdLbcRing entries; a larger one in orig / w (n_lb entries each, this
// group's at lo .. lo + A0), its destinations read through lb_dst.  pick: the
// element space (ebase), a slot per message at its stream's base.  X: n_dst
// counts, zero when the kernel starts.
__global__ __launch_bounds__(kFwdThreads) void k_fwd_lb_credit_groups(
    const uint32_t *__restrict__ gidx, const uint32_t *__restrict__ gstr, const uint32_t *__restrict__ msgs,
    const uint32_t *__restrict__ ebase, const uint32_t *__restrict__ grp_idx, uint32_t n_lb,
    const uint32_t *__restrict__ lb_dst, uint32_t n_dst, const uint32_t *__restrict__ credit, uint32_t *lb_cur,
    uint32_t *excl, uint32_t *orig, uint32_t *w, uint32_t *__restrict__ pick, uint32_t *X)
{
    __shared__ uint32_t s_msgs;
    __shared__ uint64_t s_min[kFwdThreads / 64u];
    __shared__ uint32_t s_excl[kFwdLbcStreams], s_base[kFwdLbcStreams];
    __shared__ uint32_t s_orig[kFwdLbcRing], s_w[kFwdLbcRing], s_dst[kFwdLbcRing];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, g = blockIdx.x;
    const FwdLbRange r = fwd_lb_range(grp_idx[g], grp_idx[g + 1], n_lb);
    const uint32_t A0 = r.A, k0 = gidx[g], nS = gidx[g + 1] - k0;
    if (A0 == 0) { // (the whole workgroup) no ring: the pairs report that themselves
        if (tid == 0)
            lb_cur[g] = 0;
        return;
    }
    const bool lds_s = nS <= kFwdLbcStreams, lds_r = A0 <= kFwdLbcRing;
    uint32_t *const xs = lds_s ? s_excl : excl + k0; // the streams' exclusive counts,
    uint32_t *const op = lds_r ? s_orig : orig + r.lo, *const wp = lds_r ? s_w : w + r.lo; // the working ring
    uint32_t cur = fwd_lb_cur0(lb_cur[g], A0);
    if (wave == 0) { // 64 streams a step (the sum is at most 2^31 - 1)
        uint32_t before = 0;
        for (uint32_t i0 = 0; i0 < nS; i0 += 64u) {
            const uint32_t i = i0 + lane;
            const bool in = i < nS;
            const uint32_t s = in ? gstr[k0 + i] : 0u, cnt = in ? msgs[s] : 0u;
            const uint32_t incl = (uint32_t) wave_incl_sum_u64(cnt, lane);
            if (in) {
                xs[i] = before + (incl - cnt);
                if (lds_s)
                    s_base[i] = ebase[s];
            }
            before += (uint32_t) __shfl((int) incl, 63, 64);
        }
        if (lane == 0)
            s_msgs = before;
    }
    for (uint32_t j = tid; j < A0; j += kFwdThreads) {
        const uint32_t t = lb_dst[(uint64_t) r.lo + j];
        op[j] = j;
        wp[j] = t < n_dst ? credit[t] : kFwdCreditUnlimited; // (names none: never runs out)
        if (lds_r)
            s_dst[j] = t < n_dst ? t : kFwdLbNoPeer;
    }
    __syncthreads();
    const uint32_t M = s_msgs;
    // message mi of the group -> its slot (the rank is below msgs[s], at most the stream's elements)
    auto store = [&](uint32_t mi, uint32_t v) {
        const uint32_t k = fwd_stream_of(xs, nS, mi);
        pick[(lds_s ? s_base[k] : ebase[gstr[k0 + k]]) + (mi - xs[k])] = v;
    };
    auto dest_at = [&](uint32_t pos) { // (pos < A <= A0)
        if (lds_r)
            return s_dst[pos];
        const uint32_t t = lb_dst[(uint64_t) r.lo + fwd_lbc_orig(op[pos], A0)];
        return t < n_dst ? t : kFwdLbNoPeer;
    };
    uint32_t A = A0, done = 0; // (A, cur, done: the same in every lane)
    for (;;) {
        const uint32_t rem = M - done;
        if (A == 0) { // every entry was deactivated: the rest is refused
            for (uint32_t i = tid; i < rem; i += kFwdThreads)
                store(done + i, kFwdLbRefused);
            cur = 0;
            break;
        }
        uint64_t m = kFwdLbNever;
        for (uint32_t j = tid; j < A; j += kFwdThreads) {
            const uint64_t f = fwd_lbc_full_at(fwd_lbc_dist(j, cur, A), wp[j], A);
            m = f < m ? f : m;
        }
        m = wave_min_u64(m);
        if (lane == 0)
            s_min[wave] = m;
        __syncthreads();
        uint64_t L = s_min[0];
        for (uint32_t k = 1; k < kFwdThreads / 64u; ++k)
            L = s_min[k] < L ? s_min[k] : L;
        const bool last = rem <= L;
        const uint32_t n = last ? rem : (uint32_t) L; // (below 2^31)
        for (uint32_t i = tid; i < n; i += kFwdThreads)
            store(done + i, dest_at(fwd_lb_at(cur, i, A)));
        for (uint32_t j = tid; j < A; j += kFwdThreads) {
            const uint32_t v = fwd_lbc_visits(n, fwd_lbc_dist(j, cur, A), A);
            if (v) {
                const uint32_t t = dest_at(j);
                if (t < n_dst)
                    atomicAdd(X + t, v);
                wp[j] = fwd_lbc_left(wp[j], v);
            }
        }
        if (last) {
            cur = fwd_lb_at(cur, rem, A);
            break;
        }
        __syncthreads(); // (the ring was read and w updated before the swap)
        const uint32_t js = fwd_lb_at(cur, L, A);
        FwdLbRing ring = {A, cur};
        if (fwd_lbc_deactivate(ring, js) && tid == 0) {
            const uint32_t b = ring.A, oa = op[js], wa = wp[js];
            op[js] = op[b], wp[js] = wp[b];
            op[b] = oa, wp[b] = wa;
            if (lds_r) {
                const uint32_t da = s_dst[js];
                s_dst[js] = s_dst[b], s_dst[b] = da;
            }
        }
        A = ring.A, cur = ring.cur, done += n;
        __syncthreads();
    }
    if (tid == 0) // the original position of the entry the working cursor points at
        lb_cur[g] = A ? fwd_lbc_orig(op[cur], A0) : 0u;
}

// k_fwd_pairs_lb with the destination read from the message's slot.  hwm[p]: the
// pair belongs to a refused message (what would be live, and the id slot).
__global__ __launch_bounds__(256) void k_fwd_pairs_lb_credit(
    uint32_t n, FwdSrc src, FwdTab tab, uint32_t prepend, const uint32_t *__restrict__ sgrp,
    const uint32_t *__restrict__ head, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ pick,
    const uint32_t *__restrict__ grp_idx, uint32_t n_lb, const uint64_t *__restrict__ src_id_off,
    const uint32_t *__restrict__ src_id_len, FwdPairsOut out, uint32_t *__restrict__ dest_out,
    uint8_t *__restrict__ hwm)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n)
        return;
    const uint32_t s = fwd_stream_of(tab.base, src.n_streams, p);
    const FwdSlot sl = fwd_slot(p - tab.base[s], prepend);
    const FwdElem el = fwd_elem(src, s, sl.q);
    const bool forwarded = sl.q < src.fwd[s].held_first && !(el.flags & ZMQG_MSG_COMMAND);
    const uint32_t e = tab.ebase[s] + sl.q;
    uint32_t dest = kFwdLbNone;
    bool refused = false;
    if (forwarded && (!sl.id_slot || head[e] == sl.q)) {
        dest = kFwdLbNoPeer;
        const uint32_t g = sgrp[s];
        if (g != kFwdLbNoGroup && fwd_lb_range(grp_idx[g], grp_idx[g + 1], n_lb).A) {
            const uint32_t v = pick[tab.ebase[s] + rank[e]];
            refused = v == kFwdLbRefused;
            dest = refused ? kFwdLbNoPeer : v;
        }
    }
    fwd_store_pair(out, p, dest < kFwdLbNoPeer, dest, sl.id_slot ? fwd_id_part(src_id_off, src_id_len, s) : el);
    if (dest_out)
        dest_out[p] = dest;
    hwm[p] = refused ? 1 : 0;
}

#endif // __HIPCC__

} // namespace zmqg
