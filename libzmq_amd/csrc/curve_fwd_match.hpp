// curve_fwd_match.hpp -- zmqg_forward_zmtp_sub_multi's filter: which
// destinations are subscribed to which message, what xpub_t::xsend asks of its
// trie for the first part of every message (src/xpub.cpp:290-326,
// generic_mtrie_t::match, src/generic_mtrie_impl.hpp:523-561, marking pipes
// through dist_t::match, src/dist.cpp:49-62).
//
// The subscriptions are a flat table by destination: the trie's answer for one
// pipe is "some prefix of the pipe's is a prefix of the topic", and that is
// what is computed, one prefix a lane.
//
//   k_fwd_heads  one wave per source stream, 64 elements a step: for every
//                element below held_first the index in Q(s) of its message's
//                head (the first data element, and every data element whose
//                predecessor among the data elements has MORE clear), a
//                running maximum over "is a head" from ballots (and for the
//                load balancer, curve_fwd_lb.hpp, each message's rank within
//                the stream from prefix popcounts of the same ballot)
//   k_fwd_match  one wave per element; the waves of heads stay: the topic's
//                first kFwdTopicWin bytes staged in LDS; then, 64 routes a
//                round, every lane fetches its route's range of subscriptions,
//                the ranges are laid end to end by a wave scan, and the lanes
//                stride over them, 64 (route, subscription) items a step, each
//                comparing one prefix; a hit marks its route, and the lanes
//                write one byte per (head, route) at the head's pair index
//
// k_fwd_pairs (curve_forward.hpp) ANDs the byte of its element's head into
// `live`.  fwd_prefix_match, the compare of one prefix with all its range
// checks, also compiles for the host (tests/host/test_fwd_match.cpp).
#pragma once
#include "curve_fwd_common.hpp"

namespace zmqg {

// Is sub_bytes[off .. +len) a prefix of the topic?  win holds the topic's first
// min(topic_len, win_len) bytes (a staged copy); bytes at or past win_len are
// read from `topic` itself.  A subscription that does not lie within
// sub_bytes[0 .. sub_bytes_len) never matches and none of its bytes is read; no
// byte at or past topic_len is read.
ZMQG_FWD_FN bool fwd_prefix_match(const uint8_t *win, uint32_t win_len, const uint8_t *topic, uint32_t topic_len,
                                   uint64_t off, uint32_t len, const uint8_t *sub_bytes, uint64_t sub_bytes_len)
{
    if (len > topic_len)
        return false;
    if (off > sub_bytes_len || len > sub_bytes_len - off)
        return false;
    const uint8_t *p = sub_bytes + off;
    // eight bytes a step (at any alignment), then single bytes; against the
    // window up to its end, then against the topic itself (a loop each: the
    // two are different memories on the device)
    const uint32_t wl = len < win_len ? len : win_len;
    uint32_t i = 0;
    uint64_t a, b;
    for (; i + 8u <= wl; i += 8u) {
        __builtin_memcpy(&a, p + i, 8);
        __builtin_memcpy(&b, win + i, 8);
        if (a != b)
            return false;
    }
    for (; i < wl; ++i)
        if (p[i] != win[i])
            return false;
    for (; i + 8u <= len; i += 8u) {
        __builtin_memcpy(&a, p + i, 8);
        __builtin_memcpy(&b, topic + i, 8);
        if (a != b)
            return false;
    }
    for (; i < len; ++i)
        if (p[i] != topic[i])
            return false;
    return true;
}

// destination t's subscriptions [lo, hi) of a table the host cannot validate:
// entries above n_subs clamped to it, a falling pair an empty range
ZMQG_FWD_FN void fwd_sub_range(uint32_t idx_lo, uint32_t idx_hi, uint32_t n_subs, uint32_t &lo, uint32_t &hi)
{
    lo = idx_lo < n_subs ? idx_lo : n_subs;
    hi = idx_hi < n_subs ? idx_hi : n_subs;
    if (hi < lo)
        hi = lo;
}

#if defined(__HIPCC__)

constexpr uint32_t kFwdMatchThreads = 256; // k_fwd_match: 4 waves, an element each

// the highest set bit of m at or below lane l, or -1
__device__ __forceinline__ int fwd_top_at(uint64_t m, uint32_t l)
{
    m &= (2ull << l) - 1ull;
    return m ? 63 - __builtin_clzll(m) : -1;
}

// ebase[s] = the first element of stream s in `head` (streams without routes
// have none); runs behind k_fwd_scan, whose held_first bounds what is written.
// kRank (zmqg_forward_zmtp_lb_multi, curve_fwd_lb.hpp): the same ballots also
// give rank[ebase[s] + q], for forwarded data elements, the number of heads of
// the stream before its message's head, and msgs[s], the stream's heads.
template <bool kRank>
__global__ __launch_bounds__(kFwdThreads) void k_fwd_heads(FwdSrc src, FwdTab tab, uint32_t *__restrict__ head,
                                                          uint32_t *__restrict__ rank, uint32_t *__restrict__ msgs)
{
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * (kFwdThreads / 64u) + (threadIdx.x >> 6);
    if (s >= src.n_streams)
        return; // (the whole wave)
    const uint32_t e0 = tab.ebase[s];
    if (tab.ebase[s + 1] == e0) { // no routes: no pairs read it
        if (kRank && lane == 0)
            msgs[s] = 0;
        return;
    }
    const uint32_t c0 = src.cidx[s], c = src.cidx[s + 1] - c0;
    const uint64_t lim = src.fwd[s].held_first; // (below F: every frame has status 0)
    bool closed = true;          // the last data element before this step has MORE clear (or there is none)
    uint32_t last = kFwdNoHead;  // the last head before this step
    uint32_t before = 0;         // kRank: the heads before this step
    for (uint64_t q0 = 0; q0 < lim; q0 += 64u) {
        const uint64_t q = q0 + lane;
        const bool in = q < lim;
        const uint32_t fl = in ? fwd_elem_flags(src, s, c0, c, q) : 0u;
        const bool part = in && !(fl & ZMQG_MSG_COMMAND);
        const uint64_t partm = __builtin_amdgcn_ballot_w64(part);
        const uint64_t lastm = __builtin_amdgcn_ballot_w64(part && !(fl & ZMQG_MSG_MORE));
        // the data element before this lane's: in this step, or the one carried in
        const int prev = lane ? fwd_top_at(partm, lane - 1u) : -1;
        const bool is_head = part && (prev < 0 ? closed : (bool) ((lastm >> prev) & 1ull));
        const uint64_t headm = __builtin_amdgcn_ballot_w64(is_head);
        const int h = fwd_top_at(headm, lane);
        if (in)
            head[e0 + q] = h < 0 ? last : (uint32_t) (q0 + (uint32_t) h);
        if (kRank) { // (a data element has its head at or before it: the count is at least 1)
            if (part)
                rank[e0 + q] = before + (uint32_t) __builtin_popcountll(headm & ((2ull << lane) - 1ull)) - 1u;
            before += (uint32_t) __builtin_popcountll(headm);
        }
        if (partm)
            closed = (lastm >> (63 - __builtin_clzll(partm))) & 1ull;
        if (headm)
            last = (uint32_t) (q0 + (uint32_t) (63 - __builtin_clzll(headm)));
    }
    if (kRank && lane == 0)
        msgs[s] = before;
}

// One wave per element e of the element space; s by a search of ebase as
// k_fwd_pairs searches base.  match[base[s] + q * d + k] = destination
// rdst[ridx[s] + k] is subscribed to the topic of head q (negated with invert).
__global__ __launch_bounds__(kFwdMatchThreads) void k_fwd_match(
    uint32_t n_elems, FwdSrc src, FwdTab tab, const uint8_t *__restrict__ plain, const uint32_t *__restrict__ head,
    uint32_t n_subs, const uint32_t *__restrict__ sub_idx, const uint64_t *__restrict__ sub_off,
    const uint32_t *__restrict__ sub_len, const uint8_t *__restrict__ sub_bytes, uint64_t sub_bytes_len,
    uint32_t invert, uint8_t *__restrict__ match)
{
    __shared__ uint8_t s_win[kFwdMatchThreads / 64u][kFwdTopicWin];
    __shared__ uint64_t s_start[kFwdMatchThreads / 64u][64]; // a round's routes: the first item of each,
    __shared__ uint32_t s_first[kFwdMatchThreads / 64u][64]; // its first subscription,
    __shared__ uint32_t s_any[kFwdMatchThreads / 64u][64];   // and whether one of them matched
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t e = blockIdx.x * (kFwdMatchThreads / 64u) + w;
    if (e >= n_elems)
        return; // (the whole wave; no barrier below)
    const uint32_t s = fwd_stream_of(tab.ebase, src.n_streams, e), q = e - tab.ebase[s];
    if (q >= src.fwd[s].held_first || head[e] != q)
        return; // not forwarded, or no head
    const uint32_t r0 = tab.ridx[s], d = tab.ridx[s + 1] - r0;
    const FwdElem el = fwd_elem(src, s, q);
    const uint32_t tlen = el.len;
    const uint8_t *topic = plain + el.off;
    uint8_t *win = s_win[w];
    const uint32_t wlen = tlen < kFwdTopicWin ? tlen : kFwdTopicWin;
    for (uint32_t i = lane; i < wlen; i += 64u)
        win[i] = topic[i];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // (the window is the wave's own: no barrier)
    const uint64_t m0 = (uint64_t) tab.base[s] + (uint64_t) q * d;
    // 64 routes a round: lane l holds route kb + l's range of subscriptions;
    // the ranges laid end to end are the round's items, 64 of them a step
    uint64_t *start = s_start[w];
    uint32_t *first = s_first[w], *any = s_any[w];
    for (uint32_t kb = 0; kb < d; kb += 64u) {
        const uint32_t k = kb + lane;
        uint32_t j0 = 0, j1 = 0;
        if (k < d) {
            const uint32_t t = tab.rdst[r0 + k];
            fwd_sub_range(sub_idx[t], sub_idx[t + 1], n_subs, j0, j1);
        }
        const uint64_t incl = wave_incl_sum_u64(j1 - j0, lane); // (each at most 2^31 - 1)
        const uint64_t total = __shfl((unsigned long long) incl, 63, 64);
        start[lane] = incl - (j1 - j0);
        first[lane] = j0;
        any[lane] = 0;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        for (uint64_t it = 0; it < total; it += 64u) { // (uniform)
            const uint64_t item = it + lane;
            if (item < total) {
                const uint32_t a = fwd_stream_of(start, 64u, item); // (a route without items shares its successor's)
                const uint32_t j = first[a] + (uint32_t) (item - start[a]);
                if (fwd_prefix_match(win, kFwdTopicWin, topic, tlen, sub_off[j], sub_len[j], sub_bytes,
                                     sub_bytes_len))
                    any[a] = 1; // (every writer writes 1)
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (k < d)
            match[m0 + k] = (uint8_t) (any[lane] ^ invert);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // (read before the next round's writes)
    }
}

#endif // __HIPCC__

} // namespace zmqg
