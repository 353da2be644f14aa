// curve_fwd_common.hpp -- what the four forward calls' plans share, included
// first by their headers: the table of a call's host arrays, its builder and its
// search (also compiled for the host as C++11, tests/host/test_fwd_tables.cpp),
// and on the device the source sequences, the slots of a pair space with id
// parts, the pairs' epilogue and the wave's inclusive sum.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <string.h>

#include "../../include/zmqg_curve.h"

#if defined(__HIPCC__)
#define ZMQG_FWD_FN __host__ __device__ inline
#else
#define ZMQG_FWD_FN inline
#endif

namespace zmqg {

// the limit of every count of the C ABI: 2^31 - 1
inline int check_n(uint64_t n)
{
    return n > 0x7fffffffull ? -EINVAL : 0;
}

// table[0 .. n] rises from 0 and i < table[n]: the last s with table[s] <= i.
// Streams without items share their successor's entry, and the search passes
// them over.
template <class T, class I>
__attribute__((always_inline)) ZMQG_FWD_FN uint32_t fwd_stream_of(const T *table, uint32_t n, I i)
{
    uint32_t lo = 0, hi = n; // table[lo] <= i < table[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) / 2u; // (n <= 2^31 - 1: no wrap)
        if (table[mid] <= i)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------
// The table: a forward call's host arrays as one block of 32-bit words, staged
// and copied to the device once, where every pair and element searches it.
//
//   [rows][S + 1]   base   base[s] = the first pair of stream s, base[S] = N.
//                          Stream s owns m * (c(s) + MF) * d'(s) pairs, p =
//                          base[s] + slot * d'(s) + k: c(s) its carried parts,
//                          d'(s) its routes, or 1 with one_route; m = 2 when an
//                          id part goes in front of every element (slot 2q + 1
//                          is element q, slot 2q the id part), else 1
//                   cidx   carry_idx, or zeros
//                   ridx   route_idx, or s with one_route
//                   ebase  (rows == 4: with_ebase) ebase[s] = the first element
//                          of stream s among the c(s) + MF elements of the
//                          streams that have routes, ebase[S] = EN
//   [R]             route_dst (R = 0 with one_route)
//   the load balancer's, when stream_group is given:
//   [S]             stream_group
//   [G + 1], [SG]   gidx, gstr: the streams of every group, rising within a
//                   group, as an index and a list (SG: the streams with a group)
struct FwdTableIn {
    const zmqg_forward_zmtp *a; // n_streams (S), max_frames (MF), n_dst, carry_idx, route_idx, route_dst
    bool one_route;             // ROUTE and the load balancer: d'(s) = 1, route_idx / route_dst not read
    bool with_ebase;
    uint32_t m;
    const uint32_t *stream_group; // [S], each below n_groups or ZMQG_LB_NO_GROUP; null: no load balancer
    uint64_t n_groups;
    uint64_t c(uint64_t s) const { return a->carry_idx ? a->carry_idx[s + 1] - a->carry_idx[s] : 0u; }
    uint64_t d(uint64_t s) const { return one_route ? 1u : a->route_idx[s + 1] - a->route_idx[s]; }
};

struct FwdTableDims {
    uint64_t N, EN, R, SG, rows, words;
};

// The arrays' own checks (rising from 0, every route below n_dst, a stream's
// pairs and their sum within 2^31 - 1) and the sizes; -EINVAL, or 0.
inline int fwd_table_dims(const FwdTableIn &in, FwdTableDims &t)
{
    const zmqg_forward_zmtp &a = *in.a;
    const uint64_t S = a.n_streams;
    if ((!in.one_route && (!a.route_idx || a.route_idx[0] != 0)) || (a.carry_idx && a.carry_idx[0] != 0))
        return -EINVAL;
    FwdTableDims d = {0, 0, 0, 0, in.with_ebase ? 4u : 3u, 0};
    for (uint64_t s = 0; s < S; ++s) {
        if ((!in.one_route && a.route_idx[s + 1] < a.route_idx[s]) ||
            (a.carry_idx && a.carry_idx[s + 1] < a.carry_idx[s]))
            return -EINVAL;
        const uint64_t ds = in.d(s), e = in.c(s) + a.max_frames, q = in.m * e; // (q below 2^34)
        if (ds && q > 0x7fffffffull / ds)
            return -EINVAL;
        d.N += q * ds;
        if (check_n(d.N))
            return -EINVAL;
        if (ds)
            d.EN += e; // (at most N)
        d.SG += in.stream_group && in.stream_group[s] != ZMQG_LB_NO_GROUP;
    }
    d.R = in.one_route ? 0u : a.route_idx[S];
    if (d.R > 0 && !a.route_dst)
        return -EINVAL;
    for (uint64_t i = 0; i < d.R; ++i)
        if (a.route_dst[i] >= a.n_dst)
            return -EINVAL;
    d.words = d.rows * (S + 1) + d.R + (in.stream_group ? S + (in.n_groups + 1) + d.SG : 0u);
    t = d;
    return 0;
}

// Where the rows lie in a block of t.words words (the host's or the device's,
// there a kernel argument by value); the load balancer's begin at rdst.
struct FwdTab {
    uint32_t *base, *cidx, *ridx, *ebase, *rdst;
};

inline FwdTab fwd_tab(uint32_t *w, uint64_t S, const FwdTableDims &t)
{
    return FwdTab{w, w + (S + 1), w + 2 * (S + 1), w + 3 * (S + 1), w + t.rows * (S + 1)};
}

// Fills w[0 .. t.words) for arrays that fwd_table_dims accepted.
inline void fwd_table_fill(const FwdTableIn &in, const FwdTableDims &t, uint32_t *w)
{
    const zmqg_forward_zmtp &a = *in.a;
    const uint64_t S = a.n_streams, G = in.n_groups;
    const FwdTab h = fwd_tab(w, S, t);
    if (in.stream_group) { // a counting sort of the streams by group
        uint32_t *sgrp = h.rdst, *gidx = sgrp + S, *gstr = gidx + (G + 1);
        memcpy(sgrp, in.stream_group, 4 * (size_t) S);
        memset(gidx, 0, 4 * (size_t) (G + 1));
        for (uint64_t s = 0; s < S; ++s) // counts, one slot up
            if (sgrp[s] != ZMQG_LB_NO_GROUP && sgrp[s] + 1u < G)
                ++gidx[sgrp[s] + 2u];
        for (uint64_t g = 2; g <= G; ++g) // gidx[g + 1] = the first stream of group g
            gidx[g] += gidx[g - 1];
        for (uint64_t s = 0; s < S; ++s) // gidx[g + 1] walks up to the end of group g
            if (sgrp[s] != ZMQG_LB_NO_GROUP)
                gstr[gidx[sgrp[s] + 1u]++] = (uint32_t) s;
    }
    uint32_t b = 0, eb = 0;
    for (uint64_t s = 0; s <= S; ++s) {
        h.base[s] = b;
        h.cidx[s] = a.carry_idx ? a.carry_idx[s] : 0u;
        h.ridx[s] = in.one_route ? (uint32_t) s : a.route_idx[s];
        if (in.with_ebase)
            h.ebase[s] = eb;
        if (s < S) {
            const uint64_t e = in.c(s) + a.max_frames, ds = in.d(s);
            b += (uint32_t) (in.m * e * ds); // (N <= 2^31 - 1)
            if (ds)
                eb += (uint32_t) e;
        }
    }
    if (t.R)
        memcpy(h.rdst, a.route_dst, 4 * (size_t) t.R);
}

#if defined(__HIPCC__)

constexpr uint32_t kFwdThreads = 256;  // the wave-per-item kernels: 4 waves, an item each
constexpr uint32_t kFwdTopicWin = 256; // bytes of a topic or an address staged in LDS
constexpr uint32_t kFwdNoHead = 0xffffffffu;
constexpr uint32_t kFwdNoStream = 0xffffffffu; // kZsendNoSession (curve_zmtp_send.hpp): the encode skips the frame

// The source sequences.  Q(s) is stream s's carried parts cidx[s] .. cidx[s + 1]
// of the carry arrays, then its returned frames, slots s * max_frames + i of
// the decode's outputs; a frame's payload is its box without the tag and the
// flags byte, frame_len - 33.  fwd[s] is k_fwd_scan's answer.
struct FwdSrc {
    uint32_t n_streams;
    uint64_t max_frames;
    const uint32_t *__restrict__ cidx;
    const uint64_t *__restrict__ carry_off;
    const uint32_t *__restrict__ carry_len;
    const uint8_t *__restrict__ carry_flags;
    const uint64_t *__restrict__ plain_off;
    const uint32_t *__restrict__ frame_len;
    const uint8_t *__restrict__ flags_out;
    const int32_t *__restrict__ status_out;
    const zmqg_forward_result *__restrict__ fwd;
};

struct FwdElem {
    uint32_t flags;
    uint64_t off; // the payload, in `plain`
    uint32_t len;
};

// Element q of Q(s).  (The length is right for a frame with status 0: every
// frame below held_first.)
__device__ __forceinline__ FwdElem fwd_elem(const FwdSrc &src, uint32_t s, uint64_t q)
{
    const uint32_t c0 = src.cidx[s], c = src.cidx[s + 1] - c0;
    if (q < c)
        return FwdElem{src.carry_flags[c0 + q], src.carry_off[c0 + q], src.carry_len[c0 + q]};
    const uint64_t j = (uint64_t) s * src.max_frames + (q - c);
    return FwdElem{src.flags_out[j], src.plain_off[j], src.frame_len[j] - 33u};
}

// Its flags alone, for the kernels that walk whole sequences and load c0 and c
// (as above) once, ahead of the walk; *bad (when asked for): it is a returned
// frame that failed
__device__ __forceinline__ uint32_t fwd_elem_flags(const FwdSrc &src, uint32_t s, uint32_t c0, uint32_t c, uint64_t q,
                                                   bool *bad = nullptr)
{
    if (q < c)
        return src.carry_flags[c0 + q];
    const uint64_t j = (uint64_t) s * src.max_frames + (q - c);
    if (bad)
        *bad = src.status_out[j] != 0;
    return src.flags_out[j];
}

// A slot of a pair space: element q, or with `twice` the id part in front of it.
struct FwdSlot {
    uint32_t q;
    bool id_slot;
};

__device__ __forceinline__ FwdSlot fwd_slot(uint32_t slot, bool twice)
{
    return FwdSlot{twice ? slot >> 1 : slot, twice && !(slot & 1u)};
}

// The id part of stream s: the peer's routing id, with MORE set by definition
__device__ __forceinline__ FwdElem fwd_id_part(const uint64_t *__restrict__ src_id_off,
                                               const uint32_t *__restrict__ src_id_len, uint32_t s)
{
    return FwdElem{ZMQG_MSG_MORE, src_id_off[s], src_id_len[s]};
}

// The encode's frame per pair: its stream, MORE bit, payload.  A pair that is
// not live names no stream, so the encode skips it.
struct FwdPairsOut {
    uint32_t *__restrict__ p_stream;
    uint8_t *__restrict__ p_flags;
    uint64_t *__restrict__ p_off;
    uint32_t *__restrict__ p_len;
};

__device__ __forceinline__ void fwd_store_pair(const FwdPairsOut &out, uint32_t p, bool live, uint32_t dest,
                                               const FwdElem &el)
{
    out.p_stream[p] = live ? dest : kFwdNoStream;
    out.p_flags[p] = live ? (uint8_t) (el.flags & ZMQG_MSG_MORE) : 0;
    out.p_off[p] = live ? el.off : 0;
    out.p_len[p] = live ? el.len : 0u;
}

// The inclusive sum of x over the wave's lanes up to this one
__device__ __forceinline__ uint64_t wave_incl_sum_u64(uint64_t x, uint32_t lane)
{
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint64_t up = __shfl_up((unsigned long long) x, o, 64);
        if (lane >= o)
            x += up;
    }
    return x;
}

#endif // __HIPCC__

} // namespace zmqg
