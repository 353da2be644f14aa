// curve_fwd_credit.hpp -- zmqg_forward_credit_multi's pass between a forward
// call's plan and its send side: per-destination high-water marks, counted in
// whole messages as the reference counts them (pipe_t::check_hwm,
// src/pipe.cpp:535-541; _msgs_written rises on a part without MORE only,
// pipe_t::write, src/pipe.cpp:222-234, so a message is refused at its first
// part or not at all; dist_t::write, src/dist.cpp:196-210, takes a refusing
// pipe out for the rest; router_t::xsend, src/router.cpp:185-200, drops the
// message addressed to a full pipe).
//
// A delivery is one outgoing message for one destination t: (stream s, message,
// route slot k), at the pair p0 = base(s) + slot0 * d'(s) + k of the message's
// first slot.  The i-th delivery of t in pair order is admitted iff i <
// dst_credit[t]; a refused delivery's live pairs are cleared, so the send side
// skips them like any other pair that is not live.  The rank i is a keyed
// prefix count over the unsorted pairs, the shape k_zsend_* solve for bytes
// (curve_zmtp_send.hpp): tile tables with the destination as the key and 1 as
// the value, in 32-bit counts (N <= 2^31 - 1).
//
//   k_fwd_credit_tiles    per tile of T pairs: key[p] = the destination of the
//                         delivery that starts at p, or none; per-destination
//                         counts -> tab[tile][t]
//   k_fwd_credit_colblk   per destination and block of kFwdCreditRB rows: the block
//                         sum, also added to the destination's total D(t)
//   k_fwd_credit_colscan  tab[tile][t] := t's deliveries in the tiles before
//   k_fwd_credit_ranks    one workgroup per tile, a wave per 64 pairs, the waves
//                         in pair order at the LDS row of running counts:
//                         rank[p0] = tab[tile][t] + t's starts before p0 in the
//                         tile
//   k_fwd_credit_apply    one lane per pair: p0 from the element's head, the
//                         verdict from rank[p0] and dst_credit[t]; a live pair
//                         of a refused delivery is cleared and remembered
//   k_fwd_credit_totals   one lane per destination: taken, dropped, and with
//                         ZMQG_CREDIT_CONSUME the credit that is left (behind
//                         every read of the old value: a launch of its own)
//   k_fwd_credit_status   behind the send side: ZMQG_ERR_HWM for the remembered
//                         pairs (the encode's frame kernel has given them
//                         ZMQG_ERR_SESSION like every pair without a stream)
//
// Seven launches, whatever N and n_dst are (six without pair_status), and one
// more under ZMQG_FWD_STATIC, whose plan has no heads of its own: k_fwd_heads.
//
// The admit arithmetic (fwd_credit_admits, _taken, _dropped, _left) also
// compiles for the host (tests/host/test_fwd_credit.cpp).
#pragma once
#include "curve_fwd_common.hpp"

namespace zmqg {

constexpr uint32_t kFwdCreditUnlimited = ZMQG_CREDIT_UNLIMITED;
constexpr uint32_t kFwdCreditTile = 256; // pairs per count tile, until the table outgrows zsend_tile_frames' bounds

// Is the delivery of rank `rank` (from 0) among its destination's admitted?
ZMQG_FWD_FN bool fwd_credit_admits(uint32_t rank, uint32_t credit)
{
    return credit == kFwdCreditUnlimited || rank < credit;
}

// Of D deliveries the admitted ones: min(D, credit), all of them when unlimited
ZMQG_FWD_FN uint32_t fwd_credit_taken(uint32_t D, uint32_t credit)
{
    return credit == kFwdCreditUnlimited || D < credit ? D : credit;
}

// (taken <= D: no wrap)
ZMQG_FWD_FN uint32_t fwd_credit_dropped(uint32_t D, uint32_t credit)
{
    return D - fwd_credit_taken(D, credit);
}

// The credit after the call: unlimited stays, else credit - taken (taken <=
// credit: no wrap, and never the unlimited value)
ZMQG_FWD_FN uint32_t fwd_credit_left(uint32_t D, uint32_t credit)
{
    return credit == kFwdCreditUnlimited ? credit : credit - fwd_credit_taken(D, credit);
}

#if defined(__HIPCC__)

constexpr uint32_t kFwdCreditThreads = 256; // k_fwd_credit_ranks: 4 waves, 256 pairs a round
constexpr uint32_t kFwdCreditNone = 0xffffffffu;
constexpr uint32_t kFwdCreditRB = 16; // table rows per block of the column passes (kZsendRB)

// The pair space the plan was made in: twice, id slots in front of the elements
// (PREPEND alone); one_route, one route slot a stream (ROUTE); addr, the
// message's first slot is the consumed address, whose pair names no stream, and
// the destination is the head's verdict (ROUTE without PREPEND).
struct FwdCreditSpace {
    bool twice, one_route, addr;
    const uint32_t *__restrict__ head;    // e_head
    const uint32_t *__restrict__ verdict; // e_verdict (addr)
};

// Pair p as (stream, routes of the stream, slot, route slot)
struct FwdCreditPair {
    uint32_t s, d, slot, k;
};

__device__ __forceinline__ FwdCreditPair fwd_credit_pair(const FwdSrc &src, const FwdTab &tab,
                                                         const FwdCreditSpace &sp, uint32_t p)
{
    FwdCreditPair r;
    r.s = fwd_stream_of(tab.base, src.n_streams, p);
    r.d = sp.one_route ? 1u : tab.ridx[r.s + 1] - tab.ridx[r.s]; // (d > 0: the stream has pairs)
    const uint32_t i = p - tab.base[r.s];
    r.slot = i / r.d;
    r.k = i - r.slot * r.d;
    return r;
}

// The destination of the delivery that starts at pair p, or kFwdCreditNone: p
// is the first slot of a forwarded message (head[] is written below held_first,
// and a command is no head) and the plan gave the message's pairs a destination.
__device__ __forceinline__ uint32_t fwd_credit_start(const FwdSrc &src, const FwdTab &tab, const FwdCreditSpace &sp,
                                                     const uint32_t *__restrict__ p_stream, uint32_t n_dst, uint32_t p)
{
    const FwdCreditPair r = fwd_credit_pair(src, tab, sp, p);
    const FwdSlot sl = fwd_slot(r.slot, sp.twice);
    if ((sp.twice && !sl.id_slot) || sl.q >= src.fwd[r.s].held_first)
        return kFwdCreditNone;
    const uint32_t e = tab.ebase[r.s] + sl.q;
    if (sp.head[e] != sl.q)
        return kFwdCreditNone;
    const uint32_t t = sp.addr ? sp.verdict[e] : p_stream[p];
    return t < n_dst ? t : kFwdCreditNone;
}

__global__ __launch_bounds__(256) void k_fwd_credit_tiles(uint32_t n, uint32_t T, uint32_t n_dst, FwdSrc src,
                                                         FwdTab tab, FwdCreditSpace sp,
                                                         const uint32_t *__restrict__ p_stream,
                                                         uint32_t *__restrict__ key, uint32_t *__restrict__ cnt,
                                                         uint32_t *__restrict__ tot)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t credit_row[]; // [n_dst]
    if (blockIdx.x == 0) // the destinations' totals, which k_fwd_credit_colblk adds up
        for (uint32_t t = threadIdx.x; t < n_dst; t += 256)
            tot[t] = 0;
    for (uint32_t t = threadIdx.x; t < n_dst; t += 256)
        credit_row[t] = 0;
    __syncthreads();
    const uint64_t b = (uint64_t) blockIdx.x * T, e = b + T < n ? b + T : n;
    for (uint64_t i = b + threadIdx.x; i < e; i += 256) {
        const uint32_t t = fwd_credit_start(src, tab, sp, p_stream, n_dst, (uint32_t) i);
        key[i] = t;
        if (t != kFwdCreditNone)
            atomicAdd(credit_row + t, 1u);
    }
    __syncthreads();
    uint32_t *row = cnt + (size_t) blockIdx.x * n_dst;
    for (uint32_t t = threadIdx.x; t < n_dst; t += 256)
        row[t] = credit_row[t];
}

// (the rows of a block are read by independent loads, as in k_zsend_colblk)
__global__ __launch_bounds__(256) void k_fwd_credit_colblk(uint32_t tiles, uint32_t n_dst,
                                                          const uint32_t *__restrict__ cnt,
                                                          uint32_t *__restrict__ blk, uint32_t *__restrict__ tot)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x, rb = blockIdx.y;
    if (t >= n_dst)
        return;
    const uint32_t r0 = rb * kFwdCreditRB;
    uint32_t x[kFwdCreditRB];
#pragma unroll
    for (uint32_t k = 0; k < kFwdCreditRB; ++k)
        x[k] = r0 + k < tiles ? cnt[(size_t) (r0 + k) * n_dst + t] : 0u;
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < kFwdCreditRB; ++k)
        m += x[k];
    blk[(size_t) rb * n_dst + t] = m;
    if (m)
        atomicAdd(tot + t, m);
}

__global__ __launch_bounds__(256) void k_fwd_credit_colscan(uint32_t tiles, uint32_t n_dst,
                                                           uint32_t *__restrict__ cnt,
                                                           const uint32_t *__restrict__ blk)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x, rb = blockIdx.y;
    if (t >= n_dst)
        return;
    const uint32_t r0 = rb * kFwdCreditRB;
    uint32_t x[kFwdCreditRB];
#pragma unroll
    for (uint32_t k = 0; k < kFwdCreditRB; ++k)
        x[k] = r0 + k < tiles ? cnt[(size_t) (r0 + k) * n_dst + t] : 0u;
    uint32_t m = 0;
#pragma unroll 8
    for (uint32_t k = 0; k < rb; ++k)
        m += blk[(size_t) k * n_dst + t];
#pragma unroll
    for (uint32_t k = 0; k < kFwdCreditRB; ++k) {
        if (r0 + k < tiles)
            cnt[(size_t) (r0 + k) * n_dst + t] = m;
        m += x[k];
    }
}

// A wave's 64 pairs: the lanes that hold this lane's key.  Every lane compares
// its key with each lane's in turn (zsend_group's loop without the bytes).
__device__ __forceinline__ uint64_t fwd_credit_group(uint32_t key)
{
    uint64_t m = 0;
#pragma unroll 16
    for (uint32_t j = 0; j < 64; ++j) {
        const uint32_t kj = (uint32_t) __builtin_amdgcn_readlane((int) key, (int) j);
        m |= (uint64_t) (kj == key) << j;
    }
    return m;
}

// One workgroup per tile, in rounds of 256 pairs: each wave takes 64 of them,
// then the waves take their turns, in pair order, at the LDS row of running
// counts.  Lanes without a start carry a key of their own, so they match nobody.
__global__ __launch_bounds__(kFwdCreditThreads) void k_fwd_credit_ranks(uint32_t n, uint32_t T, uint32_t n_dst,
                                                                       const uint32_t *__restrict__ key,
                                                                       const uint32_t *__restrict__ cnt,
                                                                       uint32_t *__restrict__ rank)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t credit_row[]; // [n_dst] the next rank of each destination
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t *row = cnt + (size_t) blockIdx.x * n_dst;
    for (uint32_t t = threadIdx.x; t < n_dst; t += kFwdCreditThreads)
        credit_row[t] = row[t];
    __syncthreads();
    const uint64_t b = (uint64_t) blockIdx.x * T, e = b + T < n ? b + T : n;
    for (uint64_t i0 = b; i0 < e; i0 += kFwdCreditThreads) { // (a uniform trip count: barriers inside)
        const uint64_t i = i0 + threadIdx.x;
        const uint32_t t = i < e ? key[i] : kFwdCreditNone;
        const bool start = t < n_dst;
        const uint64_t mask = fwd_credit_group(start ? t : 0x80000000u | lane); // (destinations are below 8,192)
        const uint32_t before = (uint32_t) __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        const bool has_next = (mask & ~((2ull << lane) - 1ull)) != 0;
        uint32_t r = 0;
#pragma unroll 1
        for (uint32_t g = 0; g < kFwdCreditThreads / 64u; ++g) {
            if (g == wave) {
                if (start)
                    r = credit_row[t] + before;
                __builtin_amdgcn_wave_barrier(); // (every lane has read before one writes)
                if (start && !has_next) // the destination's last start of these 64
                    credit_row[t] = r + 1u;
            }
            __syncthreads();
        }
        if (start)
            rank[i] = r;
    }
}

// One lane per pair.  A live pair belongs to the delivery at p0, the first slot
// of its element's message in its own route slot; key[p0] is its destination.
__global__ __launch_bounds__(256) void k_fwd_credit_apply(uint32_t n, uint32_t n_dst, FwdSrc src, FwdTab tab,
                                                         FwdCreditSpace sp, const uint32_t *__restrict__ key,
                                                         const uint32_t *__restrict__ rank,
                                                         const uint32_t *__restrict__ credit, FwdPairsOut out,
                                                         uint8_t *__restrict__ hwm)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n)
        return;
    bool refused = false;
    if (out.p_stream[p] != kFwdNoStream) { // (live: its element is forwarded, head[] is written)
        const FwdCreditPair r = fwd_credit_pair(src, tab, sp, p);
        const uint32_t q = fwd_slot(r.slot, sp.twice).q, h = sp.head[tab.ebase[r.s] + q];
        const uint32_t p0 = tab.base[r.s] + (sp.twice ? 2u * h : h) * r.d + r.k; // (at or below p)
        const uint32_t t = key[p0];
        refused = t < n_dst && !fwd_credit_admits(rank[p0], credit[t]);
    }
    if (refused) {
        out.p_stream[p] = kFwdNoStream;
        out.p_flags[p] = 0;
        out.p_off[p] = 0;
        out.p_len[p] = 0u;
    }
    hwm[p] = refused ? 1 : 0;
}

// tot: D(t), or NULL when the call has no pairs
__global__ __launch_bounds__(256) void k_fwd_credit_totals(uint32_t n_dst, const uint32_t *__restrict__ tot,
                                                          uint32_t *__restrict__ credit,
                                                          uint32_t *__restrict__ taken,
                                                          uint32_t *__restrict__ dropped, uint32_t consume)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_dst)
        return;
    const uint32_t D = tot[t], c = credit[t];
    taken[t] = fwd_credit_taken(D, c);
    dropped[t] = fwd_credit_dropped(D, c);
    if (consume)
        credit[t] = fwd_credit_left(D, c);
}

__global__ __launch_bounds__(256) void k_fwd_credit_status(uint32_t n, const uint8_t *__restrict__ hwm,
                                                          int32_t *__restrict__ pair_status)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < n && hwm[p])
        pair_status[p] = ZMQG_ERR_HWM;
}

#endif // __HIPCC__

} // namespace zmqg
