// curve_forward.hpp -- the plan between the receive side and the send side of
// zmqg_forward_zmtp_multi: which decoded parts go on, and to whom.
//
// A broker's steady state is "decrypt a frame from connection A, encrypt the
// same bytes for B" (zmq_proxy, src/proxy.cpp:90-138).  The decode has left
// every fact the decision needs on the device -- statuses, the MORE / COMMAND
// bits, the frame counts -- so the decision is made there, and the encode's
// descriptors are written where the encode reads them.
//
// Source stream s has the sequence Q(s): its carried parts (held back by an
// earlier call), then its returned frames.  Parts reach the reader only as
// whole messages (pipe_t::write, src/pipe.cpp:222-234), commands never
// (src/stream_engine_base.cpp:635-637), and nothing from the first failing
// frame on (pipe_t::rollback, src/pipe.cpp:236-247):
//
//   F(s)        the first returned frame with a non-zero status, or |Q(s)|
//   E(s)        the last element below F(s) that is no command and has MORE
//               clear, or -1
//   held_first  E(s) + 1; the non-command elements below it are forwarded
//
//   k_fwd_scan   one wave per source stream, 64 elements a step: F and E from
//                ballots (the lowest failing lane, the highest closing lane
//                below it), the forwarded count from popcounts -> fwd[s]
//   k_fwd_pairs  one lane per pair (element q of stream s, its k-th route):
//                the stream by a search of the base table, then the encode's
//                frame_stream / flags / in_off / len; a pair whose element is
//                not forwarded names no stream, so the encode skips it
//
// The host arrays of the call (the bases, carry_idx, route_idx, route_dst)
// arrive as one table of 32-bit words: [3][n_streams + 1], then the routes.
// zmqg_forward_zmtp_sub_multi adds a fourth row, the element bases, and two
// kernels between the scan and the pairs (curve_fwd_match.hpp).
// zmqg_forward_zmtp_router_multi has the same fourth row, the heads, a lookup
// of every head's address and a pairs kernel of its own (curve_fwd_route.hpp).
// zmqg_forward_zmtp_lb_multi has the fourth row too, behind the table
// stream_group and the group-to-streams lists, the heads with the messages'
// ranks, the groups' ring positions and a pairs kernel of its own
// (curve_fwd_lb.hpp).
#pragma once

#include <stdint.h>

namespace zmqg {

constexpr uint32_t kFwdThreads = 256; // k_fwd_scan: 4 waves, a stream each

// Element q of stream s (carry first): its flags, and whether it is a returned
// frame that failed.
__device__ __forceinline__ uint32_t fwd_element(uint64_t q, uint32_t c0, uint32_t c, uint64_t slot0,
                                                const uint8_t *__restrict__ carry_flags,
                                                const uint8_t *__restrict__ flags_out,
                                                const int32_t *__restrict__ status_out, bool &bad)
{
    bad = false;
    if (q < c)
        return carry_flags[c0 + q];
    const uint64_t j = slot0 + (q - c);
    bad = status_out[j] != 0;
    return flags_out[j];
}

__global__ __launch_bounds__(kFwdThreads) void k_fwd_scan(uint32_t n_streams, uint64_t max_frames,
                                                         const uint32_t *__restrict__ cidx,
                                                         const uint8_t *__restrict__ carry_flags,
                                                         const uint8_t *__restrict__ flags_out,
                                                         const int32_t *__restrict__ status_out,
                                                         const zmqg_zmtp_result *__restrict__ results,
                                                         zmqg_forward_result *__restrict__ fwd)
{
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * (kFwdThreads / 64u) + (threadIdx.x >> 6);
    if (s >= n_streams)
        return; // (the whole wave)
    const uint32_t c0 = cidx[s], c = cidx[s + 1] - c0;
    uint64_t frames = results[s].frames;
    frames = frames < max_frames ? frames : max_frames;
    const uint64_t seq = c + frames, slot0 = (uint64_t) s * max_frames;
    uint64_t held_first = 0, forwarded = 0, data = 0; // data: non-command elements before this step
    int32_t failed = 0;
    for (uint64_t q0 = 0; q0 < seq; q0 += 64u) {
        const uint64_t q = q0 + lane;
        const bool in = q < seq;
        bool bad = false;
        const uint32_t fl = in ? fwd_element(q, c0, c, slot0, carry_flags, flags_out, status_out, bad) : 0u;
        const uint64_t badm = __builtin_amdgcn_ballot_w64(bad);
        const uint64_t below = badm ? (1ull << __builtin_ctzll(badm)) - 1ull : ~0ull; // the lanes below F
        const bool part = in && !(fl & ZMQG_MSG_COMMAND);
        const uint64_t partm = __builtin_amdgcn_ballot_w64(part) & below;
        const uint64_t lastm = __builtin_amdgcn_ballot_w64(part && !(fl & ZMQG_MSG_MORE)) & below;
        if (lastm) {
            const uint32_t e = 63u - (uint32_t) __builtin_clzll(lastm);
            held_first = q0 + e + 1u;
            forwarded = data + (uint64_t) __builtin_popcountll(partm & ((2ull << e) - 1ull));
        }
        data += (uint64_t) __builtin_popcountll(partm);
        if (badm) {
            failed = 1;
            break;
        }
    }
    if (lane == 0) {
        zmqg_forward_result r{};
        r.seq = seq;
        r.held_first = held_first;
        r.forwarded = forwarded;
        r.failed = failed;
        fwd[s] = r;
    }
}

// base[s] = the first pair of stream s, base[n_streams] = n.  Streams without
// pairs share their successor's base: the pair's stream is the last one whose
// base is not above it.
// kSubs (zmqg_forward_zmtp_sub_multi, curve_fwd_match.hpp): a forwarded pair is
// live only when its destination is subscribed to its message's topic, the byte
// match[] holds at the pair index of the message's head (head[ebase[s] + q]),
// and match_out, when asked for, says which pairs are live.
template <bool kSubs>
__global__ __launch_bounds__(256) void k_fwd_pairs(
    uint32_t n, uint32_t n_streams, uint64_t max_frames, const uint32_t *__restrict__ base,
    const uint32_t *__restrict__ cidx, const uint32_t *__restrict__ ridx, const uint32_t *__restrict__ rdst,
    const uint64_t *__restrict__ carry_off, const uint32_t *__restrict__ carry_len,
    const uint8_t *__restrict__ carry_flags, const uint64_t *__restrict__ plain_off,
    const uint32_t *__restrict__ frame_len, const uint8_t *__restrict__ flags_out,
    const zmqg_forward_result *__restrict__ fwd, uint32_t *__restrict__ p_stream, uint8_t *__restrict__ p_flags,
    uint64_t *__restrict__ p_off, uint32_t *__restrict__ p_len, const uint32_t *__restrict__ ebase,
    const uint32_t *__restrict__ head, const uint8_t *__restrict__ match, uint8_t *__restrict__ match_out)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n)
        return;
    uint32_t lo = 0, hi = n_streams; // base[lo] <= p < base[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (base[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    const uint32_t s = lo, r0 = ridx[s], d = ridx[s + 1] - r0; // (d > 0: the stream has pairs)
    const uint32_t c0 = cidx[s], c = cidx[s + 1] - c0;
    const uint32_t r = p - base[s], q = r / d, k = r - q * d;
    uint32_t fl, len;
    uint64_t off;
    bool live = q < fwd[s].held_first;
    if (q < c) {
        fl = carry_flags[c0 + q];
        off = carry_off[c0 + q];
        len = carry_len[c0 + q];
    } else {
        const uint64_t j = (uint64_t) s * max_frames + (q - c);
        fl = flags_out[j];
        off = plain_off[j];
        len = frame_len[j] - 33u; // (a forwarded frame has status 0: a box and a flags byte)
    }
    live = live && !(fl & ZMQG_MSG_COMMAND);
    if (kSubs) {
        // (head[] and match[] are written for forwarded elements and their heads only)
        live = live && match[(uint64_t) base[s] + (uint64_t) head[ebase[s] + q] * d + k] != 0;
        if (match_out)
            match_out[p] = live ? 1 : 0;
    }
    p_stream[p] = live ? rdst[r0 + k] : kZsendNoSession;
    p_flags[p] = live ? (uint8_t) (fl & ZMQG_MSG_MORE) : 0;
    p_off[p] = live ? off : 0;
    p_len[p] = live ? len : 0u;
}

} // namespace zmqg
