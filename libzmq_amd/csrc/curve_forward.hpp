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
//                frame_stream / flags / in_off / len
//
// The host arrays of the call reach the device as one table, and the kernels
// read the sequences through one view: curve_fwd_common.hpp.
#pragma once

#include "curve_fwd_common.hpp"

namespace zmqg {

// Result: the receive side's per-stream result, zmqg_zmtp_result or
// zmqg_ws_result; `frames` is all that is read of it.
template <class Result>
__global__ __launch_bounds__(kFwdThreads) void k_fwd_scan(FwdSrc src, const Result *__restrict__ results,
                                                         zmqg_forward_result *__restrict__ fwd)
{
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * (kFwdThreads / 64u) + (threadIdx.x >> 6);
    if (s >= src.n_streams)
        return; // (the whole wave)
    uint64_t frames = results[s].frames;
    frames = frames < src.max_frames ? frames : src.max_frames;
    const uint32_t c0 = src.cidx[s], c = src.cidx[s + 1] - c0;
    const uint64_t seq = c + frames;
    uint64_t held_first = 0, forwarded = 0, data = 0; // data: non-command elements before this step
    int32_t failed = 0;
    for (uint64_t q0 = 0; q0 < seq; q0 += 64u) {
        const uint64_t q = q0 + lane;
        const bool in = q < seq;
        bool bad = false;
        const uint32_t fl = in ? fwd_elem_flags(src, s, c0, c, q, &bad) : 0u;
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

// Destination rule: the pair's route.  kSubs (zmqg_forward_zmtp_sub_multi,
// curve_fwd_match.hpp): a forwarded pair is live only when its destination is
// subscribed to its message's topic, the byte match[] holds at the pair index
// of the message's head (head[ebase[s] + q]), and match_out, when asked for,
// says which pairs are live.
template <bool kSubs>
__global__ __launch_bounds__(256) void k_fwd_pairs(uint32_t n, FwdSrc src, FwdTab tab, FwdPairsOut out,
                                                   const uint32_t *__restrict__ head,
                                                   const uint8_t *__restrict__ match, uint8_t *__restrict__ match_out)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n)
        return;
    const uint32_t s = fwd_stream_of(tab.base, src.n_streams, p);
    const uint32_t r0 = tab.ridx[s], d = tab.ridx[s + 1] - r0; // (d > 0: the stream has pairs)
    const uint32_t r = p - tab.base[s], q = r / d, k = r - q * d;
    const FwdElem el = fwd_elem(src, s, q);
    bool live = q < src.fwd[s].held_first && !(el.flags & ZMQG_MSG_COMMAND);
    if (kSubs) {
        // (head[] and match[] are written for forwarded elements and their heads only)
        live = live && match[(uint64_t) tab.base[s] + (uint64_t) head[tab.ebase[s] + q] * d + k] != 0;
        if (match_out)
            match_out[p] = live ? 1 : 0;
    }
    fwd_store_pair(out, p, live, tab.rdst[r0 + k], el);
}

} // namespace zmqg
