// curve_subs.hpp -- zmqg_subs_update_multi: the XPUB subscription store kept on
// the device.  What xpub_t::xread_activated does with the SUBSCRIBE / CANCEL
// traffic of its pipes (src/xpub.cpp:72-170: generic_mtrie_t::add / rm,
// src/generic_mtrie_impl.hpp:41-126, 376-521) and xpub_t::xpipe_terminated with
// a pipe that has gone (src/xpub.cpp:253-277), over a flat store by destination
// -- `cap` slots of `slot_bytes` each -- instead of a trie: the trie's answer to
// add / rm of one pipe is "does this pipe hold exactly these bytes, and how many
// pipes do", and that is what is computed, one slot a lane.
//
// An event is a cleared slot (event k * cap + i: slot i of clear_dst[k]) or a
// slot of the decode call (event EC + s * max_frames + j, EC = n_clear * cap);
// that order is the replay order the upstream verdicts are defined in.
//
//   k_subs_classify  one wave per stream, 64 slots a step: the stream's elements
//                    end at its first failing slot (a ballot); each element is
//                    classified (subs_classify) and its topic located; every
//                    per-slot output gets its value for "no subscription element"
//   k_subs_holders   one workgroup per event, before anything changes the store:
//                    H0 = the live slots of all destinations that hold the
//                    event's topic (subs_slot_equal: the length, then eight
//                    bytes a step), sixteen lanes a destination
//   k_subs_apply     one wave per stream walks its commands in order over its
//                    destination's slab -- the lanes compare a slot each, a
//                    ballot gives the hit, an add appends at cnt, a remove moves
//                    the last slot into the hole -- and writes each command's
//                    status and delta (+1 / -1 / 0); one wave per cleared
//                    destination records its slots and empties it
//   k_subs_resolve   one wave per event: H = H0 + the deltas of the earlier
//                    events with the same topic; the upstream verdict from it
//   k_subs_publish   one workgroup per destination: the exclusive sum of cnt up
//                    to it, then its entries of the view
//
// No destination is edited by two waves (stream_dst and clear_dst are distinct
// and disjoint, checked by the host), and nothing is handed from workgroup to
// workgroup within a launch: what a kernel reads of another's is behind a
// kernel boundary.  subs_classify and subs_slot_equal also compile for the host
// (tests/host/test_subs.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZMQG_SUBS_FN __host__ __device__ inline
#else
#define ZMQG_SUBS_FN inline
#endif

namespace zmqg {

// (the header's ZMQG_SUB_*, ZMQG_SUBS_* and ZMQG_MSG_* values, restated:
// zmqg_curve.hip asserts that they agree)
constexpr int32_t kSubNone = 0, kSubAdded = 1, kSubDuplicate = 2, kSubRemoved = 3, kSubNotFound = 4, kSubFull = 5,
                  kSubTooLong = 6;
constexpr uint32_t kSubsVerbose = 2u, kSubsVerboser = 4u;
constexpr uint32_t kSubsMsgCommand = 2u, kSubsMsgSubscribe = 12u, kSubsMsgCancel = 16u;
constexpr uint32_t kSubsNoNote = 0xffffffffu;

// What the engine and XPUB make of one decoded element, payload p[0 .. len) with
// msg_t flags `flags`: ZMQG_MSG_SUBSCRIBE, ZMQG_MSG_CANCEL or 0 (no subscription
// element); skip = where the topic starts in p.  A command is one by its name
// (zmtp_engine_t::process_command_message, src/zmtp_engine.cpp:533-563;
// msg_t::command_body, src/msg.cpp:526-559), a message by its first byte
// (src/xpub.cpp:95-99).  Reads at most p[0 .. min(len, 10)).
ZMQG_SUBS_FN uint32_t subs_classify(const uint8_t *p, uint32_t len, uint32_t flags, uint32_t &skip)
{
    skip = 0;
    if (flags & kSubsMsgCommand) {
        static const uint8_t sub[10] = {9, 'S', 'U', 'B', 'S', 'C', 'R', 'I', 'B', 'E'};
        static const uint8_t can[7] = {6, 'C', 'A', 'N', 'C', 'E', 'L'};
        if (len >= 10u) {
            bool eq = true;
            for (uint32_t i = 0; i < 10u; ++i)
                eq = eq && p[i] == sub[i];
            if (eq) {
                skip = 10u;
                return kSubsMsgSubscribe;
            }
        }
        if (len >= 7u) {
            bool eq = true;
            for (uint32_t i = 0; i < 7u; ++i)
                eq = eq && p[i] == can[i];
            if (eq) {
                skip = 7u;
                return kSubsMsgCancel;
            }
        }
        return 0u;
    }
    if (len >= 1u && p[0] <= 1u) {
        skip = 1u;
        return p[0] ? kSubsMsgSubscribe : kSubsMsgCancel;
    }
    return 0u;
}

// Does a[0 .. a_len) equal b[0 .. b_len)?  The lengths first, then eight bytes a
// step (at any alignment), then single bytes; no byte at or past a length is
// read, and none at all when the lengths differ.
ZMQG_SUBS_FN bool subs_slot_equal(const uint8_t *a, uint32_t a_len, const uint8_t *b, uint32_t b_len)
{
    if (a_len != b_len)
        return false;
    uint32_t i = 0;
    uint64_t x, y;
    for (; i + 8u <= a_len; i += 8u) {
        __builtin_memcpy(&x, a + i, 8);
        __builtin_memcpy(&y, b + i, 8);
        if (x != y)
            return false;
    }
    for (; i < a_len; ++i)
        if (a[i] != b[i])
            return false;
    return true;
}

// the store read as the contract reads it: never trusted
ZMQG_SUBS_FN uint32_t subs_clamp(uint32_t v, uint64_t lim)
{
    return v < lim ? v : (uint32_t) lim;
}

#if defined(__HIPCC__)

constexpr uint32_t kSubsThreads = 256; // 4 waves: a stream, an event or a cleared destination each

struct SubsStore {
    uint64_t n_dst, cap, slot_bytes;
    uint32_t *cnt;      // [n_dst]
    uint32_t *slot_len; // [n_dst * cap]
    uint8_t *bytes;     // [n_dst * cap * slot_bytes]
};

struct SubsResult { // zmqg_subs_result
    unsigned long long seen, changed, notes, rejected;
};

__global__ __launch_bounds__(kSubsThreads) void k_subs_classify(
    uint32_t n_streams, uint64_t max_frames, const zmqg_zmtp_result *__restrict__ results,
    const uint32_t *__restrict__ frame_len, const uint64_t *__restrict__ plain_off,
    const uint8_t *__restrict__ flags_out, const int32_t *__restrict__ status_out, const uint8_t *__restrict__ plain,
    int32_t *__restrict__ sub_status, uint64_t *__restrict__ topic_off, uint32_t *__restrict__ topic_len,
    uint8_t *__restrict__ note_flags, uint32_t *__restrict__ note_stream, int8_t *__restrict__ delta)
{
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * (kSubsThreads / 64u) + (threadIdx.x >> 6);
    if (s >= n_streams)
        return; // (the whole wave)
    const uint64_t slot0 = (uint64_t) s * max_frames;
    const uint64_t fr = results[s].frames, frames = fr < max_frames ? fr : max_frames;
    bool ended = false; // a slot before this step has failed: the connection ends there
    for (uint64_t j0 = 0; j0 < max_frames; j0 += 64u) { // (uniform)
        const uint64_t j = j0 + lane, k = slot0 + j;
        const bool in = j < frames && !ended;
        const uint64_t badm = __builtin_amdgcn_ballot_w64(in && status_out[k] != 0);
        const bool elem = in && (badm == 0 || lane < (uint32_t) __builtin_ctzll(badm));
        uint32_t kind = 0, skip = 0, len = 0;
        uint64_t off = 0;
        if (elem && frame_len[k] >= 33u) { // (a frame with status 0 has its 33 bytes)
            len = frame_len[k] - 33u;
            off = plain_off[k];
            kind = subs_classify(plain + off, len, flags_out[k], skip);
        }
        if (j < max_frames) {
            sub_status[k] = kSubNone;
            topic_off[k] = kind ? off + skip : 0u;
            topic_len[k] = kind ? len - skip : 0u;
            note_flags[k] = (uint8_t) kind;
            note_stream[k] = kSubsNoNote;
            delta[k] = 0;
        }
        ended = ended || badm != 0;
    }
}

// The topic of event e: a cleared slot's bytes and length, or a command's.
// cleared_cnt: clear_cnt once k_subs_apply has emptied the cleared destinations,
// nullptr before (their counts are the store's then).  false: the event is none
// (a NONE slot, a slot at or past the cleared destination's count).
__device__ __forceinline__ bool subs_event_topic(uint64_t e, uint64_t ec, const SubsStore &st,
                                                 const uint32_t *clear_dst, const uint32_t *cleared_cnt,
                                                 const uint8_t *note_flags, const uint64_t *topic_off,
                                                 const uint32_t *topic_len, const uint8_t *plain,
                                                 const uint8_t *&topic, uint32_t &len)
{
    if (e < ec) {
        const uint64_t k = e / st.cap, i = e % st.cap;
        const uint32_t t = clear_dst[k];
        if (i >= (cleared_cnt ? cleared_cnt[k] : subs_clamp(st.cnt[t], st.cap)))
            return false;
        const uint64_t g = (uint64_t) t * st.cap + i;
        topic = st.bytes + g * st.slot_bytes;
        len = subs_clamp(st.slot_len[g], st.slot_bytes); // (a clear leaves the slots as they are)
        return true;
    }
    const uint64_t k = e - ec;
    if (!note_flags[k])
        return false;
    topic = plain + topic_off[k];
    len = topic_len[k];
    return true;
}

// One workgroup per event (e = blockIdx.y * gridDim.x + blockIdx.x), sixteen
// lanes a destination: a store of many destinations with few prefixes each and
// one of few destinations with many both keep the lanes busy.
__global__ __launch_bounds__(kSubsThreads) void k_subs_holders(
    uint64_t n_events, uint64_t ec, SubsStore st, const uint32_t *__restrict__ clear_dst,
    const uint8_t *__restrict__ note_flags, const uint64_t *__restrict__ topic_off,
    const uint32_t *__restrict__ topic_len, const uint8_t *__restrict__ plain, uint32_t *__restrict__ h0)
{
    __shared__ uint32_t s_part[kSubsThreads / 64u];
    const uint64_t e = (uint64_t) blockIdx.y * gridDim.x + blockIdx.x;
    if (e >= n_events)
        return; // (the whole workgroup)
    const uint8_t *topic = nullptr;
    uint32_t len = 0, n = 0;
    if (subs_event_topic(e, ec, st, clear_dst, nullptr, note_flags, topic_off, topic_len, plain, topic, len) &&
        len <= st.slot_bytes) { // (uniform over the workgroup)
        for (uint64_t t = threadIdx.x >> 4; t < st.n_dst; t += kSubsThreads / 16u) {
            const uint32_t c = subs_clamp(st.cnt[t], st.cap);
            for (uint32_t i = threadIdx.x & 15u; i < c; i += 16u) {
                const uint64_t g = t * st.cap + i;
                n += subs_slot_equal(st.bytes + g * st.slot_bytes, subs_clamp(st.slot_len[g], st.slot_bytes), topic, len);
            }
        }
    }
    for (uint32_t o = 32u; o; o >>= 1)
        n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63u) == 0)
        s_part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        n = 0;
        for (uint32_t i = 0; i < kSubsThreads / 64u; ++i)
            n += s_part[i];
        h0[e] = n;
    }
}

// Waves [0, n_streams): stream s's commands over destination stream_dst[s].
// Waves [n_streams, n_streams + n_clear): cleared destination clear_dst[k].
// The slab is written and read by different lanes of the one wave: a wavefront
// fence between a command's writes and the next command's reads.
__global__ __launch_bounds__(kSubsThreads) void k_subs_apply(
    uint32_t n_streams, uint64_t max_frames, uint32_t n_clear, uint64_t ec, SubsStore st,
    const uint32_t *__restrict__ stream_dst, const uint32_t *__restrict__ clear_dst,
    const uint8_t *__restrict__ note_flags, const uint64_t *__restrict__ topic_off,
    const uint32_t *__restrict__ topic_len, const uint8_t *__restrict__ plain, int32_t *__restrict__ sub_status,
    int8_t *__restrict__ delta, SubsResult *__restrict__ results_out, uint32_t *__restrict__ clear_cnt,
    uint32_t *__restrict__ clear_len)
{
    const uint32_t lane = threadIdx.x & 63u, w = blockIdx.x * (kSubsThreads / 64u) + (threadIdx.x >> 6);
    if (w >= n_streams + n_clear)
        return; // (the whole wave)
    if (w >= n_streams) {
        const uint32_t k = w - n_streams, t = clear_dst[k];
        const uint32_t c = subs_clamp(st.cnt[t], st.cap);
        for (uint64_t i = lane; i < st.cap; i += 64u) {
            const uint64_t g = (uint64_t) t * st.cap + i;
            if (i < c)
                clear_len[g] = subs_clamp(st.slot_len[g], st.slot_bytes);
            delta[(uint64_t) k * st.cap + i] = i < c ? -1 : 0;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // (cnt is read above by every lane)
        if (lane == 0) {
            clear_cnt[k] = c;
            st.cnt[t] = 0;
        }
        return;
    }
    const uint32_t s = w, t = stream_dst[s];
    const uint64_t g0 = (uint64_t) t * st.cap, slot0 = (uint64_t) s * max_frames;
    uint32_t c = subs_clamp(st.cnt[t], st.cap); // (uniform, as everything below but the compares and copies)
    unsigned long long seen = 0, changed = 0, rejected = 0;
    for (uint64_t j = 0; j < max_frames; ++j) {
        const uint64_t k = slot0 + j;
        const uint32_t kind = note_flags[k];
        if (!kind)
            continue;
        ++seen;
        const uint8_t *topic = plain + topic_off[k];
        const uint32_t len = topic_len[k];
        int32_t status;
        int8_t d = 0;
        if (len > st.slot_bytes) {
            status = kind == kSubsMsgSubscribe ? kSubTooLong : kSubNotFound;
        } else {
            uint32_t hit = 0xffffffffu; // the first slot that holds the topic
            for (uint32_t i0 = 0; i0 < c && hit == 0xffffffffu; i0 += 64u) {
                const uint32_t i = i0 + lane;
                bool eq = false;
                if (i < c)
                    eq = subs_slot_equal(st.bytes + (g0 + i) * st.slot_bytes,
                                         subs_clamp(st.slot_len[g0 + i], st.slot_bytes), topic, len);
                const uint64_t m = __builtin_amdgcn_ballot_w64(eq);
                if (m)
                    hit = i0 + (uint32_t) __builtin_ctzll(m);
            }
            if (kind == kSubsMsgSubscribe) {
                if (hit != 0xffffffffu) {
                    status = kSubDuplicate;
                } else if (c >= st.cap) {
                    status = kSubFull;
                } else {
                    uint8_t *dst = st.bytes + (g0 + c) * st.slot_bytes;
                    for (uint32_t b = lane; b < len; b += 64u)
                        dst[b] = topic[b];
                    if (lane == 0)
                        st.slot_len[g0 + c] = len;
                    ++c;
                    status = kSubAdded;
                    d = 1;
                }
            } else if (hit == 0xffffffffu) {
                status = kSubNotFound;
            } else {
                const uint32_t last = c - 1u;
                if (hit != last) { // the last slot into the hole
                    const uint32_t ll = subs_clamp(st.slot_len[g0 + last], st.slot_bytes);
                    const uint8_t *src = st.bytes + (g0 + last) * st.slot_bytes;
                    uint8_t *dst = st.bytes + (g0 + hit) * st.slot_bytes;
                    for (uint32_t b = lane; b < ll; b += 64u)
                        dst[b] = src[b];
                    if (lane == 0)
                        st.slot_len[g0 + hit] = ll;
                }
                --c;
                status = kSubRemoved;
                d = -1;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        }
        changed += d != 0;
        rejected += status == kSubFull || status == kSubTooLong;
        if (lane == 0) {
            sub_status[k] = status;
            delta[ec + k] = d;
        }
    }
    if (lane == 0) {
        st.cnt[t] = c;
        results_out[s] = SubsResult{seen, changed, 0ull, rejected}; // (notes: k_subs_resolve adds them)
    }
}

__global__ __launch_bounds__(kSubsThreads) void k_subs_resolve(
    uint64_t n_events, uint64_t ec, uint64_t max_frames, uint32_t flags, SubsStore st,
    const uint32_t *__restrict__ clear_dst, const uint32_t *__restrict__ clear_cnt,
    const uint8_t *__restrict__ note_flags, const uint64_t *__restrict__ topic_off, const uint32_t *__restrict__ topic_len,
    const uint8_t *__restrict__ plain, const int32_t *__restrict__ sub_status, const int8_t *__restrict__ delta,
    const uint32_t *__restrict__ h0, uint32_t *__restrict__ note_stream, uint8_t *__restrict__ clear_note,
    SubsResult *__restrict__ results_out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t e = (uint64_t) blockIdx.x * (kSubsThreads / 64u) + (threadIdx.x >> 6);
    if (e >= n_events)
        return; // (the whole wave)
    const uint8_t *topic = nullptr;
    uint32_t len = 0;
    if (!subs_event_topic(e, ec, st, clear_dst, clear_cnt, note_flags, topic_off, topic_len, plain, topic, len))
        return;
    // the earlier events that changed a destination's hold on this topic
    int32_t sum = 0;
    for (uint64_t f0 = 0; f0 < e; f0 += 64u) { // (uniform)
        const uint64_t f = f0 + lane;
        const uint8_t *ft = nullptr;
        uint32_t fl = 0;
        if (f < e && delta[f] != 0 &&
            subs_event_topic(f, ec, st, clear_dst, clear_cnt, note_flags, topic_off, topic_len, plain, ft, fl) &&
            subs_slot_equal(ft, fl, topic, len))
            sum += delta[f];
    }
    for (uint32_t o = 32u; o; o >>= 1)
        sum += __shfl_xor(sum, o, 64);
    const int64_t H = (int64_t) h0[e] + sum;
    const bool verbose = flags & (kSubsVerbose | kSubsVerboser), verboser = flags & kSubsVerboser;
    if (e < ec) { // a cleared prefix: an unsubscription when nobody else holds it (xpipe_terminated)
        if (lane == 0)
            clear_note[(uint64_t) clear_dst[e / st.cap] * st.cap + e % st.cap] = verboser || H == 1;
        return;
    }
    const uint64_t k = e - ec;
    const int32_t status = sub_status[k];
    // first_added; last_value_removed; and rm_result != values_remain also for not_found (src/xpub.cpp:118-126)
    const bool note = status == kSubAdded       ? verbose || H == 0
                      : status == kSubDuplicate ? verbose
                      : status == kSubRemoved   ? verboser || H == 1
                                                : status == kSubNotFound;
    if (note && lane == 0) {
        note_stream[k] = 0;
        atomicAdd(&results_out[k / max_frames].notes, 1ull);
    }
}

// Block t: destination t's entries of the view; block n_dst - 1 also the total.
// With n_dst == 0 one block writes sub_idx[0].
__global__ __launch_bounds__(kSubsThreads) void k_subs_publish(SubsStore st, uint32_t *__restrict__ sub_idx,
                                                              uint64_t *__restrict__ sub_off,
                                                              uint32_t *__restrict__ sub_len)
{
    __shared__ uint32_t s_part[kSubsThreads / 64u];
    const uint32_t t = blockIdx.x, lane = threadIdx.x & 63u;
    if (st.n_dst == 0) {
        if (threadIdx.x == 0)
            sub_idx[0] = 0;
        return;
    }
    uint32_t sum = 0; // (n_dst * cap <= 2^31 - 1)
    for (uint32_t u = threadIdx.x; u < t; u += kSubsThreads)
        sum += subs_clamp(st.cnt[u], st.cap);
    for (uint32_t o = 32u; o; o >>= 1)
        sum += __shfl_xor(sum, o, 64);
    if (lane == 0)
        s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t i = 0; i < kSubsThreads / 64u; ++i)
        base += s_part[i];
    const uint32_t c = subs_clamp(st.cnt[t], st.cap);
    if (threadIdx.x == 0) {
        sub_idx[t] = base;
        if (t + 1u == st.n_dst)
            sub_idx[t + 1u] = base + c;
    }
    for (uint32_t i = threadIdx.x; i < c; i += kSubsThreads) {
        const uint64_t g = (uint64_t) t * st.cap + i;
        sub_off[base + i] = g * st.slot_bytes;
        sub_len[base + i] = subs_clamp(st.slot_len[g], st.slot_bytes);
    }
}

#endif // __HIPCC__

} // namespace zmqg
