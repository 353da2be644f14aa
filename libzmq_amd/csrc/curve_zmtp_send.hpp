// curve_zmtp_send.hpp -- the ZMTP encoder over many connections' send buffers
// in one call (zmqg_encode_zmtp_multi).
//
// An I/O thread's outgoing messages arrive interleaved over its connections
// (A1 B1 A2 C1 B2 ...), and every connection needs its own contiguous byte run
// for send(): what stream_engine_base_t::out_event builds per connection in
// _outpos (src/stream_engine_base.cpp:314-380: the pull loop :331, the ZMTP
// encoder :343, src/v2_encoder.cpp:23-60; up to out_batch_size bytes,
// src/options.cpp:222).  The layout is a per-stream exclusive sum of the frame
// sizes in batch order, with the streams' regions packed in stream order; the
// batch is not sorted.  It is the problem k_nonce_* solve for counts: tile
// tables, with the stream as the key and the frame's bytes F as the value.
//
//   k_zsend_tiles    per tile of T frames, per-stream byte sums -> tab[t][s]
//   k_zsend_colblk   per stream and block of kZsendRB rows: the block sum, also
//                    added to the stream's total B(s)
//   k_zsend_base     one workgroup: base(s) = the exclusive sum of B over the
//                    streams; results[s] but for the frame count;
//                    frame_off[n] = the total
//   k_zsend_colscan  tab[t][s] := base(s) + bytes of s in tiles < t
//   k_zsend_frames   one workgroup per tile, a wave per 64 frames: a frame's
//                    offset is tab[t][stream] + the bytes of the stream's
//                    earlier frames in the tile; writes frame_off, the status,
//                    the ZMTP header, and the session and body offset the
//                    encode runs with (session 0xffffffff for a frame that is
//                    invalid or does not fit: the encode neither writes it nor
//                    gives it a nonce), and counts the fitting frames in
//                    results[s] (one atomic per wave and stream)
//
// Five launches before the encode's own, whatever n and n_streams are.
//
// The two kernels that know a frame's size and header, k_zsend_tiles and
// k_zsend_frames, take the framing as a template parameter (ZsendFraming):
// ZMTP's, or the WebSocket binary frame of zmqg_encode_ws_multi, whose masked
// form adds one launch behind the encode (k_ws_mask_bodies, curve_ws.hpp).
#pragma once

#include <errno.h>
#include <stdint.h>

#include <hipcub/hipcub.hpp>

namespace zmqg {

constexpr uint32_t kZsendMaxStreams = 8192; // an LDS row of 8-byte sums: 64 KiB, a workgroup's whole LDS
constexpr uint32_t kZsendRB = 16;           // table rows per block of the column passes
constexpr uint32_t kZsendMaxTiles = 4096;
constexpr uint32_t kZsendBaseThreads = 1024;
constexpr uint32_t kZsendBaseRounds = kZsendMaxStreams / kZsendBaseThreads;
constexpr uint32_t kZsendFramesThreads = 256; // k_zsend_frames: 4 waves, 256 frames a round
constexpr uint32_t kZsendNoSession = 0xffffffffu;

// Frame i's stream when the frame is valid (a stream below n_streams whose
// session exists), with the session in sid; else kZsendNoSession.
__device__ __forceinline__ uint32_t zsend_stream(uint32_t fs, uint32_t n_streams,
                                                 const uint32_t *__restrict__ stream_sid, uint32_t max_sessions,
                                                 uint32_t &sid)
{
    sid = kZsendNoSession;
    if (fs >= n_streams)
        return kZsendNoSession;
    const uint32_t s = stream_sid[fs];
    if (s >= max_sessions)
        return kZsendNoSession;
    sid = s;
    return fs;
}

// The framing around a MESSAGE command: ZMTP's (src/v2_encoder.cpp:23-60), or
// ws_encoder_t's binary frame (src/ws_encoder.cpp:26-126) without or with a
// masking key (zmqg_encode_ws_multi).  The layout kernels are the same for
// all three: a framing sets a frame's bytes F and writes its header.
enum ZsendFraming : uint32_t { kZsendZmtp = 0, kZsendWs = 1, kZsendWsMasked = 2 };

// Bytes of a valid frame's MESSAGE command (zmqg_wire_size)
__device__ __forceinline__ uint64_t zsend_wire_bytes(uint32_t flags, uint32_t len,
                                                     const DevSession *__restrict__ sessions, uint32_t sid)
{
    const uint32_t ct = flags & 0x1cu;
    uint64_t extra = 0;
    if (ct == 12u || ct == 16u)
        extra = sessions[sid].downgrade_sub ? 1u : (ct == 12u ? 10u : 7u);
    return 32u + 1u + extra + len;
}

// Bytes of a valid frame: the header and the MESSAGE command (ZMTP:
// k_zmtp_sizes's rule; WebSocket: 2 bytes, the extended size of W + 1 -- the
// flags byte counts --, the key, the flags byte).
template <ZsendFraming FR>
__device__ __forceinline__ uint64_t zsend_frame_bytes(uint32_t flags, uint32_t len,
                                                      const DevSession *__restrict__ sessions, uint32_t sid)
{
    const uint64_t W = zsend_wire_bytes(flags, len, sessions, sid);
    if constexpr (FR == kZsendZmtp)
        return (W > 255u ? 9u : 2u) + W;
    const uint64_t size = W + 1u;
    return 2u + (size <= 125u ? 0u : size <= 0xffffu ? 2u : 8u) + (FR == kZsendWsMasked ? 4u : 0u) + size;
}

// Bytes in front of the MESSAGE command of a frame of F bytes
template <ZsendFraming FR>
__device__ __forceinline__ uint32_t zsend_header_bytes(uint64_t F)
{
    if constexpr (FR == kZsendZmtp)
        return F > 257u ? 9u : 2u;
    constexpr uint32_t m = FR == kZsendWsMasked ? 4u : 0u;
    return 2u + (F <= 2u + m + 125u ? 0u : F <= 4u + m + 0xffffu ? 2u : 8u) + m + 1u;
}

// The header of a fitting frame of F bytes at h; mask: the frame's key value
// (kZsendWsMasked), whose bytes are BE32(mask) (put_uint32, src/ws_encoder.cpp:64-69).
template <ZsendFraming FR>
__device__ __forceinline__ void zsend_write_header(uint8_t *h, uint64_t F, uint32_t hdr, uint32_t mask)
{
    const uint64_t W = F - hdr;
    if constexpr (FR == kZsendZmtp) {
        if (hdr == 2u) { // body <= 255 bytes: flags 0, one size byte
            h[0] = 0;
            h[1] = (uint8_t) W;
        } else {
            h[0] = kZmtpLarge;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                h[1 + k] = (uint8_t) (W >> (56 - 8 * k));
        }
    } else {
        constexpr uint32_t m = FR == kZsendWsMasked ? 4u : 0u;
        const uint64_t size = W + 1u;
        const uint32_t ext = hdr - 3u - m;
        h[0] = 0x82; // FIN | binary
        h[1] = (uint8_t) ((m ? 0x80u : 0u) | (ext == 0u ? (uint32_t) size : ext == 2u ? 126u : 127u));
        if (ext == 2u) {
            h[2] = (uint8_t) (size >> 8);
            h[3] = (uint8_t) size;
        } else if (ext == 8u) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                h[2 + k] = (uint8_t) (size >> (56 - 8 * k));
        }
        uint8_t *q = h + 2u + ext;
        if (m) {
            q[0] = (uint8_t) (mask >> 24);
            q[1] = (uint8_t) (mask >> 16);
            q[2] = (uint8_t) (mask >> 8);
            q[3] = (uint8_t) mask;
            q += 4;
        }
        q[0] = m ? (uint8_t) (mask >> 24) : 0; // the flags byte: 0 ^ k[0]
    }
}

template <ZsendFraming FR>
__global__ __launch_bounds__(256) void k_zsend_tiles(uint32_t n, uint32_t T, uint32_t n_streams,
                                                    const uint32_t *__restrict__ stream_sid,
                                                    const uint32_t *__restrict__ frame_stream,
                                                    const uint8_t *__restrict__ flags,
                                                    const uint32_t *__restrict__ len,
                                                    const DevSession *__restrict__ sessions, uint32_t max_sessions,
                                                    unsigned long long *__restrict__ tab,
                                                    unsigned long long *__restrict__ tot)
{
    extern __shared__ unsigned long long zsend_row[]; // [n_streams]
    if (blockIdx.x == 0) // the streams' totals, which k_zsend_colblk adds up
        for (uint32_t k = threadIdx.x; k < n_streams; k += 256)
            tot[k] = 0;
    for (uint32_t k = threadIdx.x; k < n_streams; k += 256)
        zsend_row[k] = 0;
    __syncthreads();
    const uint64_t b = (uint64_t) blockIdx.x * T, e = b + T < n ? b + T : n;
    for (uint64_t i = b + threadIdx.x; i < e; i += 256) {
        uint32_t sid;
        const uint32_t s = zsend_stream(frame_stream[i], n_streams, stream_sid, max_sessions, sid);
        if (s != kZsendNoSession)
            atomicAdd(zsend_row + s, (unsigned long long) zsend_frame_bytes<FR>(flags[i], len[i], sessions, sid));
    }
    __syncthreads();
    unsigned long long *row = tab + (size_t) blockIdx.x * n_streams;
    for (uint32_t k = threadIdx.x; k < n_streams; k += 256)
        row[k] = zsend_row[k];
}

// (the rows of a block are read by independent loads: a thread's time is one
// load's latency, not kZsendRB of them)
__global__ __launch_bounds__(256) void k_zsend_colblk(uint32_t tiles, uint32_t n_streams,
                                                     const unsigned long long *__restrict__ tab,
                                                     unsigned long long *__restrict__ blk,
                                                     unsigned long long *__restrict__ tot)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x, rb = blockIdx.y;
    if (s >= n_streams)
        return;
    const uint32_t r0 = rb * kZsendRB;
    unsigned long long x[kZsendRB];
#pragma unroll
    for (uint32_t k = 0; k < kZsendRB; ++k)
        x[k] = r0 + k < tiles ? tab[(size_t) (r0 + k) * n_streams + s] : 0ull;
    unsigned long long m = 0;
#pragma unroll
    for (uint32_t k = 0; k < kZsendRB; ++k)
        m += x[k];
    blk[(size_t) rb * n_streams + s] = m;
    if (m) // (one workgroup reading every block sum would be bound by its CU's load rate)
        atomicAdd(tot + s, m);
}

// One workgroup: the streams 1,024 at a time, thread t on stream 1024 k + t.
// tot: B(s), or NULL when the batch is empty.  results[s] is complete here
// but for the frame count: a stream whose region ends within out_bytes sends
// all of it; one that does not gets ENOBUFS, and its bytes from its first
// frame that does not fit (k_zsend_frames), or none when the region starts
// beyond out_bytes.
__global__ __launch_bounds__(kZsendBaseThreads) void k_zsend_base(
    uint32_t n_streams, const uint32_t *__restrict__ stream_sid, uint32_t max_sessions,
    const unsigned long long *__restrict__ tot, uint64_t out_bytes, unsigned long long *__restrict__ base,
    zmqg_zmtp_send_result *__restrict__ results, uint64_t *__restrict__ total_out)
{
    using Scan = hipcub::BlockScan<unsigned long long, kZsendBaseThreads>;
    __shared__ typename Scan::TempStorage tmp;
    unsigned long long B[kZsendBaseRounds];
#pragma unroll
    for (uint32_t k = 0; k < kZsendBaseRounds; ++k) {
        const uint32_t s = k * kZsendBaseThreads + threadIdx.x;
        B[k] = tot && s < n_streams ? tot[s] : 0ull;
    }
    unsigned long long carry = 0;
#pragma unroll
    for (uint32_t k = 0; k < kZsendBaseRounds; ++k) {
        if (k * kZsendBaseThreads >= n_streams)
            break;
        const uint32_t s = k * kZsendBaseThreads + threadIdx.x;
        unsigned long long before = 0, total = 0;
        Scan(tmp).ExclusiveSum(B[k], before, total);
        __syncthreads(); // (tmp is the next round's)
        if (s < n_streams) {
            const unsigned long long start = carry + before, end = start + B[k];
            base[s] = start;
            zmqg_zmtp_send_result r{};
            r.out_off = start;
            r.out_bytes = end <= out_bytes ? B[k] : 0;
            r.error = stream_sid[s] >= max_sessions ? EINVAL : B[k] > 0 && end > out_bytes ? ENOBUFS : 0;
            results[s] = r;
        }
        carry += total;
    }
    if (threadIdx.x == 0)
        *total_out = carry;
}

__global__ __launch_bounds__(256) void k_zsend_colscan(uint32_t tiles, uint32_t n_streams,
                                                      unsigned long long *__restrict__ tab,
                                                      const unsigned long long *__restrict__ blk,
                                                      const unsigned long long *__restrict__ base)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x, rb = blockIdx.y;
    if (s >= n_streams)
        return;
    const uint32_t r0 = rb * kZsendRB;
    unsigned long long x[kZsendRB];
#pragma unroll
    for (uint32_t k = 0; k < kZsendRB; ++k)
        x[k] = r0 + k < tiles ? tab[(size_t) (r0 + k) * n_streams + s] : 0ull;
    unsigned long long m = base[s];
#pragma unroll 8
    for (uint32_t k = 0; k < rb; ++k)
        m += blk[(size_t) k * n_streams + s];
#pragma unroll
    for (uint32_t k = 0; k < kZsendRB; ++k) {
        if (r0 + k < tiles)
            tab[(size_t) (r0 + k) * n_streams + s] = m;
        m += x[k];
    }
}

// A wave's 64 frames: for every lane the bytes of its stream's frames in lower
// lanes, and the lanes of its stream (mask).  Every lane compares its key with
// each lane's in turn (wave-uniform reads of one lane's key and bytes), which
// costs the same for 1 and for 64 distinct streams in the wave -- an I/O
// thread's round-robin batch has 64.  WIDE: some frame has 2^32 bytes or more.
template <bool WIDE>
__device__ __forceinline__ void zsend_group(uint32_t key, uint64_t F, uint32_t lane, uint64_t &before, uint64_t &mask)
{
    const uint32_t F_lo = (uint32_t) F, F_hi = (uint32_t) (F >> 32);
    uint64_t sum = 0, m = 0;
#pragma unroll 16
    for (uint32_t j = 0; j < 64; ++j) {
        const uint32_t kj = (uint32_t) __builtin_amdgcn_readlane((int) key, (int) j);
        uint64_t Fj = (uint32_t) __builtin_amdgcn_readlane((int) F_lo, (int) j);
        if (WIDE)
            Fj |= (uint64_t) (uint32_t) __builtin_amdgcn_readlane((int) F_hi, (int) j) << 32;
        const bool same = kj == key;
        m |= (uint64_t) same << j;
        sum += same && j < lane ? Fj : 0ull;
    }
    before = sum;
    mask = m;
}

// One workgroup per tile, in rounds of 256 frames: each wave takes 64 of them
// (loads, sizes, the in-wave sums -- the four waves side by side), then the
// waves take their turns, in frame order, at the LDS row of running offsets.
// Invalid lanes carry a key of their own, so they match nobody.  (The row is
// the workgroup's whole LDS at 8,192 streams: no other shared variable.)
// ws_key: the frames' key values (kZsendWsMasked only).
template <ZsendFraming FR>
__global__ __launch_bounds__(kZsendFramesThreads) void k_zsend_frames(
    uint32_t n, uint32_t T, uint32_t n_streams, const uint32_t *__restrict__ stream_sid,
    const uint32_t *__restrict__ frame_stream, const uint8_t *__restrict__ flags, const uint32_t *__restrict__ len,
    const uint32_t *__restrict__ ws_key,
    const DevSession *__restrict__ sessions, uint32_t max_sessions, const unsigned long long *__restrict__ tab,
    const unsigned long long *__restrict__ base, uint64_t out_bytes, uint8_t *__restrict__ out,
    uint64_t *__restrict__ frame_off, int32_t *__restrict__ status_out, uint32_t *__restrict__ enc_sid,
    uint64_t *__restrict__ wire_off, zmqg_zmtp_send_result *__restrict__ results)
{
    extern __shared__ unsigned long long zsend_row[]; // [n_streams] the next offset of each stream
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long *row = tab + (size_t) blockIdx.x * n_streams;
    for (uint32_t k = threadIdx.x; k < n_streams; k += kZsendFramesThreads)
        zsend_row[k] = row[k];
    __syncthreads();
    const uint64_t b = (uint64_t) blockIdx.x * T, e = b + T < n ? b + T : n;
    for (uint64_t i0 = b; i0 < e; i0 += kZsendFramesThreads) { // (a uniform trip count: barriers inside)
        const uint64_t i = i0 + threadIdx.x;
        uint32_t sid = kZsendNoSession, s = kZsendNoSession;
        uint64_t F = 0;
        if (i < e) {
            s = zsend_stream(frame_stream[i], n_streams, stream_sid, max_sessions, sid);
            if (s != kZsendNoSession)
                F = zsend_frame_bytes<FR>(flags[i], len[i], sessions, sid);
        }
        const bool valid = s != kZsendNoSession;
        const uint32_t key = valid ? s : 0x80000000u | lane; // (streams are below 8,192)
        uint64_t before, mask;
        if (__builtin_amdgcn_ballot_w64((F >> 32) != 0))
            zsend_group<true>(key, F, lane, before, mask);
        else
            zsend_group<false>(key, F, lane, before, mask);
        const uint64_t higher = mask & ~((2ull << lane) - 1ull); // my stream's lanes above me
        const bool has_next = higher != 0;
        const uint32_t rank = (uint32_t) __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        uint64_t off = 0;
#pragma unroll 1
        for (uint32_t g = 0; g < kZsendFramesThreads / 64u; ++g) {
            if (g == wave) {
                if (valid)
                    off = zsend_row[s] + before;
                __builtin_amdgcn_wave_barrier(); // (every lane has read before one writes)
                if (valid && !has_next) // the stream's last frame of these 64
                    zsend_row[s] = off + F;
            }
            __syncthreads();
        }
        // offsets rise within a stream: its fitting frames are a prefix
        const bool fit = valid && off + F <= out_bytes;
        const bool next_fits = __shfl((int) fit, has_next ? (int) __builtin_ctzll(higher) : (int) lane) != 0;
        if (i < e) {
            frame_off[i] = valid ? off : UINT64_MAX;
            const uint32_t hdr = zsend_header_bytes<FR>(F);
            enc_sid[i] = fit ? sid : kZsendNoSession;
            wire_off[i] = fit ? off + hdr : 0;
            if (status_out)
                status_out[i] = !valid ? ZMQG_ERR_SESSION : fit ? 0 : ZMQG_ERR_BOUND;
            if (fit)
                zsend_write_header<FR>(out + off, F, hdr, FR == kZsendWsMasked ? ws_key[i] : 0u);
        }
        if (valid) {
            zmqg_zmtp_send_result *r = results + s;
            if (fit) {
                // the last fitting frame of the stream in these 64: it and the
                // `rank` frames below it fit
                if (!has_next || !next_fits)
                    atomicAdd((unsigned long long *) &r->frames, (unsigned long long) rank + 1ull);
            } else if (off <= out_bytes) {
                // the stream's first frame that does not fit (the one before it
                // ends within out_bytes): the fitting frames end where it starts
                r->out_bytes = off - base[s];
            }
        }
    }
}

} // namespace zmqg
