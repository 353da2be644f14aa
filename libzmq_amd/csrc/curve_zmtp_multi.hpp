// curve_zmtp_multi.hpp -- the ZMTP decoder over many connections' receive
// buffers in one launch (zmqg_decode_zmtp_multi).
//
// curve_zmtp.hpp parses one long stream with every workgroup of the device:
// a candidate scan, links, a walk over linked runs.  An I/O thread's workload
// is the other shape: many connections, each with at most in_batch_size =
// 8,192 bytes per read (src/options.cpp:221).  There the parallelism is across
// the streams, and a short stream needs no candidates: k_zmtp_streams gives
// each stream one workgroup, which copies it into LDS in 16 KiB tiles while
// one lane walks the chain from offset 0 (src/v2_decoder.cpp:35-140: flags
// byte, 1- or 8-byte size, maxmsgsize :74-84, body).  The walk is the
// decoder's own loop, so it is exact whatever the bodies contain: a
// "\x07MESSAGE" signature planted inside a body is never looked at.
//
// Tiles.  The stream is seen through 16-byte chunks of the address space: u =
// stream offset + (address of byte 0 mod 16), so chunk c = [16 c, 16 c + 16)
// is one aligned 16-byte load wherever it lies wholly inside the stream; the
// first and last chunk are read bytewise, and no byte outside the stream is
// read.  Tile t = u in [t T, (t + 1) T), consecutive lanes on consecutive
// chunks.  While the lane walks tile t the loads of tile t + 1 are in flight
// (registers); they are not issued when the frame the walk enters the tile
// with already covers tile t + 1, and a walk that leaves tile t by a body
// which ends beyond tile t + 1 loads the tile of its end next: tiles wholly
// inside a body are not loaded (at most the one in flight when the walk met
// the body's header is).  A header or signature that straddles a tile edge is
// read after the next tile has arrived, through the 16 bytes of the old tile
// kept in front of it.
//
// Output.  The walker appends the frames to an LDS list (flushed by all lanes
// whenever it fills); all lanes write the stream's slots [s max_frames,
// (s + 1) max_frames) of the descriptor arrays -- the frames, then empty
// frames (offset 0, length 0: the decode reports them malformed and writes
// nothing else) -- with the per-frame session and ZMTP flags of the decode
// (decode_batch_impl: sid, zflags), and results[s].
#pragma once

#include <errno.h>
#include <stdint.h>

namespace zmqg {

constexpr uint32_t kZmtpMultiThreads = 256;
constexpr uint32_t kZmtpMultiTile = 16384; // bytes of a stream in LDS at a time (a power of two)
constexpr uint32_t kZmtpMultiRounds = kZmtpMultiTile / 16u / kZmtpMultiThreads; // 16-byte chunks per lane and tile
constexpr uint32_t kZmtpMultiKeep = 16;  // bytes of the previous tile kept in front (a header + signature: 17)
constexpr uint32_t kZmtpMultiSlack = 32; // readable bytes behind the tile (the walker's 24-byte window)
constexpr uint32_t kZmtpMultiList = 512; // frames the LDS list holds between two flushes
static_assert((kZmtpMultiTile & (kZmtpMultiTile - 1)) == 0 && kZmtpMultiRounds >= 1, "tile: a power of two");
static_assert(kZmtpMultiTile >= 4096 && kZmtpMultiTile <= 65536, "tile size");

// walker -> workgroup
enum : uint32_t { kZmWalkTile = 0, kZmWalkDone = 1, kZmWalkFlush = 2 };
struct ZmtpMultiState {
    uint32_t p;        // u of the next header
    uint32_t status;   // kZmWalk*
    uint32_t cnt;      // frames in the list
    uint32_t error;    // 0 or EMSGSIZE
    unsigned long long first;     // frames of the stream before the list's
    unsigned long long consumed;  // u behind the last returned frame
    unsigned long long out_bytes; // payload bytes of the returned frames
};

// Tile tb of the stream [mis, end) (u coordinates) at the aligned base `a`:
// this lane's chunks into registers.  Chunks outside the stream are not read.
__device__ __forceinline__ void zmtp_multi_load(const uint8_t *a, uint32_t mis, uint32_t end, uint32_t tb,
                                                uint4 (&r)[kZmtpMultiRounds])
{
#pragma unroll
    for (uint32_t k = 0; k < kZmtpMultiRounds; ++k) {
        const uint32_t u0 = tb + 16u * (k * kZmtpMultiThreads + threadIdx.x);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (u0 >= mis && u0 + 16u <= end) {
            v = *(const uint4 *) (a + u0);
        } else if (u0 + 16u > mis && u0 < end) { // the stream's first or last chunk
            uint64_t lo = 0, hi = 0;
#pragma unroll 1
            for (uint32_t j = 0; j < 8u; ++j) {
                const uint32_t ul = u0 + j, uh = ul + 8u;
                if (ul >= mis && ul < end)
                    lo |= (uint64_t) a[ul] << (8u * j);
                if (uh >= mis && uh < end)
                    hi |= (uint64_t) a[uh] << (8u * j);
            }
            v = make_uint4((uint32_t) lo, (uint32_t) (lo >> 32), (uint32_t) hi, (uint32_t) (hi >> 32));
        }
        r[k] = v;
    }
}

// Registers -> LDS.  `adjacent`: the new tile follows the one in LDS, whose
// last 16 bytes move in front of it (the lane that overwrites them moves them).
__device__ __forceinline__ void zmtp_multi_store(uint8_t *lds, uint32_t end, uint32_t tb, bool adjacent,
                                                 const uint4 (&r)[kZmtpMultiRounds])
{
    if (adjacent && threadIdx.x == kZmtpMultiThreads - 1u)
        *(uint4 *) lds = *(const uint4 *) (lds + kZmtpMultiTile);
#pragma unroll
    for (uint32_t k = 0; k < kZmtpMultiRounds; ++k) {
        const uint32_t c = 16u * (k * kZmtpMultiThreads + threadIdx.x);
        if (tb + c < end)
            *(uint4 *) (lds + kZmtpMultiKeep + c) = r[k];
    }
}

// The 20 bytes at u = p (p >= tb - kZmtpMultiKeep, p < tb + tile) as five
// little-endian words: aligned LDS reads, shifted by p's byte offset.  Bytes
// behind the tile's valid part are whatever the LDS holds; the callers test
// positions before they use a byte.
__device__ __forceinline__ void zmtp_multi_window(const uint8_t *lds, uint32_t tb, uint32_t p, uint32_t (&x)[5])
{
    const uint32_t i = p + kZmtpMultiKeep - tb, o = i & 3u;
    const uint32_t *w = (const uint32_t *) (lds + (i & ~3u));
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4], w5 = w[5];
    x[0] = __builtin_amdgcn_alignbyte(w1, w0, o);
    x[1] = __builtin_amdgcn_alignbyte(w2, w1, o);
    x[2] = __builtin_amdgcn_alignbyte(w3, w2, o);
    x[3] = __builtin_amdgcn_alignbyte(w4, w3, o);
    x[4] = __builtin_amdgcn_alignbyte(w5, w4, o);
}

// flags byte, header bytes and body size of the header in window x
__device__ __forceinline__ void zmtp_multi_header(const uint32_t (&x)[5], uint32_t &flags, uint32_t &hdr,
                                                  uint64_t &size)
{
    flags = x[0] & 0xffu;
    if (flags & kZmtpLarge) {
        // bytes 1..8, big endian
        const uint32_t hi = __builtin_amdgcn_alignbyte(x[1], x[0], 1), lo = __builtin_amdgcn_alignbyte(x[2], x[1], 1);
        hdr = 9;
        size = ((uint64_t) __builtin_bswap32(hi) << 32) | __builtin_bswap32(lo);
    } else {
        hdr = 2;
        size = (x[0] >> 8) & 0xffu;
    }
}

// "\x07MESSAGE" at byte hdr (2 or 9) of window x
__device__ __forceinline__ bool zmtp_multi_signature(const uint32_t (&x)[5], uint32_t hdr)
{
    uint32_t a, b;
    if (hdr == 9) {
        a = __builtin_amdgcn_alignbyte(x[3], x[2], 1);
        b = __builtin_amdgcn_alignbyte(x[4], x[3], 1);
    } else {
        a = __builtin_amdgcn_alignbyte(x[1], x[0], 2);
        b = __builtin_amdgcn_alignbyte(x[2], x[1], 2);
    }
    return a == 0x53454d07u && b == 0x45474153u; // "\x07MES" "SAGE"
}

// Whether the walk that enters the tile in LDS at p can go on into the next
// tile: false when the frame at p ends at or beyond that tile's end (or its
// header is not yet readable: then the next tile is the one needed).
__device__ __forceinline__ bool zmtp_multi_wants_next(const uint8_t *lds, uint32_t tb, uint32_t end, uint32_t p)
{
    const uint32_t tile_end = tb + kZmtpMultiTile;
    if (tile_end >= end)
        return false; // the last tile
    if (p + 9u > tile_end)
        return true;
    uint32_t x[5], flags, hdr;
    uint64_t size;
    zmtp_multi_window(lds, tb, p, x);
    zmtp_multi_header(x, flags, hdr, size);
    return size < (uint64_t) (tile_end + kZmtpMultiTile - p - hdr);
}

// One lane: the decoder's loop over the tile in LDS, from st.p, until the
// stream's parse ends (Done), the list is full (Flush) or bytes of another
// tile are needed (Tile: the tile of st.p, or -- st.p inside this tile, a
// straddling header or signature -- the next one).
__device__ __forceinline__ void zmtp_multi_walk(const uint8_t *lds, uint32_t tb, uint32_t end, int64_t max_msg,
                                                uint64_t max_frames, uint32_t *l_body, uint32_t *l_len,
                                                uint8_t *l_flag, ZmtpMultiState &st)
{
    const uint32_t tile_end = tb + kZmtpMultiTile;
    uint32_t p = st.p, cnt = 0, status = kZmWalkDone;
    const uint64_t first = st.first + st.cnt;
    uint64_t consumed = st.consumed, out_bytes = st.out_bytes;
    for (;;) {
        if (first + cnt >= max_frames || p + 2u > end)
            break;
        if (p >= tile_end || p + 2u > tile_end) {
            status = kZmWalkTile;
            break;
        }
        uint32_t x[5], flags, hdr;
        uint64_t size;
        zmtp_multi_window(lds, tb, p, x);
        zmtp_multi_header(x, flags, hdr, size);
        if (p + hdr > end)
            break; // an incomplete LARGE header
        if (p + hdr > tile_end) {
            status = kZmWalkTile;
            break;
        }
        if (!zmtp_size_ok(size, max_msg)) {
            st.error = EMSGSIZE; // src/v2_decoder.cpp:74-84: the decoder fails here
            break;
        }
        if (size > (uint64_t) (end - p - hdr))
            break; // an incomplete body: left for the next call
        if (size >= 8u && p + hdr + 8u > tile_end) {
            status = kZmWalkTile; // the signature straddles the tile's end
            break;
        }
        if (cnt == kZmtpMultiList) {
            status = kZmWalkFlush;
            break;
        }
        l_body[cnt] = p + hdr;
        l_len[cnt] = (uint32_t) size;
        l_flag[cnt] = (uint8_t) flags;
        ++cnt;
        p += hdr + (uint32_t) size;
        consumed = p;
        out_bytes += size >= 33u ? size - 33u : 0u;
        if (size < 8u || !zmtp_multi_signature(x, hdr))
            break; // not a MESSAGE: returned as the stream's last frame
    }
    st.p = p;
    st.status = status;
    st.cnt = cnt;
    st.first = first;
    st.consumed = consumed;
    st.out_bytes = out_bytes;
}

// One workgroup per stream (a persistent grid over the streams).
__global__ __launch_bounds__(kZmtpMultiThreads) void k_zmtp_streams(
    uint32_t n_streams, const uint32_t *__restrict__ stream_sid, const uint64_t *__restrict__ stream_off,
    const uint32_t *__restrict__ stream_len, const uint8_t *__restrict__ in, int64_t max_msg, uint64_t max_frames,
    uint64_t *__restrict__ f_off, uint32_t *__restrict__ f_len, uint64_t *__restrict__ out_off,
    uint32_t *__restrict__ sid_fill, uint8_t *__restrict__ f_flags, zmqg_zmtp_result *__restrict__ results)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kZmtpMultiKeep + kZmtpMultiTile + kZmtpMultiSlack];
    __shared__ uint32_t l_body[kZmtpMultiList], l_len[kZmtpMultiList];
    __shared__ uint8_t l_flag[kZmtpMultiList];
    __shared__ ZmtpMultiState st;
    const uint32_t tid = threadIdx.x;
    for (uint32_t s = blockIdx.x; s < n_streams; s += gridDim.x) {
        const uint64_t off = stream_off[s];
        const uint32_t n = stream_len[s], sid = stream_sid[s];
        const uint32_t mis = (uint32_t) ((uintptr_t) (in + off) & 15u), end = mis + n;
        const uint8_t *const a = in + off - mis; // (16-byte aligned; only [a + mis, a + end) is read)
        const uint64_t slot0 = (uint64_t) s * max_frames;
        uint4 r[kZmtpMultiRounds];
        uint32_t tb = 0;
        uint64_t frames = 0;
        if (tid == 0) {
            ZmtpMultiState z{};
            z.p = mis;
            z.consumed = mis;
            st = z;
        }
        if (n > 0) {
            zmtp_multi_load(a, mis, end, tb, r);
            zmtp_multi_store(lds, end, tb, false, r);
        }
        bool have_next = false; // r holds tile tb + tile
        uint32_t p = mis;       // st.p, read behind the walk's barrier only (the walker rewrites st)
        while (n > 0) {
            __syncthreads(); // the tile and the walk's state
            if (!have_next && zmtp_multi_wants_next(lds, tb, end, p)) {
                zmtp_multi_load(a, mis, end, tb + kZmtpMultiTile, r);
                have_next = true;
            }
            if (tid == 0)
                zmtp_multi_walk(lds, tb, end, max_msg, max_frames, l_body, l_len, l_flag, st);
            __syncthreads(); // the list and the walk's state
            const uint32_t status = st.status, cnt = st.cnt;
            const uint64_t first = st.first;
            p = st.p;
            for (uint32_t i = tid; i < cnt; i += kZmtpMultiThreads) {
                const uint64_t j = slot0 + first + i, body = off + (l_body[i] - mis);
                f_off[j] = body;
                f_len[j] = l_len[i];
                f_flags[j] = l_flag[i];
                out_off[j] = body; // the payload at its body's offset (see zmqg_decode_zmtp)
            }
            frames = first + cnt;
            if (status == kZmWalkDone)
                break;
            if (status == kZmWalkTile) {
                // p inside the tile: a straddling header, the next tile
                const uint32_t ntb = p < tb + kZmtpMultiTile ? tb + kZmtpMultiTile : p & ~(kZmtpMultiTile - 1u);
                const bool adjacent = ntb == tb + kZmtpMultiTile;
                if (!(adjacent && have_next))
                    zmtp_multi_load(a, mis, end, ntb, r);
                zmtp_multi_store(lds, end, ntb, adjacent, r);
                tb = ntb;
                have_next = false;
            }
        }
        // every slot's session, and the stream's remaining slots: empty frames
        // (on session 0: malformed whatever the stream's session is, and a
        // frame that fails its header checks touches no peer nonce)
        for (uint64_t j = tid; j < max_frames; j += kZmtpMultiThreads) {
            sid_fill[slot0 + j] = j < frames ? sid : 0u;
            if (j >= frames) {
                f_off[slot0 + j] = 0;
                f_len[slot0 + j] = 0;
                f_flags[slot0 + j] = 0;
                out_off[slot0 + j] = 0;
            }
        }
        if (tid == 0) {
            zmqg_zmtp_result res{};
            res.frames = frames;
            res.consumed = st.consumed - mis;
            res.out_bytes = st.out_bytes;
            res.error = (int32_t) st.error;
            results[s] = res;
        }
        __syncthreads(); // st and the LDS are the next stream's
    }
}

} // namespace zmqg
