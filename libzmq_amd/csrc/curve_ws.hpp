// curve_ws.hpp -- the WebSocket framing of many connections' receive buffers
// (zmqg_decode_ws_multi) and the masking pass of the send side
// (zmqg_encode_ws_multi).
//
// The reference runs its CURVE mechanism over WebSocket frames as well
// (ws_engine_t::decode_and_push, src/ws_engine.cpp:887-915); the frames come
// from ws_decoder_t (src/ws_decoder.cpp:39-249): byte 0 = FIN | opcode, byte 1
// = MASK | size (below 126, or 126 + 2 bytes, or 127 + 8 bytes, big endian),
// the 4-byte masking key when the sender is a client, then -- binary frames --
// one flags byte (src/ws_protocol.hpp:23-27: more 1, command 2) and the body,
// all XORed with the key from key byte 0 on.
//
// k_ws_streams has k_zmtp_streams's shape (curve_zmtp_multi.hpp): a workgroup
// per stream, the stream in LDS in 16 KiB tiles cut in 16-byte-aligned address
// space, one lane running the decoder's loop from offset 0, all lanes writing
// the slots.  What differs:
//   - a header with its key, flags byte and the 8 signature bytes is up to
//     2 + 8 + 4 + 1 + 8 = 23 bytes, so 32 bytes of the previous tile are kept
//     in front of a tile, and the walker reads two windows: 12 bytes at the
//     frame's first byte (byte 0, byte 1, the extended size), then 16 bytes
//     behind the size (key, flags byte, signature);
//   - the signature test unmasks its 8 bytes with the key rotated by one (the
//     flags byte took key byte 0);
//   - a control frame (close / ping / pong) takes no slot and ends the parse:
//     it goes to results[s].ctl_*;
//   - the frame's flags byte is turned into ZMTP's bit values for the decode
//     (zmtp_msg_bits, curve_frames.hpp).
// This kernel only reads the streams.  k_ws_unmask, the launch behind it,
// rewrites: a workgroup per stream XORs the bodies of the stream's returned
// frames (and its control payload) from `in` into `out`, which may be `in`.
// So the parse sees every byte masked, the decode behind the unmask sees every
// body byte unmasked, and no byte is read in two states by one kernel; the
// unmask reads each key from its header, which nothing rewrites.
#pragma once

#include <errno.h>
#include <stdint.h>

namespace zmqg {

constexpr uint32_t kWsThreads = 256;
constexpr uint32_t kWsTile = 16384; // bytes of a stream in LDS at a time (a power of two)
constexpr uint32_t kWsRounds = kWsTile / 16u / kWsThreads; // 16-byte chunks per lane and tile
constexpr uint32_t kWsHeaderMax = 2 + 8 + 4 + 1 + 8; // header, key, flags byte, signature
constexpr uint32_t kWsKeep = 32;  // bytes of the previous tile kept in front (whole chunks, >= kWsHeaderMax - 1)
constexpr uint32_t kWsSlack = 32; // readable bytes behind the tile (a 16-byte window that starts at its last byte)
constexpr uint32_t kWsList = 512; // frames the LDS list holds between two flushes
constexpr uint32_t kWsSmallBody = 512; // k_ws_unmask: shorter bodies take 8 lanes each
constexpr uint32_t kWsBigBody = 8192;  // bodies from here on are split over the whole workgroup (send: over gridDim.y)
static_assert((kWsTile & (kWsTile - 1)) == 0 && kWsRounds >= 1, "tile: a power of two");
static_assert(kWsKeep % 16 == 0 && kWsKeep >= kWsHeaderMax - 1 && kWsKeep / 16 <= kWsThreads, "kept bytes");
static_assert(kWsSlack >= 3 + 20, "the second window: 5 words from the last byte's word");

enum : uint32_t { kWsWalkTile = 0, kWsWalkDone = 1, kWsWalkFlush = 2 };
struct WsState {
    uint32_t p;        // u of the next header
    uint32_t status;   // kWsWalk*
    uint32_t cnt;      // frames in the list
    uint32_t error;    // 0, EPROTO or EMSGSIZE
    uint32_t ctl_op;   // 0, or the control frame that ended the parse
    uint32_t ctl_len;
    uint32_t ctl_off;  // u of its payload
    unsigned long long first;     // frames of the stream before the list's
    unsigned long long consumed;  // u behind the last returned frame (or the control frame)
    unsigned long long out_bytes; // payload bytes of the returned frames
};

// Tile tb of the stream [mis, end) (u coordinates) at the aligned base `a`:
// this lane's chunks into registers.  Chunks outside the stream are not read.
__device__ __forceinline__ void ws_load(const uint8_t *a, uint32_t mis, uint32_t end, uint32_t tb,
                                        uint4 (&r)[kWsRounds])
{
#pragma unroll
    for (uint32_t k = 0; k < kWsRounds; ++k) {
        const uint32_t u0 = tb + 16u * (k * kWsThreads + threadIdx.x);
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
// last kWsKeep bytes move in front of it (the lanes that overwrite them move them).
__device__ __forceinline__ void ws_store(uint8_t *lds, uint32_t end, uint32_t tb, bool adjacent,
                                         const uint4 (&r)[kWsRounds])
{
    constexpr uint32_t kMovers = kWsKeep / 16u;
    if (adjacent && threadIdx.x >= kWsThreads - kMovers) {
        const uint32_t m = threadIdx.x - (kWsThreads - kMovers);
        *(uint4 *) (lds + 16u * m) = *(const uint4 *) (lds + kWsTile + 16u * m);
    }
#pragma unroll
    for (uint32_t k = 0; k < kWsRounds; ++k) {
        const uint32_t c = 16u * (k * kWsThreads + threadIdx.x);
        if (tb + c < end)
            *(uint4 *) (lds + kWsKeep + c) = r[k];
    }
}

// The 4 N bytes at u = p (tb - kWsKeep <= p < tb + tile) as N little-endian
// words: aligned LDS reads, shifted by p's byte offset.  Bytes behind the
// tile's valid part are whatever the LDS holds; the walker tests positions
// before it uses a byte.
template <uint32_t N>
__device__ __forceinline__ void ws_window(const uint8_t *lds, uint32_t tb, uint32_t p, uint32_t (&x)[N])
{
    const uint32_t i = p + kWsKeep - tb, o = i & 3u;
    const uint32_t *w = (const uint32_t *) (lds + (i & ~3u));
    uint32_t v[N + 1];
#pragma unroll
    for (uint32_t k = 0; k <= N; ++k)
        v[k] = w[k];
#pragma unroll
    for (uint32_t k = 0; k < N; ++k)
        x[k] = __builtin_amdgcn_alignbyte(v[k + 1], v[k], o);
}

// One lane: ws_decoder_t's loop over the tile in LDS, from st.p, until the
// stream's parse ends (Done), the list is full (Flush) or bytes of another
// tile are needed (Tile: the tile of st.p, or -- st.p inside this tile, a
// header or signature across its end -- the next one).  A check is made as
// soon as the bytes that decide it are in the stream; the first one whose
// bytes are missing leaves the frame for the next call.
__device__ __forceinline__ void ws_walk(const uint8_t *lds, uint32_t tb, uint32_t end, uint32_t must_mask,
                                        int64_t max_msg, uint64_t max_frames, uint32_t *l_body, uint32_t *l_len,
                                        uint8_t *l_flag, WsState &st)
{
    const uint32_t tile_end = tb + kWsTile;
    uint32_t p = st.p, cnt = 0, status = kWsWalkDone;
    const uint64_t first = st.first + st.cnt;
    uint64_t consumed = st.consumed, out_bytes = st.out_bytes;
    // whether the first k bytes of the frame at p are missing from the tile: not
    // in the stream (the parse ends), or in the next tile
    const uint32_t here = end < tile_end ? end : tile_end;
    auto missing = [&](uint32_t k) -> bool {
        if (p + k <= here)
            return false;
        if (p + k > end)
            return true;
        if (p + k > tile_end) {
            status = kWsWalkTile;
            return true;
        }
        return false;
    };
    for (;;) {
        if (first + cnt >= max_frames || p >= end)
            break;
        if (p >= tile_end) {
            status = kWsWalkTile;
            break;
        }
        uint32_t x[3];
        ws_window<3>(lds, tb, p, x);
        // byte 0 (src/ws_decoder.cpp:41-63): FIN, and a binary, close, ping or pong frame
        const uint32_t b0 = x[0] & 0xffu, op = b0 & 0x0fu;
        if (!(b0 & 0x80u) || !(op == 2u || op == 8u || op == 9u || op == 10u)) {
            st.error = EPROTO;
            break;
        }
        if (missing(2u))
            break;
        // byte 1 (:72-128): the MASK bit, the size or its form
        const uint32_t b1 = (x[0] >> 8) & 0xffu, l7 = b1 & 0x7fu;
        if ((b1 >> 7) != must_mask) {
            st.error = EPROTO;
            break;
        }
        const uint32_t ext = l7 == 126u ? 2u : l7 == 127u ? 8u : 0u;
        uint32_t hdr = 2u + ext + (must_mask ? 4u : 0u);
        if (missing(2u + ext))
            break;
        uint64_t size = l7;
        if (ext == 2u) {
            size = __builtin_bswap32(x[0]) & 0xffffu; // bytes 2, 3
        } else if (ext == 8u) {
            const uint32_t hi = __builtin_amdgcn_alignbyte(x[1], x[0], 2),
                           lo = __builtin_amdgcn_alignbyte(x[2], x[1], 2);
            size = ((uint64_t) __builtin_bswap32(hi) << 32) | __builtin_bswap32(lo);
        }
        if (missing(hdr)) // the key (:131-144)
            break;
        if (op == 2u && size == 0u) { // (:83-84, :104-105, :122-123, :136-137)
            st.error = EPROTO;
            break;
        }
        if (op == 2u && missing(hdr + 1u)) // the flags byte (:146-163)
            break;
        // key, flags byte, the body's first bytes
        uint32_t y[4], key = 0, wsflags = 0, s0 = 0, s1 = 0;
        ws_window<4>(lds, tb, p + 2u + ext, y);
        if (must_mask) {
            key = y[0];
            y[0] = y[1], y[1] = y[2], y[2] = y[3];
        }
        if (op == 2u) {
            wsflags = (y[0] ^ key) & 0xffu;
            const uint32_t k1 = (key >> 8) | (key << 24); // body byte i under key byte (i + 1) % 4
            s0 = __builtin_amdgcn_alignbyte(y[1], y[0], 1) ^ k1;
            s1 = __builtin_amdgcn_alignbyte(y[2], y[1], 1) ^ k1;
            hdr += 1u;
            size -= 1u;
        }
        if (!zmtp_size_ok(size, max_msg)) { // (:166-173, and this library's 32-bit lengths)
            st.error = EMSGSIZE;
            break;
        }
        if (size > (uint64_t) (end - p - hdr))
            break; // an incomplete body: left for the next call
        if (op != 2u) {
            // not for the mechanism (src/ws_engine.cpp:891-894): the host answers it
            st.ctl_op = op;
            st.ctl_off = p + hdr;
            st.ctl_len = (uint32_t) size;
            p += hdr + (uint32_t) size;
            consumed = p;
            break;
        }
        if (size >= 8u && p + hdr + 8u > tile_end) {
            status = kWsWalkTile; // the signature straddles the tile's end
            break;
        }
        if (cnt == kWsList) {
            status = kWsWalkFlush;
            break;
        }
        l_body[cnt] = p + hdr;
        l_len[cnt] = (uint32_t) size;
        l_flag[cnt] = (uint8_t) ((wsflags & 1u) | ((wsflags & 2u) << 1)); // more, command as ZMTP's 1, 4
        ++cnt;
        p += hdr + (uint32_t) size;
        consumed = p;
        out_bytes += size >= 33u ? size - 33u : 0u;
        if (size < 8u || s0 != 0x53454d07u || s1 != 0x45474153u) // "\x07MES" "SAGE"
            break; // not a MESSAGE: returned as the stream's last frame
    }
    st.p = p;
    st.status = status;
    st.cnt = cnt;
    st.first = first;
    st.consumed = consumed;
    st.out_bytes = out_bytes;
}

// One workgroup per stream (a persistent grid over the streams).  `in` is only
// read; nothing here writes `out`.
__global__ __launch_bounds__(kWsThreads) void k_ws_streams(
    uint32_t n_streams, const uint32_t *__restrict__ stream_sid, const uint64_t *__restrict__ stream_off,
    const uint32_t *__restrict__ stream_len, const uint8_t *in, uint32_t must_mask, int64_t max_msg,
    uint64_t max_frames, uint64_t *__restrict__ f_off, uint32_t *__restrict__ f_len, uint64_t *__restrict__ out_off,
    uint32_t *__restrict__ sid_fill, uint8_t *__restrict__ f_flags, zmqg_ws_result *__restrict__ results)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWsKeep + kWsTile + kWsSlack];
    __shared__ uint32_t l_body[kWsList], l_len[kWsList];
    __shared__ uint8_t l_flag[kWsList];
    __shared__ WsState st;
    const uint32_t tid = threadIdx.x;
    for (uint32_t s = blockIdx.x; s < n_streams; s += gridDim.x) {
        const uint64_t off = stream_off[s];
        const uint32_t n = stream_len[s], sid = stream_sid[s];
        const uint32_t mis = (uint32_t) ((uintptr_t) (in + off) & 15u), end = mis + n;
        const uint8_t *const a = in + off - mis; // (16-byte aligned; only [a + mis, a + end) is read)
        const uint64_t slot0 = (uint64_t) s * max_frames;
        uint4 r[kWsRounds];
        uint32_t tb = 0;
        uint64_t frames = 0;
        if (tid == 0) {
            WsState z{};
            z.p = mis;
            z.consumed = mis;
            st = z;
        }
        if (n > 0) {
            ws_load(a, mis, end, tb, r);
            ws_store(lds, end, tb, false, r);
        }
        bool have_next = false; // r holds tile tb + tile
        uint32_t p = mis;       // st.p, read behind the walk's barrier only (the walker rewrites st)
        while (n > 0) {
            __syncthreads(); // the tile and the walk's state
            if (!have_next && tb + kWsTile < end) { // in flight while the lane walks
                ws_load(a, mis, end, tb + kWsTile, r);
                have_next = true;
            }
            if (tid == 0)
                ws_walk(lds, tb, end, must_mask, max_msg, max_frames, l_body, l_len, l_flag, st);
            __syncthreads(); // the list and the walk's state
            const uint32_t status = st.status, cnt = st.cnt;
            const uint64_t first = st.first;
            p = st.p;
            for (uint32_t i = tid; i < cnt; i += kWsThreads) {
                const uint64_t j = slot0 + first + i, body = off + (l_body[i] - mis);
                f_off[j] = body;
                f_len[j] = l_len[i];
                f_flags[j] = l_flag[i];
                out_off[j] = body; // the payload at its body's offset (see zmqg_decode_zmtp)
            }
            frames = first + cnt;
            if (status == kWsWalkDone)
                break;
            if (status == kWsWalkTile) {
                // p inside the tile: a straddling header, the next tile; else
                // the tile of p (tiles wholly inside a body are not loaded)
                const uint32_t ntb = p < tb + kWsTile ? tb + kWsTile : p & ~(kWsTile - 1u);
                const bool adjacent = ntb == tb + kWsTile;
                if (!(adjacent && have_next))
                    ws_load(a, mis, end, ntb, r);
                ws_store(lds, end, ntb, adjacent, r);
                tb = ntb;
                have_next = false;
            }
        }
        // every slot's session, and the stream's remaining slots: empty frames
        // (on session 0: malformed whatever the stream's session is, and a
        // frame that fails its header checks touches no peer nonce)
        for (uint64_t j = tid; j < max_frames; j += kWsThreads) {
            sid_fill[slot0 + j] = j < frames ? sid : 0u;
            if (j >= frames) {
                f_off[slot0 + j] = 0;
                f_len[slot0 + j] = 0;
                f_flags[slot0 + j] = 0;
                out_off[slot0 + j] = 0;
            }
        }
        if (tid == 0) {
            zmqg_ws_result res{};
            res.frames = frames;
            res.consumed = st.consumed - mis;
            res.out_bytes = st.out_bytes;
            res.error = (int32_t) st.error;
            res.ctl_opcode = (int32_t) st.ctl_op;
            res.ctl_off = st.ctl_op ? off + (st.ctl_off - mis) : 0;
            res.ctl_len = st.ctl_len;
            results[s] = res;
        }
        __syncthreads(); // st and the LDS are the next stream's
    }
}

// dst[off + i] = src[off + i] ^ key[(i + rot) % 4], i < len, by lanes t of nt
// (key: the four key bytes as a little-endian word).  16-byte pieces at
// 16-byte-aligned addresses inside the range -- one key word for all of them,
// rotated by the first piece's index in the WebSocket payload mod 4 --, the
// partial pieces at both ends bytewise.  Every byte is read once and written
// once, by one lane: dst may be src.  (src and dst 16 bytes apart mod 16: all
// bytewise.)
__device__ __forceinline__ void ws_xor_range(const uint8_t *src, uint8_t *dst, uint64_t off, uint64_t len,
                                             uint32_t key, uint32_t rot, uint32_t t, uint32_t nt)
{
    const uint8_t *s = src + off;
    uint8_t *d = dst + off;
    const bool same = (((uintptr_t) s ^ (uintptr_t) d) & 15u) == 0;
    uint64_t head = (uint64_t) (-(uintptr_t) d & 15u);
    if (head > len || !same)
        head = len;
    const uint64_t pieces = (len - head) / 16u, tail0 = head + 16u * pieces;
    for (uint64_t i = t; i < head; i += nt)
        d[i] = (uint8_t) (s[i] ^ (key >> (8u * (((uint32_t) i + rot) & 3u))));
    const uint32_t sh = 8u * (((uint32_t) head + rot) & 3u);
    const uint32_t kw = sh ? (key >> sh) | (key << (32u - sh)) : key;
    for (uint64_t m = t; m < pieces; m += nt) {
        uint4 v = *(const uint4 *) (s + head + 16u * m);
        v.x ^= kw, v.y ^= kw, v.z ^= kw, v.w ^= kw;
        *(uint4 *) (d + head + 16u * m) = v;
    }
    for (uint64_t i = tail0 + t; i < len; i += nt)
        d[i] = (uint8_t) (s[i] ^ (key >> (8u * (((uint32_t) i + rot) & 3u))));
}

__device__ __forceinline__ uint32_t ws_key_at(const uint8_t *p)
{
    return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24);
}

// The launch behind k_ws_streams: one workgroup per stream (a persistent
// grid), over the frames the parse returned.  MASKED: every returned body,
// and the control payload, from `in` to `out` under the frame's key (read from
// its header: the 4 bytes in front of the flags byte, or of a control
// payload); 8 lanes per body below kWsSmallBody bytes, the whole workgroup per
// body of kWsBigBody bytes or more, a wave per body in between.  !MASKED
// (out != in): the control payload is copied.
template <bool MASKED>
__global__ __launch_bounds__(kWsThreads) void k_ws_unmask(uint32_t n_streams, uint64_t max_frames, const uint8_t *in,
                                                         uint8_t *out, const uint64_t *__restrict__ f_off,
                                                         const uint32_t *__restrict__ f_len,
                                                         const zmqg_ws_result *__restrict__ results)
{
    constexpr uint32_t kWaves = kWsThreads / 64u;
    static_assert(kWaves * 8u * 2u == 64u, "two rounds of 8-lane groups cover a wave's 64 frames");
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t s = blockIdx.x; s < n_streams; s += gridDim.x) {
        const zmqg_ws_result res = results[s];
        if (MASKED) {
            // 64 frames at a time, their lengths one per lane (every wave
            // holds the same 64): the short bodies 8 lanes each, 32 of them
            // side by side over the workgroup; the others a wave each, in
            // turns; the long ones all lanes together
            const uint64_t slot0 = (uint64_t) s * max_frames;
            for (uint64_t base = 0; base < res.frames; base += 64u) {
                const uint32_t len_l = base + lane < res.frames ? f_len[slot0 + base + lane] : 0u;
#pragma unroll
                for (uint32_t r = 0; r < 2u; ++r) {
                    const uint32_t b = 32u * r + 8u * wave + (lane >> 3);
                    const uint32_t len = (uint32_t) __shfl((int) len_l, (int) b);
                    if (len > 0 && len < kWsSmallBody) {
                        const uint64_t body = f_off[slot0 + base + b];
                        ws_xor_range(in, out, body, len, ws_key_at(in + body - 5), 1u, lane & 7u, 8u);
                    }
                }
                uint64_t mid = __builtin_amdgcn_ballot_w64(len_l >= kWsSmallBody && len_l < kWsBigBody);
                uint64_t big = __builtin_amdgcn_ballot_w64(len_l >= kWsBigBody);
                for (uint32_t k = 0; mid; mid &= mid - 1u, ++k) {
                    if (k % kWaves != wave)
                        continue;
                    const uint32_t b = (uint32_t) __builtin_ctzll(mid);
                    const uint64_t body = f_off[slot0 + base + b];
                    ws_xor_range(in, out, body, (uint32_t) __shfl((int) len_l, (int) b), ws_key_at(in + body - 5), 1u,
                                 lane, 64u);
                }
                for (; big; big &= big - 1u) {
                    const uint32_t b = (uint32_t) __builtin_ctzll(big);
                    const uint64_t body = f_off[slot0 + base + b];
                    ws_xor_range(in, out, body, (uint32_t) __shfl((int) len_l, (int) b), ws_key_at(in + body - 5), 1u,
                                 tid, kWsThreads);
                }
            }
        }
        if (res.ctl_opcode && res.ctl_len > 0)
            ws_xor_range(in, out, res.ctl_off, res.ctl_len, MASKED ? ws_key_at(in + res.ctl_off - 4) : 0u, 0u, tid,
                         kWsThreads);
    }
}

// zmqg_encode_ws_multi's launch behind the encode: the MESSAGE commands of the
// fitting frames XORed in place with their keys (src/ws_encoder.cpp:94-121:
// byte j under key byte (j + 1) % 4, the flags byte took key byte 0).  Eight
// lanes per frame, the frames strided over the grid's x (a frame's loads do
// not wait for another frame's); a command of kWsBigBody bytes or more is cut
// into gridDim.y slabs of whole 16-byte pieces, one per y, and a shorter
// one is row 0's.  enc_sid / wire_off: what k_zsend_frames gave the encode
// (kZsendNoSession: invalid or not fitting, left untouched).
__global__ __launch_bounds__(kWsThreads) void k_ws_mask_bodies(
    uint32_t n, const uint32_t *__restrict__ enc_sid, const uint64_t *__restrict__ wire_off,
    const uint8_t *__restrict__ flags, const uint32_t *__restrict__ len, const uint32_t *__restrict__ mask,
    const DevSession *__restrict__ sessions, uint8_t *out)
{
    constexpr uint32_t kGroups = kWsThreads / 8u;
    const uint32_t t = threadIdx.x & 7u;
    for (uint64_t i = (uint64_t) blockIdx.x * kGroups + (threadIdx.x >> 3); i < n;
         i += (uint64_t) gridDim.x * kGroups) {
        const uint32_t sid = enc_sid[i];
        if (sid == kZsendNoSession)
            continue;
        const uint64_t W = zsend_wire_bytes(flags[i], len[i], sessions, sid);
        const uint32_t key = __builtin_bswap32(mask[i]); // key byte 0 = the value's top byte, in the word's low byte
        if (W < kWsBigBody) {
            if (blockIdx.y == 0)
                ws_xor_range(out, out, wire_off[i], W, key, 1u, t, 8u);
        } else {
            const uint64_t slab = ((W + gridDim.y - 1) / gridDim.y + 15u) & ~15ull, a = slab * blockIdx.y;
            if (a < W)
                ws_xor_range(out, out, wire_off[i] + a, W - a < slab ? W - a : slab, key, 1u + (uint32_t) (a & 3u), t,
                             8u);
        }
    }
}

} // namespace zmqg
