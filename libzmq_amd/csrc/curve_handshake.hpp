// curve_handshake.hpp -- the server side of the CURVE handshake in batches
// (SURVEY.md section 8f row 3): HELLO -> WELCOME, INITIATE -> READY for many
// connections per call.
//
//   k_hs_hello     curve_server_t::process_hello + produce_welcome
//                  (reference src/curve_server.cpp:117-254)
//   k_hs_initiate  curve_server_t::process_initiate up to the ZAP decision
//                  (src/curve_server.cpp:256-383)
//   k_hs_ready     curve_server_t::produce_ready (src/curve_server.cpp:419-458)
//
// Not here: the client side (produce_hello, process_welcome, produce_initiate,
// process_ready) is curve_handshake_client.hpp, built on the helpers below;
// ZAP and parse_metadata (the host does them between INITIATE and READY, as
// the reference does) and ERROR commands are in neither.
//
// Work split.  A HELLO needs three X25519 ladders that do not depend on each
// other -- X25519(server_sk, C') for the HELLO / WELCOME key, X25519(s', 9) for
// S', X25519(s', C') for the connection's precom -- and a ladder is ~99 % of
// the call.  A workgroup of three waves serves 64 connections: wave r runs
// ladder r for all 64 (one x25519() call whose inputs are selected by the wave
// index, so there is no divergence inside a ladder and no lane idles through
// it), the 3 x 32 result bytes per connection cross through LDS, and wave 0
// then does the HSalsa20s, the HELLO open, the cookie secretbox and the
// WELCOME seal, one lane per connection, with every box in registers.  A HELLO
// so costs the latency of one ladder, not three in a row.  INITIATE has one
// ladder left, X25519(s', C), which depends on the opened box: one lane per
// connection, the checks in the reference's order.  READY is one seal.
//
// A box here is crypto_box_easy_afternm (curve_box.hpp): HSalsa20(key,
// nonce[0:16]) gives the subkey, keystream block 0 the Poly1305 key (bytes
// 0..31) and the first 32 message bytes' stream (bytes 32..63), message byte p
// is stream byte 32 + p.  All stores are ordinary vector stores.
#pragma once

#include "curve_device.hpp"
#include "curve_x25519.hpp"

namespace zmqg {

constexpr int32_t kHsErrUnexpected = 0x10000001;       // ZMQ_PROTOCOL_ERROR_ZMTP_UNEXPECTED_COMMAND
constexpr int32_t kHsErrKeyExchange = 0x10000003;      // ..._KEY_EXCHANGE
constexpr int32_t kHsErrMalformed = 0x10000011;        // ..._MALFORMED_COMMAND_UNSPECIFIED
constexpr int32_t kHsErrMalformedHello = 0x10000013;   // ..._MALFORMED_COMMAND_HELLO
constexpr int32_t kHsErrMalformedInitiate = 0x10000014; // ..._MALFORMED_COMMAND_INITIATE
constexpr int32_t kHsErrCrypto = 0x11000001;           // ..._CRYPTOGRAPHIC

constexpr uint32_t kHsState = 128, kHsRandom = 96, kHsWelcome = 168;
constexpr int kHsHelloThreads = 192; // three waves: one per ladder

// four characters as the little-endian word they are in memory
__device__ constexpr uint32_t hs_w4(char a, char b, char c, char d)
{
    return (uint32_t) (uint8_t) a | ((uint32_t) (uint8_t) b << 8) | ((uint32_t) (uint8_t) c << 16) |
           ((uint32_t) (uint8_t) d << 24);
}

// 8 little-endian words <-> 32 bytes (x25519() works on bytes)
__device__ __forceinline__ void hs_words_to_bytes(uint8_t b[32], const uint32_t w[8])
{
#pragma unroll
    for (int i = 0; i < 32; ++i)
        b[i] = (uint8_t) (w[i >> 2] >> (8 * (i & 3)));
}

__device__ __forceinline__ void hs_bytes_to_words(uint32_t w[8], const uint8_t b[32])
{
#pragma unroll
    for (int i = 0; i < 8; ++i)
        w[i] = (uint32_t) b[4 * i] | ((uint32_t) b[4 * i + 1] << 8) | ((uint32_t) b[4 * i + 2] << 16) |
               ((uint32_t) b[4 * i + 3] << 24);
}

// crypto_box_beforenm's second half: HSalsa20(shared point, 0^16)
__device__ __forceinline__ void hs_beforenm_core(uint32_t k[8], const uint32_t q[8])
{
    const uint32_t zero[4] = {0, 0, 0, 0};
    hsalsa20(k, q, zero);
}

// The per-box key material: the XSalsa20 subkey, the 8 stream-nonce bytes,
// the Poly1305 key and keystream bytes 32..63 (the first 32 message bytes').
struct HsBox {
    uint32_t sub[8], n0, n1;
    fe r;
    uint32_t s1, s2, s3, s4, pad[4], ks0[8];
};

// nonce = 24 bytes as six words: HSalsa20 takes the first four
__device__ __forceinline__ void hs_box_init(HsBox &b, const uint32_t key[8], const uint32_t nonce[6])
{
    hsalsa20(b.sub, key, nonce);
    b.n0 = nonce[4];
    b.n1 = nonce[5];
    uint32_t ks[16];
    salsa20_block(ks, b.sub, b.n0, b.n1, 0, 0);
    b.r = poly_r_from_key(ks[0], ks[1], ks[2], ks[3]);
    b.s1 = b.r.l[1] * 5, b.s2 = b.r.l[2] * 5, b.s3 = b.r.l[3] * 5, b.s4 = b.r.l[4] * 5;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        b.pad[k] = ks[4 + k];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        b.ks0[k] = ks[8 + k];
}

// XSalsa20 over MW message words held in registers (in place): word k is
// stream word 8 + k
template <int MW>
__device__ __forceinline__ void hs_xor_words(const HsBox &b, uint32_t m[MW])
{
#pragma unroll
    for (int k = 0; k < 8 && k < MW; ++k)
        m[k] ^= b.ks0[k];
#pragma unroll
    for (int w = 1; 16 * w - 8 < MW; ++w) {
        uint32_t ks[16];
        salsa20_block(ks, b.sub, b.n0, b.n1, (uint32_t) w, 0);
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (16 * w - 8 + k < MW)
                m[16 * w - 8 + k] ^= ks[k];
    }
}

// Poly1305 tag over MW ciphertext words (whole 64-byte steps)
template <int MW>
__device__ __forceinline__ void hs_tag_words(const HsBox &b, const uint32_t c[MW], uint32_t tag[4])
{
    static_assert(MW % 16 == 0, "whole 64-byte steps");
    fe h = fe_zero();
#pragma unroll
    for (int p = 0; p < MW; p += 16) {
        uint32_t w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k)
            w[k] = c[p + k];
        poly_absorb64(h, b.r, b.s1, b.s2, b.s3, b.s4, w, 64);
    }
    poly_finish(h, b.pad, tag);
}

// Seal MW words in place under (key, nonce): m becomes the ciphertext
template <int MW>
__device__ __forceinline__ void hs_seal_words(const uint32_t key[8], const uint32_t nonce[6], uint32_t m[MW],
                                              uint32_t tag[4])
{
    HsBox b;
    hs_box_init(b, key, nonce);
    hs_xor_words<MW>(b, m);
    hs_tag_words<MW>(b, m, tag);
}

// Open MW words in place: verify the tag over the ciphertext, then decrypt.
// False (c left as it was) when the tag does not verify.
template <int MW>
__device__ __forceinline__ bool hs_open_words(const uint32_t key[8], const uint32_t nonce[6], const uint32_t tag[4],
                                              uint32_t c[MW])
{
    HsBox b;
    hs_box_init(b, key, nonce);
    uint32_t t[4];
    hs_tag_words<MW>(b, c, t);
    if ((t[0] ^ tag[0]) | (t[1] ^ tag[1]) | (t[2] ^ tag[2]) | (t[3] ^ tag[3]))
        return false;
    hs_xor_words<MW>(b, c);
    return true;
}

__device__ __forceinline__ void hs_zero_words(uint32_t *p, int nw)
{
    for (int k = 0; k < nw; ++k)
        p[k] = 0;
}

// The first `want` (<= 12) bytes of a command of `len` bytes, zero beyond len:
// nothing is read for an empty command.
__device__ __forceinline__ void hs_head(const uint8_t *c, uint32_t len, int want, uint32_t w[16])
{
    const int nv = (int) (len < (uint32_t) want ? len : (uint32_t) want);
    if (nv > 0) {
        load_window(c, nv, w);
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            w[k] = 0;
    }
}

// process_hello's checks before the box (src/curve_server.cpp:119-151,
// check_basic_command_structure src/mechanism_base.cpp:14-25), in order
__device__ __forceinline__ int32_t hs_hello_checks(const uint8_t *c, uint32_t len)
{
    uint32_t w[16];
    hs_head(c, len, 8, w);
    if (len <= 1u || len <= (w[0] & 0xffu))
        return kHsErrMalformed;
    if (len < 6u || w[0] != hs_w4('\x05', 'H', 'E', 'L') || (w[1] & 0xffffu) != (hs_w4('L', 'O', 0, 0)))
        return kHsErrUnexpected;
    if (len != 200u)
        return kHsErrMalformedHello;
    if ((w[1] >> 16) != 0x0001u) // major 1, minor 0
        return kHsErrMalformedHello;
    return 0;
}

// HELLO -> WELCOME.  Connection i: command cmd[cmd_off[i] .. +cmd_len[i]),
// random[96 i ..] = s' | cookie key | cookie nonce(16) | WELCOME nonce(16).
// Writes status[i], welcome[168 i ..] and state[128 i ..] = C' | s' | cookie
// key | precom; both zero-filled on failure.
__global__ __launch_bounds__(kHsHelloThreads) __attribute__((amdgpu_waves_per_eu(3))) void k_hs_hello(
    uint32_t n, const uint8_t *__restrict__ server_sk, const uint64_t *__restrict__ cmd_off,
    const uint32_t *__restrict__ cmd_len, const uint8_t *__restrict__ cmd, const uint8_t *__restrict__ random,
    uint8_t *__restrict__ state, uint8_t *__restrict__ welcome, int32_t *__restrict__ status)
{
    __shared__ uint32_t lds_q[3][8][64]; // ladder r's result, word-major: lanes hit distinct banks
    __shared__ uint32_t lds_keep[22][64]; // wave 0's C' | short nonce | box tag (14 words) and s' (8)
    const uint32_t lane = threadIdx.x & 63u, r = threadIdx.x >> 6; // r is wave-uniform
    const uint32_t i = blockIdx.x * 64u + lane;
    const bool live = i < n;
    const uint8_t *c = nullptr;
    int32_t st = 0;
    // a | nonce | tag of the command: C'(8 words) short nonce(2) box tag(4)
    uint32_t a[16], sp[8];
#pragma unroll
    for (int k = 0; k < 16; ++k)
        a[k] = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        sp[k] = 0;
    if (live) {
        c = cmd + cmd_off[i];
        st = hs_hello_checks(c, cmd_len[i]);
        if (st == 0)
            load_window(c + 80, 56, a);
        const uint32_t *rw = (const uint32_t *) (random + (uint64_t) kHsRandom * i);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            sp[k] = rw[k];
    }
    // Ladder r: 0 X25519(server_sk, C'), 1 X25519(s', 9), 2 X25519(s', C').
    // A connection that failed its checks, or a lane past n, runs the ladder
    // on zeros: every lane reaches the barrier.
    {
        uint32_t sw[8], pw[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            sw[k] = r == 0 ? ((uint32_t) server_sk[4 * k] | ((uint32_t) server_sk[4 * k + 1] << 8) |
                              ((uint32_t) server_sk[4 * k + 2] << 16) | ((uint32_t) server_sk[4 * k + 3] << 24))
                           : sp[k];
            pw[k] = r == 1 ? (k == 0 ? 9u : 0u) : a[k];
        }
        // what wave 0 needs again after the ladder waits in LDS, not in
        // registers: the ladder then runs in k_beforenm's register budget
        // (three waves per SIMD)
        if (r == 0) {
#pragma unroll
            for (int k = 0; k < 14; ++k)
                lds_keep[k][lane] = a[k];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                lds_keep[14 + k][lane] = sp[k];
        }
        uint8_t sb[32], pb[32], qb[32];
        hs_words_to_bytes(sb, sw);
        hs_words_to_bytes(pb, pw);
        (void) x25519(qb, sb, pb);
        uint32_t qw[8];
        hs_bytes_to_words(qw, qb);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            lds_q[r][k][lane] = qw[k];
    }
    __syncthreads();
    if (r != 0 || !live)
        return;
#pragma unroll
    for (int k = 0; k < 14; ++k)
        a[k] = lds_keep[k][lane];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        sp[k] = lds_keep[14 + k][lane];
    uint32_t *wel = (uint32_t *) (welcome + (uint64_t) kHsWelcome * i);
    uint32_t *sta = (uint32_t *) (state + (uint64_t) kHsState * i);
    uint32_t k1[8];
    if (st == 0) {
        uint32_t q[8], d = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            q[k] = lds_q[0][k][lane];
            d |= q[k];
        }
        // an all-zero shared point (small-order C'): crypto_box_open fails
        if (d == 0)
            st = kHsErrCrypto;
        hs_beforenm_core(k1, q);
    }
    if (st == 0) {
        // Open Box [64 * %x0](C'->S): only the verdict is needed
        uint32_t ct[16];
        load_window(c + 136, 64, ct);
        const uint32_t nonce[6] = {hs_w4('C', 'u', 'r', 'v'), hs_w4('e', 'Z', 'M', 'Q'), hs_w4('H', 'E', 'L', 'L'),
                                   hs_w4('O', '-', '-', '-'), a[8], a[9]};
        const uint32_t tag[4] = {a[10], a[11], a[12], a[13]};
        if (!hs_open_words<16>(k1, nonce, tag, ct))
            st = kHsErrCrypto;
    }
    if (st != 0) {
        status[i] = st;
        hs_zero_words(wel, kHsWelcome / 4);
        hs_zero_words(sta, kHsState / 4);
        return;
    }
    const uint32_t *rw = (const uint32_t *) (random + (uint64_t) kHsRandom * i);
    uint32_t ck[8], cn[4], wn[4];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        ck[k] = rw[8 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cn[k] = rw[16 + k];
        wn[k] = rw[20 + k];
    }
    // WELCOME plaintext: S' | cookie nonce | cookie box (tag | Box [C' + s'](t))
    uint32_t m[32];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        m[k] = lds_q[1][k][lane];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        m[8 + k] = cn[k];
    {
        uint32_t cookie[16], tag[4];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            cookie[k] = a[k];
            cookie[8 + k] = sp[k];
        }
        const uint32_t nonce[6] = {hs_w4('C', 'O', 'O', 'K'), hs_w4('I', 'E', '-', '-'), cn[0], cn[1], cn[2], cn[3]};
        hs_seal_words<16>(ck, nonce, cookie, tag);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            m[12 + k] = tag[k];
#pragma unroll
        for (int k = 0; k < 16; ++k)
            m[16 + k] = cookie[k];
    }
    uint32_t wtag[4];
    {
        const uint32_t nonce[6] = {hs_w4('W', 'E', 'L', 'C'), hs_w4('O', 'M', 'E', '-'), wn[0], wn[1], wn[2], wn[3]};
        hs_seal_words<32>(k1, nonce, m, wtag);
    }
    wel[0] = hs_w4('\x07', 'W', 'E', 'L');
    wel[1] = hs_w4('C', 'O', 'M', 'E');
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        wel[2 + k] = wn[k];
        wel[6 + k] = wtag[k];
    }
#pragma unroll
    for (int k = 0; k < 32; ++k)
        wel[10 + k] = m[k];
    // precom = crypto_box_beforenm(C', s'): the reference derives it at
    // INITIATE (src/curve_server.cpp:382-383); the value is the same
    uint32_t q2[8], pre[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        q2[k] = lds_q[2][k][lane];
    hs_beforenm_core(pre, q2);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        sta[k] = a[k];
        sta[8 + k] = sp[k];
        sta[16 + k] = ck[k];
        sta[24 + k] = pre[k];
    }
    status[i] = 0;
}

// INITIATE.  state[128 i ..] is what k_hs_hello wrote for the connection.
__global__ __launch_bounds__(64) void k_hs_initiate(uint32_t n, const uint8_t *__restrict__ state,
                                                    const uint64_t *__restrict__ cmd_off,
                                                    const uint32_t *__restrict__ cmd_len,
                                                    const uint8_t *__restrict__ cmd,
                                                    uint8_t *__restrict__ client_key,
                                                    uint8_t *__restrict__ precom_out,
                                                    unsigned long long *__restrict__ peer_nonce,
                                                    const uint64_t *__restrict__ meta_off,
                                                    uint8_t *__restrict__ meta_out, uint32_t *__restrict__ meta_len,
                                                    int32_t *__restrict__ status)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint8_t *c = cmd + cmd_off[i];
    const uint32_t len = cmd_len[i];
    const uint32_t *sta = (const uint32_t *) (state + (uint64_t) kHsState * i);
    uint32_t *ck_out = (uint32_t *) (client_key + 32ull * i);
    uint32_t *pre_out = (uint32_t *) (precom_out + 32ull * i);
    int32_t st = 0;
    uint32_t cp[8], sp[8], pre[8]; // C', s', precom
    uint32_t pt[32];               // C | vouch nonce | vouch box: the first 128 plaintext bytes
    uint32_t n0 = 0, n1 = 0;
    HsBox ib;
    do {
        // src/curve_server.cpp:258-278
        uint32_t w[16];
        hs_head(c, len, 9, w);
        if (len <= 1u || len <= (w[0] & 0xffu)) {
            st = kHsErrMalformed;
            break;
        }
        if (len < 9u || w[0] != hs_w4('\x08', 'I', 'N', 'I') || w[1] != hs_w4('T', 'I', 'A', 'T') ||
            (w[2] & 0xffu) != (uint32_t) 'E') {
            st = kHsErrUnexpected;
            break;
        }
        if (len < 257u) {
            st = kHsErrMalformedInitiate;
            break;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            cp[k] = sta[k];
            sp[k] = sta[8 + k];
            pre[k] = sta[24 + k];
        }
        // Open Box [C' + s'](t) (:280-299) and compare (:301-313)
        {
            uint32_t ck[8], h[16], ct[16];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                ck[k] = sta[16 + k];
            load_window(c + 9, 32, h); // cookie nonce(16) | cookie box tag(16)
            load_window(c + 41, 64, ct);
            const uint32_t nonce[6] = {hs_w4('C', 'O', 'O', 'K'), hs_w4('I', 'E', '-', '-'), h[0], h[1], h[2], h[3]};
            const uint32_t tag[4] = {h[4], h[5], h[6], h[7]};
            if (!hs_open_words<16>(ck, nonce, tag, ct)) {
                st = kHsErrCrypto;
                break;
            }
            uint32_t d = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                d |= (ct[k] ^ cp[k]) | (ct[8 + k] ^ sp[k]);
            if (d) {
                st = kHsErrCrypto;
                break;
            }
        }
        // Open Box [C + vouch + metadata](C'->S') (:315-342): the tag over the
        // whole ciphertext first; only the first 128 plaintext bytes are
        // decrypted now, into registers
        const uint32_t mlen = len - 129u; // >= 128
        const uint8_t *ct = c + 129;
        {
            uint32_t h[16];
            load_window(c + 105, 24, h); // short nonce(8) | tag(16)
            n0 = h[0], n1 = h[1];
            const uint32_t nonce[6] = {hs_w4('C', 'u', 'r', 'v'), hs_w4('e', 'Z', 'M', 'Q'),
                                       hs_w4('I', 'N', 'I', 'T'), hs_w4('I', 'A', 'T', 'E'), n0, n1};
            hs_box_init(ib, pre, nonce);
            fe acc = fe_zero();
            for (uint32_t p = 0; p < mlen; p += 64u) {
                const int nv = (int) (mlen - p < 64u ? mlen - p : 64u);
                uint32_t x[16];
                load_window(ct + p, nv, x);
                poly_absorb64(acc, ib.r, ib.s1, ib.s2, ib.s3, ib.s4, x, nv);
            }
            uint32_t t[4];
            poly_finish(acc, ib.pad, t);
            if ((t[0] ^ h[2]) | (t[1] ^ h[3]) | (t[2] ^ h[4]) | (t[3] ^ h[5])) {
                st = kHsErrCrypto;
                break;
            }
            uint32_t x[16];
            load_window(ct, 64, x);
#pragma unroll
            for (int k = 0; k < 16; ++k)
                pt[k] = x[k];
            load_window(ct + 64, 64, x);
#pragma unroll
            for (int k = 0; k < 16; ++k)
                pt[16 + k] = x[k];
            hs_xor_words<32>(ib, pt);
        }
        // Open Box [C',S](C->S') (:344-367) under crypto_box_beforenm(C, s')
        uint32_t kv[8];
        {
            uint8_t sb[32], pb[32], qb[32];
            hs_words_to_bytes(sb, sp);
            hs_words_to_bytes(pb, pt);
            if (x25519(qb, sb, pb) != 0) { // small-order C: crypto_box_open fails
                st = kHsErrCrypto;
                break;
            }
            uint32_t q[8];
            hs_bytes_to_words(q, qb);
            hs_beforenm_core(kv, q);
        }
        {
            uint32_t v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k)
                v[k] = pt[16 + k];
            const uint32_t nonce[6] = {hs_w4('V', 'O', 'U', 'C'), hs_w4('H', '-', '-', '-'), pt[8], pt[9], pt[10],
                                       pt[11]};
            const uint32_t tag[4] = {pt[12], pt[13], pt[14], pt[15]};
            if (!hs_open_words<16>(kv, nonce, tag, v)) {
                st = kHsErrCrypto;
                break;
            }
            // what we decrypted must be the client's short-term public key (:369-379)
            uint32_t d = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                d |= v[k] ^ cp[k];
            if (d) {
                st = kHsErrKeyExchange;
                break;
            }
        }
        // accepted: the metadata, message bytes 128 .. mlen, is decrypted only now
        uint8_t *dst = meta_out + meta_off[i];
        for (uint32_t w = 2; w == 2 ? mlen > 128u : 64u * w - 32u < mlen; ++w) {
            const uint32_t p0 = w == 2 ? 128u : 64u * w - 32u; // first message byte of this piece
            const uint32_t cap = w == 2 ? 32u : 64u;
            const int nv = (int) (mlen - p0 < cap ? mlen - p0 : cap);
            uint32_t ks[16], x[16], y[16];
            salsa20_block(ks, ib.sub, ib.n0, ib.n1, w, 0);
            load_window(ct + p0, nv, x);
#pragma unroll
            for (int k = 0; k < 16; ++k)
                y[k] = x[k] ^ (w == 2 ? (k < 8 ? ks[8 + k] : 0u) : ks[k]);
            mask_tail(y, nv);
            store_window(dst + (p0 - 128u), nv, y);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            ck_out[k] = pt[k];
            pre_out[k] = pre[k];
        }
        // get_uint64 (initiate + 105): the value set_peer_nonce receives (:330)
        peer_nonce[i] = ((unsigned long long) bswap32(n0) << 32) | bswap32(n1);
        meta_len[i] = len - 257u;
        status[i] = 0;
        return;
    } while (0);
    hs_zero_words(ck_out, 8);
    hs_zero_words(pre_out, 8);
    peer_nonce[i] = 0;
    meta_len[i] = 0;
    status[i] = st;
}

// READY: "\x05READY" | BE64(nonce) | Box [metadata](S'->C') under precom
__global__ __launch_bounds__(64) void k_hs_ready(uint32_t n, const uint8_t *__restrict__ precom,
                                                 const unsigned long long *__restrict__ nonce,
                                                 const uint64_t *__restrict__ meta_off,
                                                 const uint32_t *__restrict__ meta_len,
                                                 const uint8_t *__restrict__ meta,
                                                 const uint64_t *__restrict__ out_off, uint8_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t *pw = (const uint32_t *) (precom + 32ull * i);
    uint32_t key[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        key[k] = pw[k];
    const unsigned long long nn = nonce[i];
    const uint32_t n0 = bswap32((uint32_t) (nn >> 32)), n1 = bswap32((uint32_t) nn); // put_uint64: big endian
    const uint32_t bn[6] = {hs_w4('C', 'u', 'r', 'v'), hs_w4('e', 'Z', 'M', 'Q'), hs_w4('R', 'E', 'A', 'D'),
                            hs_w4('Y', '-', '-', '-'), n0, n1};
    HsBox b;
    hs_box_init(b, key, bn);
    const uint32_t mlen = meta_len[i];
    const uint8_t *src = meta + meta_off[i];
    uint8_t *dst = out + out_off[i];
    fe h = fe_zero();
    const uint32_t nwin = (mlen + 32u + 63u) / 64u;
    for (uint32_t w = 0; w < nwin; ++w) {
        const uint32_t p0 = w == 0 ? 0u : 64u * w - 32u;
        const uint32_t cap = w == 0 ? 32u : 64u;
        const int nv = (int) (mlen - p0 < cap ? mlen - p0 : cap);
        uint32_t ks[16], x[16], y[16];
        if (w > 0)
            salsa20_block(ks, b.sub, b.n0, b.n1, w, 0);
        if (nv > 0) {
            load_window(src + p0, nv, x);
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                x[k] = 0;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k)
            y[k] = x[k] ^ (w == 0 ? (k < 8 ? b.ks0[k] : 0u) : ks[k]);
        mask_tail(y, nv);
        store_window(dst + 30 + p0, nv, y);
        poly_absorb64(h, b.r, b.s1, b.s2, b.s3, b.s4, y, nv);
    }
    uint32_t head[16] = {0};
    poly_finish(h, b.pad, head + 4); // bytes 16..31 of the window below
    // "\x05READY" | nonce | tag as one 30-byte window: shift the 14 prefix bytes in
    uint32_t o[16] = {0};
    o[0] = hs_w4('\x05', 'R', 'E', 'A');
    o[1] = hs_w4('D', 'Y', 0, 0) | (n0 << 16);
    o[2] = (n0 >> 16) | (n1 << 16);
    o[3] = (n1 >> 16) | (head[4] << 16);
    o[4] = (head[4] >> 16) | (head[5] << 16);
    o[5] = (head[5] >> 16) | (head[6] << 16);
    o[6] = (head[6] >> 16) | (head[7] << 16);
    o[7] = head[7] >> 16;
    store_window(dst, 30, o);
}

} // namespace zmqg
