// curve_handshake_client.hpp -- the client side of the CURVE handshake in
// batches: HELLO, WELCOME -> INITIATE, READY for many connections per call.
//
//   k_hc_hello    crypto_box_keypair + curve_client_tools_t::produce_hello
//                 (reference src/curve_client_tools.hpp:230-234, :29-65,
//                 src/curve_client.cpp:112-131)
//   k_hc_welcome  process_welcome + produce_initiate
//                 (src/curve_client_tools.hpp:67-199, src/curve_client.cpp:133-177)
//   k_hc_ready    curve_client_t::process_ready up to parse_metadata
//                 (src/curve_client.cpp:179-214)
//
// Not here: which command to send when, parse_metadata and ERROR commands
// (the host does them, as the reference's curve_client_t does).
//
// Work split, as k_hs_hello's (curve_handshake.hpp).  A HELLO needs two ladders
// that do not depend on each other -- C' = X25519(c', 9) and X25519(c', S) for
// the HELLO / WELCOME key k1 -- and so does a WELCOME once its box is open:
// X25519(c', S') for the connection's precom and X25519(c, S') for the vouch
// key.  (The reference runs three ladders on S' there; the INITIATE box's
// crypto_box(.., S', c') derives the precom a second time.)  A workgroup of two
// waves serves 64 connections: wave r runs ladder r for all 64 in one x25519()
// call whose inputs are selected by the wave index, the results cross through
// LDS, and wave 0 then does the HSalsa20s and the boxes, one lane per
// connection.  The WELCOME box opens under k1, which HELLO left in the state
// record, so wave 0 opens it before the ladders and hands S' to wave 1 through
// LDS.  READY is one open.
//
// The device has no RNG: c', the vouch nonce and the command nonces come in as
// arguments.  All stores are ordinary vector stores.
#pragma once

#include "curve_handshake.hpp"

namespace zmqg {

constexpr int32_t kHsErrMalformedReady = 0x10000016; // ZMQ_PROTOCOL_ERROR_ZMTP_MALFORMED_COMMAND_READY

constexpr uint32_t kHcState = 128, kHcHello = 200;
constexpr int kHcThreads = 128; // two waves: one per ladder

// one x25519() on words: q = X25519(s, p)
__device__ __forceinline__ void hc_ladder(uint32_t q[8], const uint32_t s[8], const uint32_t p[8])
{
    uint8_t sb[32], pb[32], qb[32];
    hs_words_to_bytes(sb, s);
    hs_words_to_bytes(pb, p);
    (void) x25519(qb, sb, pb);
    hs_bytes_to_words(q, qb);
}

// HELLO.  Connection i: server_pk[32 i ..] = S, cn_secret[32 i ..] = c',
// nonce[i].  Writes status[i], hello[200 i ..] and state[128 i ..] = C' | c' |
// k1 | S; both zero-filled where X25519(c', S) is all zero.
__global__ __launch_bounds__(kHcThreads) __attribute__((amdgpu_waves_per_eu(3))) void k_hc_hello(
    uint32_t n, const uint8_t *__restrict__ server_pk, const uint8_t *__restrict__ cn_secret,
    const unsigned long long *__restrict__ nonce, uint8_t *__restrict__ state, uint8_t *__restrict__ hello,
    int32_t *__restrict__ status)
{
    __shared__ uint32_t lds_q[2][8][64];  // ladder r's result, word-major: lanes hit distinct banks
    __shared__ uint32_t lds_keep[16][64]; // wave 0's c' and S
    const uint32_t lane = threadIdx.x & 63u, r = threadIdx.x >> 6; // r is wave-uniform
    const uint32_t i = blockIdx.x * 64u + lane;
    const bool live = i < n;
    // Ladder r: 0 X25519(c', 9), 1 X25519(c', S).  A lane past n runs the
    // ladder on zeros: every lane reaches the barrier.
    {
        uint32_t sw[8], pw[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            sw[k] = pw[k] = 0;
        if (live) {
            const uint32_t *cw = (const uint32_t *) (cn_secret + 32ull * i);
            const uint32_t *sv = (const uint32_t *) (server_pk + 32ull * i);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                sw[k] = cw[k];
                pw[k] = sv[k];
            }
        }
        // what wave 0 needs again after the ladder waits in LDS, not in
        // registers: the ladder then runs in k_beforenm's register budget
        if (r == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                lds_keep[k][lane] = sw[k];
                lds_keep[8 + k][lane] = pw[k];
                pw[k] = k == 0 ? 9u : 0u;
            }
        }
        uint32_t qw[8];
        hc_ladder(qw, sw, pw);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            lds_q[r][k][lane] = qw[k];
    }
    __syncthreads();
    if (r != 0 || !live)
        return;
    uint32_t *hel = (uint32_t *) (hello + (uint64_t) kHcHello * i);
    uint32_t *sta = (uint32_t *) (state + (uint64_t) kHcState * i);
    uint32_t q[8], d = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        q[k] = lds_q[1][k][lane];
        d |= q[k];
    }
    // an all-zero shared point (small-order S): crypto_box fails
    // (src/curve_client.cpp:118-120)
    if (d == 0) {
        status[i] = kHsErrCrypto;
        hs_zero_words(hel, kHcHello / 4);
        hs_zero_words(sta, kHcState / 4);
        return;
    }
    uint32_t k1[8];
    hs_beforenm_core(k1, q);
    const unsigned long long nn = nonce[i];
    const uint32_t n0 = bswap32((uint32_t) (nn >> 32)), n1 = bswap32((uint32_t) nn); // put_uint64: big endian
    // Box [64 * %x0](C'->S)
    uint32_t m[16], tag[4];
#pragma unroll
    for (int k = 0; k < 16; ++k)
        m[k] = 0;
    {
        const uint32_t bn[6] = {hs_w4('C', 'u', 'r', 'v'), hs_w4('e', 'Z', 'M', 'Q'), hs_w4('H', 'E', 'L', 'L'),
                                hs_w4('O', '-', '-', '-'), n0, n1};
        hs_seal_words<16>(k1, bn, m, tag);
    }
    // "\x05HELLO" 1 0 | 72 zero bytes | C' | short nonce | box
    hel[0] = hs_w4('\x05', 'H', 'E', 'L');
    hel[1] = hs_w4('L', 'O', '\x01', '\x00');
    hs_zero_words(hel + 2, 18);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t cp = lds_q[0][k][lane];
        hel[20 + k] = cp;
        sta[k] = cp;
        sta[8 + k] = lds_keep[k][lane];
        sta[16 + k] = k1[k];
        sta[24 + k] = lds_keep[8 + k][lane];
    }
    hel[28] = n0;
    hel[29] = n1;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        hel[30 + k] = tag[k];
#pragma unroll
    for (int k = 0; k < 16; ++k)
        hel[34 + k] = m[k];
    status[i] = 0;
}

// WELCOME -> INITIATE.  state[128 i ..] is what k_hc_hello wrote for the
// connection.  Writes status[i], precom_out[32 i ..] (zero on failure) and,
// for an accepted command only, the 257 + meta_len[i] bytes of the INITIATE.
__global__ __launch_bounds__(kHcThreads) __attribute__((amdgpu_waves_per_eu(3))) void k_hc_welcome(
    uint32_t n, const uint8_t *__restrict__ state, const uint8_t *__restrict__ client_pk,
    const uint8_t *__restrict__ client_sk, const uint64_t *__restrict__ cmd_off,
    const uint32_t *__restrict__ cmd_len, const uint8_t *__restrict__ cmd, const uint8_t *__restrict__ vouch_nonce,
    const unsigned long long *__restrict__ nonce, const uint64_t *__restrict__ meta_off,
    const uint32_t *__restrict__ meta_len, const uint8_t *__restrict__ meta, const uint64_t *__restrict__ out_off,
    uint8_t *__restrict__ out, uint8_t *__restrict__ precom_out, int32_t *__restrict__ status)
{
    __shared__ uint32_t lds_q[2][8][64];  // ladder r's result, word-major
    __shared__ uint32_t lds_sp[8][64];    // S', from wave 0's open to both ladders
    __shared__ uint32_t lds_keep[24][64]; // wave 0's cookie
    __shared__ int32_t lds_st[64];
    const uint32_t lane = threadIdx.x & 63u, r = threadIdx.x >> 6; // r is wave-uniform
    const uint32_t i = blockIdx.x * 64u + lane;
    const bool live = i < n;
    const uint32_t *sta = (const uint32_t *) (state + (uint64_t) kHcState * i);
    // Wave 0: the checks and the WELCOME open under k1 (no ladder needed).  A
    // connection that fails, or a lane past n, hands on S' = 0.
    if (r == 0) {
        int32_t st = 0;
        uint32_t pt[32];
#pragma unroll
        for (int k = 0; k < 32; ++k)
            pt[k] = 0;
        if (live) {
            const uint8_t *c = cmd + cmd_off[i];
            const uint32_t len = cmd_len[i];
            uint32_t w[16];
            hs_head(c, len, 8, w);
            // is_handshake_command (src/curve_client_tools.hpp:286-290); the
            // size check of process_welcome (:73-77) reports CRYPTOGRAPHIC
            // (src/curve_client.cpp:139-141)
            if (len < 8u || w[0] != hs_w4('\x07', 'W', 'E', 'L') || w[1] != hs_w4('C', 'O', 'M', 'E')) {
                st = kHsErrUnexpected;
            } else if (len != kHsWelcome) {
                st = kHsErrCrypto;
            } else {
                uint32_t k1[8], h[16], x[16];
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    k1[k] = sta[16 + k];
                load_window(c + 8, 32, h); // WELCOME nonce(16) | box tag(16)
                load_window(c + 40, 64, x);
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    pt[k] = x[k];
                load_window(c + 104, 64, x);
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    pt[16 + k] = x[k];
                const uint32_t bn[6] = {hs_w4('W', 'E', 'L', 'C'), hs_w4('O', 'M', 'E', '-'), h[0], h[1], h[2], h[3]};
                const uint32_t tag[4] = {h[4], h[5], h[6], h[7]};
                if (!hs_open_words<32>(k1, bn, tag, pt))
                    st = kHsErrCrypto;
            }
        }
        // plaintext: S'(32) | cookie(96)
#pragma unroll
        for (int k = 0; k < 8; ++k)
            lds_sp[k][lane] = st == 0 ? pt[k] : 0u;
#pragma unroll
        for (int k = 0; k < 24; ++k)
            lds_keep[k][lane] = pt[8 + k];
        lds_st[lane] = st;
    }
    __syncthreads();
    // Ladder r: 0 X25519(c', S'), 1 X25519(c, S')
    {
        uint32_t sw[8], pw[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            sw[k] = 0;
            pw[k] = lds_sp[k][lane];
        }
        if (live) {
            const uint32_t *sv = r == 0 ? sta + 8 : (const uint32_t *) (client_sk + 32ull * i);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                sw[k] = sv[k];
        }
        uint32_t qw[8];
        hc_ladder(qw, sw, pw);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            lds_q[r][k][lane] = qw[k];
    }
    __syncthreads();
    if (r != 0 || !live)
        return;
    int32_t st = lds_st[lane];
    uint32_t *pre_out = (uint32_t *) (precom_out + 32ull * i);
    uint32_t q0[8], q1[8], d0 = 0, d1 = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        q0[k] = lds_q[0][k][lane];
        q1[k] = lds_q[1][k][lane];
        d0 |= q0[k];
        d1 |= q1[k];
    }
    // an all-zero shared point (small-order S' inside a valid box): the
    // reference asserts on crypto_box_beforenm (src/curve_client_tools.hpp:
    // 105-106); a batch call reports it instead
    if (st == 0 && (d0 == 0 || d1 == 0))
        st = kHsErrCrypto;
    if (st != 0) {
        hs_zero_words(pre_out, 8);
        status[i] = st;
        return;
    }
    uint32_t pre[8];
    hs_beforenm_core(pre, q0);
    // INITIATE plaintext: C | vouch nonce | vouch box (tag | Box [C',S](C->S'))
    uint32_t pt[32];
    {
        const uint32_t *cw = (const uint32_t *) (client_pk + 32ull * i);
        const uint32_t *vw = (const uint32_t *) (vouch_nonce + 16ull * i);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            pt[k] = cw[k];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            pt[8 + k] = vw[k];
        uint32_t kv[8], v[16], tag[4];
        hs_beforenm_core(kv, q1);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            v[k] = sta[k];          // C'
            v[8 + k] = sta[24 + k]; // S
        }
        const uint32_t bn[6] = {hs_w4('V', 'O', 'U', 'C'), hs_w4('H', '-', '-', '-'), pt[8], pt[9], pt[10], pt[11]};
        hs_seal_words<16>(kv, bn, v, tag);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            pt[12 + k] = tag[k];
#pragma unroll
        for (int k = 0; k < 16; ++k)
            pt[16 + k] = v[k];
    }
    // Box [C + vouch + metadata](C'->S') under precom (:177 derives the same
    // key once more): the first 128 bytes from registers, the metadata
    // streamed from memory as k_hs_ready does
    const unsigned long long nn = nonce[i];
    const uint32_t n0 = bswap32((uint32_t) (nn >> 32)), n1 = bswap32((uint32_t) nn);
    const uint32_t bn[6] = {hs_w4('C', 'u', 'r', 'v'), hs_w4('e', 'Z', 'M', 'Q'), hs_w4('I', 'N', 'I', 'T'),
                            hs_w4('I', 'A', 'T', 'E'), n0, n1};
    HsBox b;
    hs_box_init(b, pre, bn);
    hs_xor_words<32>(b, pt);
    uint8_t *dst = out + out_off[i];
    fe h = fe_zero();
#pragma unroll
    for (int p = 0; p < 32; p += 16) {
        uint32_t y[16];
#pragma unroll
        for (int k = 0; k < 16; ++k)
            y[k] = pt[p + k];
        store_window(dst + 129 + 4 * p, 64, y);
        poly_absorb64(h, b.r, b.s1, b.s2, b.s3, b.s4, y, 64);
    }
    const uint32_t mlen = meta_len[i];
    const uint8_t *src = meta + meta_off[i];
    // message byte 128 + p0 is stream byte 160 + p0: the second half of
    // block 2, then whole blocks
    for (uint32_t w = 2; w == 2 ? mlen > 0u : 64u * w - 160u < mlen; ++w) {
        const uint32_t p0 = w == 2 ? 0u : 64u * w - 160u; // first metadata byte of this piece
        const uint32_t cap = w == 2 ? 32u : 64u;
        const int nv = (int) (mlen - p0 < cap ? mlen - p0 : cap);
        uint32_t ks[16], x[16], y[16];
        salsa20_block(ks, b.sub, b.n0, b.n1, w, 0);
        load_window(src + p0, nv, x);
#pragma unroll
        for (int k = 0; k < 16; ++k)
            y[k] = x[k] ^ (w == 2 ? (k < 8 ? ks[8 + k] : 0u) : ks[k]);
        mask_tail(y, nv);
        store_window(dst + 257 + p0, nv, y);
        poly_absorb64(h, b.r, b.s1, b.s2, b.s3, b.s4, y, nv);
    }
    uint32_t tag[4];
    poly_finish(h, b.pad, tag);
    // "\x08INITIATE" | cookie(96) | short nonce(8) | tag(16)
    {
        uint32_t o[16] = {0};
        o[0] = hs_w4('\x08', 'I', 'N', 'I');
        o[1] = hs_w4('T', 'I', 'A', 'T');
        o[2] = (uint32_t) 'E';
        store_window(dst, 9, o);
#pragma unroll
        for (int k = 0; k < 16; ++k)
            o[k] = lds_keep[k][lane];
        store_window(dst + 9, 64, o);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            o[k] = lds_keep[16 + k][lane];
        o[8] = n0;
        o[9] = n1;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            o[10 + k] = tag[k];
        o[14] = o[15] = 0;
        store_window(dst + 73, 56, o);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
        pre_out[k] = pre[k];
    status[i] = 0;
}

// READY: open Box [metadata](S'->C') under precom
__global__ __launch_bounds__(64) void k_hc_ready(uint32_t n, const uint8_t *__restrict__ precom,
                                                 const uint64_t *__restrict__ cmd_off,
                                                 const uint32_t *__restrict__ cmd_len,
                                                 const uint8_t *__restrict__ cmd,
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
    int32_t st = 0;
    do {
        // src/curve_client.cpp:65-78, :179-214
        uint32_t w[16];
        hs_head(c, len, 6, w);
        if (len < 6u || w[0] != hs_w4('\x05', 'R', 'E', 'A') || (w[1] & 0xffffu) != hs_w4('D', 'Y', 0, 0)) {
            st = kHsErrUnexpected;
            break;
        }
        if (len < 30u) {
            st = kHsErrMalformedReady;
            break;
        }
        const uint32_t *pw = (const uint32_t *) (precom + 32ull * i);
        uint32_t key[8], hd[16];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            key[k] = pw[k];
        load_window(c + 6, 24, hd); // short nonce(8) | tag(16)
        const uint32_t n0 = hd[0], n1 = hd[1];
        const uint32_t bn[6] = {hs_w4('C', 'u', 'r', 'v'), hs_w4('e', 'Z', 'M', 'Q'), hs_w4('R', 'E', 'A', 'D'),
                                hs_w4('Y', '-', '-', '-'), n0, n1};
        HsBox b;
        hs_box_init(b, key, bn);
        // the tag over the whole ciphertext before any byte is decrypted
        const uint32_t mlen = len - 30u;
        const uint8_t *ct = c + 30;
        fe acc = fe_zero();
        for (uint32_t p = 0; p < mlen; p += 64u) {
            const int nv = (int) (mlen - p < 64u ? mlen - p : 64u);
            uint32_t x[16];
            load_window(ct + p, nv, x);
            poly_absorb64(acc, b.r, b.s1, b.s2, b.s3, b.s4, x, nv);
        }
        uint32_t t[4];
        poly_finish(acc, b.pad, t);
        if ((t[0] ^ hd[2]) | (t[1] ^ hd[3]) | (t[2] ^ hd[4]) | (t[3] ^ hd[5])) {
            st = kHsErrCrypto;
            break;
        }
        uint8_t *dst = meta_out + meta_off[i];
        for (uint32_t wi = 0; wi == 0 ? mlen > 0u : 64u * wi - 32u < mlen; ++wi) {
            const uint32_t p0 = wi == 0 ? 0u : 64u * wi - 32u; // first message byte of this piece
            const uint32_t cap = wi == 0 ? 32u : 64u;
            const int nv = (int) (mlen - p0 < cap ? mlen - p0 : cap);
            uint32_t ks[16], x[16], y[16];
            if (wi > 0)
                salsa20_block(ks, b.sub, b.n0, b.n1, wi, 0);
            load_window(ct + p0, nv, x);
#pragma unroll
            for (int k = 0; k < 16; ++k)
                y[k] = x[k] ^ (wi == 0 ? (k < 8 ? b.ks0[k] : 0u) : ks[k]);
            mask_tail(y, nv);
            store_window(dst + p0, nv, y);
        }
        // get_uint64 (msg_data + 6): the value set_peer_nonce receives (:204)
        peer_nonce[i] = ((unsigned long long) bswap32(n0) << 32) | bswap32(n1);
        meta_len[i] = mlen;
        status[i] = 0;
        return;
    } while (0);
    peer_nonce[i] = 0;
    meta_len[i] = 0;
    status[i] = st;
}

} // namespace zmqg
