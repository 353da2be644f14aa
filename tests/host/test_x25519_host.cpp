// The device X25519 (libzmq_amd/csrc/curve_x25519.hpp) on the host: the header
// itself, unmodified, with the HIP qualifiers defined away, k_scalarmult and
// k_beforenm called one "thread" at a time through stub blockIdx / blockDim /
// threadIdx objects.  Reads lines of
//     scalar point expected rc [k | -]
// (hex; rc as libsodium returns it; k: crypto_box_beforenm's key, "-" where it
// fails, absent when the line is for k_scalarmult only) from the file named on
// the command line and compares.  Outputs and status are allocated for
// exactly n items and one block past the last one is "launched", so a write by
// a thread i >= n is a heap overflow.  Built with
// -fsanitize=address,undefined by tests/test_x25519_host.py; -DX25519_HPP
// names the header (a mutated copy, for the sensitivity runs).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#define __device__
#define __global__ static
#define __forceinline__ inline
#define __launch_bounds__(x)

struct stub_dim3 {
    unsigned x, y, z;
};
static stub_dim3 blockIdx = {0, 1, 1}, blockDim = {64, 1, 1}, threadIdx = {0, 1, 1};

namespace zmqg {

static inline uint32_t rotl(uint32_t v, int c)
{
    return (v << c) | (v >> (32 - c));
}

// HSalsa20 (the Salsa20/20 core without the feed-forward; words 0, 5, 10, 15
// and 6..9 of the state), restated from the Salsa20 specification
inline void hsalsa20(uint32_t out[8], const uint32_t k[8], const uint32_t in[4])
{
    uint32_t x[16] = {0x61707865, k[0], k[1], k[2], k[3], 0x3320646e, in[0], in[1],
                      in[2], in[3], 0x79622d32, k[4], k[5], k[6], k[7], 0x6b206574};
    static const int Q[8][4] = {{0, 4, 8, 12}, {5, 9, 13, 1}, {10, 14, 2, 6}, {15, 3, 7, 11},   // columns
                                {0, 1, 2, 3},  {5, 6, 7, 4},  {10, 11, 8, 9}, {15, 12, 13, 14}}; // rows
    for (int r = 0; r < 10; ++r)
        for (const auto &q : Q) {
            x[q[1]] ^= rotl(x[q[0]] + x[q[3]], 7);
            x[q[2]] ^= rotl(x[q[1]] + x[q[0]], 9);
            x[q[3]] ^= rotl(x[q[2]] + x[q[1]], 13);
            x[q[0]] ^= rotl(x[q[3]] + x[q[2]], 18);
        }
    const int pick[8] = {0, 5, 10, 15, 6, 7, 8, 9};
    for (int i = 0; i < 8; ++i)
        out[i] = x[pick[i]];
}

} // namespace zmqg

#ifndef X25519_HPP
#define X25519_HPP "../../libzmq_amd/csrc/curve_x25519.hpp"
#endif
#include X25519_HPP

static bool unhex(const char *s, uint8_t *out)
{
    if (strlen(s) != 64)
        return false;
    for (int i = 0; i < 32; ++i) {
        unsigned v;
        if (sscanf(s + 2 * i, "%2x", &v) != 1)
            return false;
        out[i] = (uint8_t) v;
    }
    return true;
}

static std::string hex(const uint8_t *p)
{
    char b[65];
    for (int i = 0; i < 32; ++i)
        snprintf(b + 2 * i, 3, "%02x", p[i]);
    return b;
}

struct Item {
    uint8_t scalar[32], point[32], expect[32], k[32];
    int rc;
    int has_k; // 0: no beforenm check, 1: k, 2: fails
};

// every thread of (n / 64 + 1) blocks of 64: at least one whole block of i >= n
template <typename F> static void launch(uint32_t n, F kernel)
{
    for (blockIdx.x = 0; blockIdx.x <= n / 64; ++blockIdx.x)
        for (threadIdx.x = 0; threadIdx.x < blockDim.x; ++threadIdx.x)
            kernel();
}

int main(int argc, char **argv)
{
    if (argc != 2)
        return fprintf(stderr, "usage: %s vectors.txt\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "r");
    if (!f)
        return perror(argv[1]), 2;
    std::vector<Item> items;
    char a[80], b[80], c[80], d[80], line[512];
    while (fgets(line, sizeof line, f)) {
        Item it;
        d[0] = 0;
        const int got = sscanf(line, "%79s %79s %79s %d %79s", a, b, c, &it.rc, d);
        if (got < 4 || !unhex(a, it.scalar) || !unhex(b, it.point) || !unhex(c, it.expect))
            return fprintf(stderr, "bad line %zu\n", items.size() + 1), 2;
        it.has_k = got < 5 ? 0 : strcmp(d, "-") == 0 ? 2 : 1;
        if (it.has_k == 1 && !unhex(d, it.k))
            return fprintf(stderr, "bad k on line %zu\n", items.size() + 1), 2;
        items.push_back(it);
    }
    fclose(f);
    int fails = 0;

    // k_scalarmult over every line; arrays of exactly n items
    {
        const uint32_t n = (uint32_t) items.size();
        uint8_t *sc = new uint8_t[32 * n], *pt = new uint8_t[32 * n], *out = new uint8_t[32 * n];
        int32_t *st = new int32_t[n];
        for (uint32_t i = 0; i < n; ++i) {
            memcpy(sc + 32 * i, items[i].scalar, 32);
            memcpy(pt + 32 * i, items[i].point, 32);
            st[i] = 7;
        }
        memset(out, 0x5a, 32 * n);
        launch(n, [&] { zmqg::k_scalarmult(n, sc, pt, out, st); });
        for (uint32_t i = 0; i < n; ++i)
            if (st[i] != items[i].rc || memcmp(out + 32 * i, items[i].expect, 32) != 0) {
                ++fails; // every failing line is named: the driver maps them to classes
                printf("scalarmult line %u: rc %d out %s, expected rc %d out %s\n", i + 1, st[i],
                       hex(out + 32 * i).c_str(), items[i].rc, hex(items[i].expect).c_str());
            }
        delete[] sc, delete[] pt, delete[] out, delete[] st;
    }

    // k_beforenm over the lines that carry a key (or "-")
    {
        std::vector<const Item *> sub;
        for (const Item &it : items)
            if (it.has_k)
                sub.push_back(&it);
        const uint32_t n = (uint32_t) sub.size();
        uint8_t *sk = new uint8_t[32 * n], *pk = new uint8_t[32 * n], *k = new uint8_t[32 * n];
        int32_t *st = new int32_t[n];
        for (uint32_t i = 0; i < n; ++i) {
            memcpy(sk + 32 * i, sub[i]->scalar, 32);
            memcpy(pk + 32 * i, sub[i]->point, 32);
            st[i] = 7;
        }
        memset(k, 0x5a, 32 * n);
        launch(n, [&] { zmqg::k_beforenm(n, pk, sk, k, st); });
        uint8_t untouched[32];
        memset(untouched, 0x5a, 32);
        for (uint32_t i = 0; i < n; ++i) {
            const bool fail = sub[i]->has_k == 2;
            if (st[i] != (fail ? -1 : 0) || memcmp(k + 32 * i, fail ? untouched : sub[i]->k, 32) != 0) {
                ++fails;
                printf("beforenm item %u: rc %d k %s, expected %s\n", i, st[i], hex(k + 32 * i).c_str(),
                       fail ? "rc -1, k untouched" : hex(sub[i]->k).c_str());
            }
        }
        printf("beforenm items %u\n", n);
        delete[] sk, delete[] pk, delete[] k, delete[] st;
    }

    if (fails)
        return printf("%d failures\n", fails), 1;
    printf("x25519 host ok %zu\n", items.size());
    return 0;
}
