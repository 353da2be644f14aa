// fwd_lbc_dist / fwd_lbc_full_at / fwd_lbc_visits / fwd_lbc_left /
// fwd_lbc_deactivate / fwd_lbc_orig (libzmq_amd/csrc/curve_fwd_lb_credit.hpp) on
// the host under AddressSanitizer and UBSan (tests/test_fwd_lb_credit_host.py):
// a sequential driver that walks a group in epochs, as k_fwd_lb_credit_groups
// does with a workgroup, against lb_t's loop taken message by message
// (src/lb.cpp:56-131, the deactivation at :103-107).  The ring, the credits and
// the working arrays each lie in a heap block of exactly their size.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../libzmq_amd/csrc/curve_fwd_lb_credit.hpp"

using namespace zmqg;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
            ++failures;                                            \
        }                                                          \
    } while (0)

static const uint32_t UNL = 0xffffffffu, BIG = 0xfffffffeu, REFUSED = kFwdLbRefused;

// a heap block of exactly n words
struct Exact {
    uint32_t *p;
    size_t n;
    explicit Exact(size_t n_) : p((uint32_t *) malloc(4 * (n_ ? n_ : 1))), n(n_) {}
    explicit Exact(const std::vector<uint32_t> &v) : p((uint32_t *) malloc(4 * (v.size() ? v.size() : 1))), n(v.size())
    {
        if (n)
            memcpy(p, v.data(), 4 * n);
    }
    ~Exact() { free(p); }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
};

struct Result {
    std::vector<uint32_t> pick; // per message: the ring's original position, or REFUSED
    std::vector<uint32_t> sent; // per original position: the messages it took
    uint32_t cur;               // the original position the cursor points at, 0 for an empty ring
};

// The header's loop, literally
static Result literal(const Exact &credit, uint32_t cur0, uint32_t M)
{
    const uint32_t A0 = (uint32_t) credit.n;
    Exact orig(A0), w(credit.n);
    for (uint32_t j = 0; j < A0; ++j)
        orig.p[j] = j, w.p[j] = credit.p[j];
    Result r;
    r.sent.assign(A0, 0u);
    uint32_t A = A0, cur = cur0;
    for (uint32_t i = 0; i < M; ++i) {
        uint32_t to = REFUSED;
        while (A > 0) {
            if (w.p[cur] == UNL || w.p[cur] > 0) {
                to = orig.p[cur];
                if (w.p[cur] != UNL)
                    --w.p[cur];
                if (++cur >= A)
                    cur = 0;
                break;
            }
            A -= 1;
            if (cur < A) {
                const uint32_t o = orig.p[cur], c = w.p[cur];
                orig.p[cur] = orig.p[A], w.p[cur] = w.p[A];
                orig.p[A] = o, w.p[A] = c;
            } else
                cur = 0;
        }
        r.pick.push_back(to);
        if (to != REFUSED)
            ++r.sent[to];
    }
    r.cur = A ? orig.p[cur] : 0u;
    return r;
}

// k_fwd_lb_credit_groups' walk, one lane
static Result epochs(const Exact &credit, uint32_t cur0, uint32_t M, uint32_t *n_epochs)
{
    const uint32_t A0 = (uint32_t) credit.n;
    Exact orig(A0), w(credit.n);
    for (uint32_t j = 0; j < A0; ++j)
        orig.p[j] = j, w.p[j] = credit.p[j];
    Result r;
    r.sent.assign(A0, 0u);
    r.pick.assign(M, 0x55555555u);
    uint32_t A = A0, cur = cur0, done = 0;
    *n_epochs = 0;
    if (A0 == 0) {
        r.pick.assign(M, REFUSED);
        r.cur = 0;
        return r;
    }
    for (;;) {
        ++*n_epochs;
        const uint32_t rem = M - done;
        if (A == 0) {
            for (uint32_t i = 0; i < rem; ++i)
                r.pick[done + i] = REFUSED;
            cur = 0;
            break;
        }
        uint64_t L = kFwdLbNever;
        for (uint32_t j = 0; j < A; ++j) {
            const uint64_t f = fwd_lbc_full_at(fwd_lbc_dist(j, cur, A), w.p[j], A);
            L = f < L ? f : L;
        }
        const bool last = rem <= L;
        const uint32_t n = last ? rem : (uint32_t) L;
        for (uint32_t i = 0; i < n; ++i)
            r.pick[done + i] = fwd_lbc_orig(orig.p[fwd_lb_at(cur, i, A)], A0);
        for (uint32_t j = 0; j < A; ++j) {
            const uint32_t v = fwd_lbc_visits(n, fwd_lbc_dist(j, cur, A), A);
            if (v) {
                CHECK(w.p[j] == UNL || v <= w.p[j]);
                r.sent[fwd_lbc_orig(orig.p[j], A0)] += v;
                w.p[j] = fwd_lbc_left(w.p[j], v);
            }
        }
        if (last) {
            cur = fwd_lb_at(cur, rem, A);
            break;
        }
        const uint32_t js = fwd_lb_at(cur, L, A);
        CHECK(w.p[js] == 0); // the entry that is found full
        FwdLbRing ring = {A, cur};
        if (fwd_lbc_deactivate(ring, js)) {
            const uint32_t o = orig.p[js], c = w.p[js];
            orig.p[js] = orig.p[ring.A], w.p[js] = w.p[ring.A];
            orig.p[ring.A] = o, w.p[ring.A] = c;
        }
        A = ring.A, cur = ring.cur, done += n;
    }
    r.cur = A ? fwd_lbc_orig(orig.p[cur], A0) : 0u;
    return r;
}

static uint64_t small_sum(const std::vector<uint32_t> &c)
{
    uint64_t s = 0;
    for (uint32_t x : c)
        s += x < 16u ? x : 0u;
    return s;
}

static void run(const std::vector<uint32_t> &c, uint32_t cur0, uint32_t M)
{
    Exact credit(c);
    uint32_t n_epochs = 0;
    const Result a = literal(credit, cur0, M), b = epochs(credit, cur0, M, &n_epochs);
    CHECK(a.pick == b.pick);
    CHECK(a.sent == b.sent);
    CHECK(a.cur == b.cur);
    CHECK(n_epochs <= c.size() + 1u);
    for (size_t j = 0; j < c.size(); ++j) // an entry takes at most its credit
        CHECK(c[j] == UNL || b.sent[j] <= c[j]);
}

// every cursor, M from 0 to the sum of the small credits + 3
static void sweep(const std::vector<uint32_t> &c, const std::vector<uint32_t> &cursors)
{
    const uint32_t top = (uint32_t) small_sum(c) + 3u;
    for (uint32_t cur0 : cursors)
        for (uint32_t M = 0; M <= top; ++M)
            run(c, cur0, M);
}

static std::vector<uint32_t> all_cursors(size_t A)
{
    std::vector<uint32_t> v;
    for (uint32_t i = 0; i < A; ++i)
        v.push_back(i);
    return v;
}

static const uint32_t kCredits[] = {0u, 1u, 2u, UNL, BIG};

static void test_small_rings()
{
    // rings of 1, 2 and 3 entries: every combination of the five credits
    for (size_t A = 1; A <= 3; ++A) {
        size_t combos = 1;
        for (size_t k = 0; k < A; ++k)
            combos *= 5;
        for (size_t x = 0; x < combos; ++x) {
            std::vector<uint32_t> c(A);
            size_t y = x;
            for (size_t k = 0; k < A; ++k, y /= 5)
                c[k] = kCredits[y % 5];
            sweep(c, all_cursors(A));
        }
    }
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n)
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t) ((rng_state >> 33) % n);
}

static void test_large_rings()
{
    const size_t sizes[] = {64, 65, 257};
    for (size_t A : sizes) {
        // every entry finite and small: the ring empties (every cursor up to 65 entries; five cursors at 257,
        // where a full sweep is 257 * 260 walks of up to 257 epochs)
        std::vector<uint32_t> c(A);
        for (size_t j = 0; j < A; ++j)
            c[j] = A > 65 ? rnd(2) : rnd(3);
        std::vector<uint32_t> cursors = all_cursors(A);
        if (A > 65)
            cursors = {0u, 1u, (uint32_t) A / 2u, (uint32_t) A - 2u, (uint32_t) A - 1u};
        sweep(c, cursors);
        // a few finite entries among entries that never run out, every cursor
        for (int it = 0; it < 3; ++it) {
            for (size_t j = 0; j < A; ++j)
                c[j] = rnd(2) ? UNL : BIG;
            for (int k = 0; k < 6; ++k)
                c[rnd((uint32_t) A)] = rnd(3);
            c[it == 0 ? 63 : it == 1 ? 64 % A : A - 1] = 0; // lane 63, lane 0 of the second step, the last position
            sweep(c, all_cursors(A));
        }
        // zeros side by side: deactivations with no message between
        for (size_t j = 0; j < A; ++j)
            c[j] = j % 7 == 3 || j % 7 == 4 ? 0u : j % 5 == 0 ? 1u : UNL;
        sweep(c, all_cursors(A));
    }
}

static void test_random()
{
    for (int it = 0; it < 20000; ++it) {
        const size_t A = 1 + rnd(9);
        std::vector<uint32_t> c(A);
        for (size_t j = 0; j < A; ++j)
            c[j] = rnd(5) == 0 ? UNL : rnd(4);
        run(c, rnd((uint32_t) A), rnd((uint32_t) small_sum(c) + 6u));
    }
    run(std::vector<uint32_t>(), 0u, 5u); // an empty ring refuses everything
}

// The 64-bit arithmetic alone, at the largest ring and the largest finite credit
static void test_wide()
{
    const uint32_t A = 0x7fffffffu, w = BIG;
    const unsigned __int128 one = 1;
    for (uint32_t d : {0u, 1u, A - 2u, A - 1u}) {
        const uint64_t f = fwd_lbc_full_at(d, w, A);
        CHECK((unsigned __int128) f == d + (one * w) * A && f < (1ull << 63));
        CHECK(fwd_lbc_visits(f, d, A) == w);          // every visit before the one that finds it full
        CHECK(fwd_lbc_visits(f + 1u, d, A) == w + 1u); // (that visit itself: never asked for, and still no wrap)
        CHECK(fwd_lbc_visits(f - A, d, A) == w - 1u);
        CHECK(fwd_lbc_visits(d, d, A) == 0u && fwd_lbc_visits(d + 1ull, d, A) == 1u);
        CHECK(fwd_lbc_visits((uint64_t) d + A, d, A) == 1u && fwd_lbc_visits((uint64_t) d + A + 1u, d, A) == 2u);
        CHECK(fwd_lbc_left(w, fwd_lbc_visits(f, d, A)) == 0u);
        CHECK(fwd_lb_at(5u % A, f, A) == (uint32_t) ((5u + (unsigned __int128) f) % A));
    }
    CHECK(fwd_lbc_full_at(0u, UNL, A) == kFwdLbNever && fwd_lbc_left(UNL, 77u) == UNL);
    CHECK(fwd_lbc_full_at(A - 1u, 0u, A) == A - 1u);
    // distances at the ends of the largest ring
    CHECK(fwd_lbc_dist(0u, A - 1u, A) == 1u && fwd_lbc_dist(A - 1u, 0u, A) == A - 1u);
    CHECK(fwd_lbc_dist(A - 1u, A - 1u, A) == 0u && fwd_lbc_dist(A - 2u, A - 1u, A) == A - 1u);
    // the 32-bit and the 64-bit branch of the visits agree across 2^32
    for (uint64_t n : {0xfffffffeull, 0xffffffffull, 0x100000000ull, 0x100000001ull, 0x1fffffffeull})
        for (uint32_t a : {2u, 3u, 0x10000u, A})
            for (uint32_t d = 0; d < 2u; ++d)
                CHECK(fwd_lbc_visits(n, d, a) == (uint32_t) ((n - d - 1u) / a) + 1u);
    // the swap rule
    FwdLbRing r = {4u, 1u};
    CHECK(fwd_lbc_deactivate(r, 1u) && r.A == 3u && r.cur == 1u);
    CHECK(!fwd_lbc_deactivate(r, 2u) && r.A == 2u && r.cur == 0u);
    CHECK(fwd_lbc_deactivate(r, 0u) && r.A == 1u && r.cur == 0u);
    CHECK(!fwd_lbc_deactivate(r, 0u) && r.A == 0u && r.cur == 0u);
    CHECK(fwd_lbc_orig(3u, 4u) == 3u && fwd_lbc_orig(4u, 4u) == 0u && fwd_lbc_orig(0xffffffffu, 4u) == 0u);
}

int main()
{
    test_small_rings();
    test_large_rings();
    test_random();
    test_wide();
    if (failures)
        return 1;
    printf("fwd_lb_credit ok\n");
    return 0;
}
