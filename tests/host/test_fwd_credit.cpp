// fwd_credit_admits / fwd_credit_taken / fwd_credit_dropped / fwd_credit_left
// (libzmq_amd/csrc/curve_fwd_credit.hpp) on the host under AddressSanitizer and
// UBSan (tests/test_fwd_credit_host.py).  dst_credit, dst_taken and dst_dropped
// each lie in a heap block of exactly their size, so one element read or
// written past either end is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../libzmq_amd/csrc/curve_fwd_credit.hpp"

using namespace zmqg;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
            ++failures;                                            \
        }                                                          \
    } while (0)

static const uint32_t UNL = 0xffffffffu;

// a heap block of exactly v.size() words
struct Exact {
    uint32_t *p;
    size_t n;
    explicit Exact(const std::vector<uint32_t> &v) : p((uint32_t *) malloc(4 * v.size())), n(v.size())
    {
        memcpy(p, v.data(), 4 * n);
    }
    ~Exact() { free(p); }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
};

// pipe_t's counters (src/pipe.cpp:207-234, :535-541); the peer reads nothing
struct Pipe {
    uint64_t hwm, written, read;
    bool check_hwm() const { return !(hwm > 0 && written - read >= hwm); }
};

// What the totals kernel does for every destination, and the verdict on each
// of its D deliveries, against a pipe with that credit
static void run_dst(const Exact &credit, Exact &taken, Exact &dropped, Exact &left, size_t t, uint32_t D,
                    uint32_t probe)
{
    const uint32_t c = credit.p[t];
    taken.p[t] = fwd_credit_taken(D, c);
    dropped.p[t] = fwd_credit_dropped(D, c);
    left.p[t] = fwd_credit_left(D, c);
    CHECK((uint64_t) taken.p[t] + dropped.p[t] == D);
    CHECK(taken.p[t] == (c == UNL || D < c ? D : c));
    CHECK(c == UNL ? left.p[t] == UNL : left.p[t] == c - taken.p[t] && left.p[t] <= c && left.p[t] != UNL);
    // the verdicts: the first `taken` ranks are admitted, the rest refused
    // (every rank when D is small, else the ranks around the edges)
    std::vector<uint32_t> ranks;
    if (D <= probe)
        for (uint32_t i = 0; i < D; ++i)
            ranks.push_back(i);
    else {
        const uint32_t at[] = {0u, 1u, taken.p[t] - 1u, taken.p[t], taken.p[t] + 1u, D - 2u, D - 1u};
        for (uint32_t i : at)
            if (i < D)
                ranks.push_back(i);
    }
    for (uint32_t i : ranks)
        CHECK(fwd_credit_admits(i, c) == (i < taken.p[t]));
    // pipe_t with hwm - (written - read) == credit: the i-th whole message is written iff check_hwm allows it
    if (D <= probe) {
        Pipe pipe = {c == UNL ? 0u : (uint64_t) c + 7u, 7u, 0u};
        uint32_t wrote = 0, refused = 0;
        for (uint32_t i = 0; i < D; ++i) {
            const bool ok = pipe.check_hwm();
            CHECK(ok == fwd_credit_admits(i, c));
            if (ok)
                ++pipe.written, ++wrote;
            else
                ++refused;
        }
        CHECK(wrote == taken.p[t] && refused == dropped.p[t]);
        CHECK(c == UNL || pipe.hwm - (pipe.written - pipe.read) == left.p[t]);
    }
}

static void test_edges()
{
    const uint32_t Ds[] = {0u, 1u, 2u, 5u, 64u, 257u};
    for (uint32_t D : Ds) {
        // credit 0, 1, D - 1, D, D + 1 and unlimited
        std::vector<uint32_t> c = {0u, 1u, D ? D - 1u : 0u, D, D + 1u, UNL};
        Exact credit(c), taken(std::vector<uint32_t>(c.size(), 0xdeadbeefu)),
            dropped(std::vector<uint32_t>(c.size(), 0xdeadbeefu)), left(std::vector<uint32_t>(c.size(), 0xdeadbeefu));
        for (size_t t = 0; t < c.size(); ++t)
            run_dst(credit, taken, dropped, left, t, D, 1000u);
        CHECK(taken.p[0] == 0 && dropped.p[0] == D && left.p[0] == 0);
        CHECK(taken.p[1] == (D ? 1u : 0u) && left.p[1] == (D ? 0u : 1u));
        CHECK(taken.p[3] == D && dropped.p[3] == 0 && left.p[3] == 0);
        CHECK(taken.p[4] == D && dropped.p[4] == 0 && left.p[4] == 1);
        CHECK(taken.p[5] == D && dropped.p[5] == 0 && left.p[5] == UNL);
        if (D) {
            CHECK(taken.p[2] == D - 1u && dropped.p[2] == 1u && left.p[2] == 0);
            CHECK(!fwd_credit_admits(D - 1u, D - 1u) && fwd_credit_admits(D - 1u, D) && fwd_credit_admits(D - 1u, UNL));
        }
    }
}

static void test_near_wrap()
{
    // counts up to 2^31 - 1 (the call's limit) and beyond, credits up to 2^32 - 2: no sum or difference wraps
    const uint32_t Ds[] = {0x7ffffffeu, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    const uint32_t Cs[] = {0u, 1u, 0x7ffffffeu, 0x7fffffffu, 0x80000000u, 0xfffffffdu, 0xfffffffeu, UNL};
    for (uint32_t D : Ds) {
        std::vector<uint32_t> c(Cs, Cs + sizeof Cs / sizeof *Cs);
        Exact credit(c), taken(std::vector<uint32_t>(c.size(), 0)), dropped(std::vector<uint32_t>(c.size(), 0)),
            left(std::vector<uint32_t>(c.size(), 0));
        for (size_t t = 0; t < c.size(); ++t)
            run_dst(credit, taken, dropped, left, t, D, 0u);
    }
    CHECK(fwd_credit_taken(0xffffffffu, 0xfffffffeu) == 0xfffffffeu);
    CHECK(fwd_credit_dropped(0xffffffffu, 0xfffffffeu) == 1u);
    CHECK(fwd_credit_left(0xffffffffu, 0xfffffffeu) == 0u && fwd_credit_left(0u, 0xfffffffeu) == 0xfffffffeu);
    CHECK(fwd_credit_left(0xffffffffu, UNL) == UNL && fwd_credit_taken(0xffffffffu, UNL) == 0xffffffffu);
    CHECK(fwd_credit_admits(0xfffffffeu, UNL) && fwd_credit_admits(0xfffffffdu, 0xfffffffeu) &&
          !fwd_credit_admits(0xfffffffeu, 0xfffffffeu));
    // consume over calls: the credit only falls, never below 0, never to the unlimited value
    uint32_t c = 0xfffffffeu;
    for (int call = 0; call < 8; ++call) {
        const uint32_t D = 0x7fffffffu, before = c;
        c = fwd_credit_left(D, c);
        CHECK(c <= before && c != UNL && before - c == fwd_credit_taken(D, before));
    }
    CHECK(c == 0u);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n)
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t) ((rng_state >> 33) % n);
}

// calls in sequence on one credit array with consume, the host refilling between them, against pipes
static void test_sweep()
{
    for (int it = 0; it < 300; ++it) {
        const size_t n = 1 + rnd(6);
        std::vector<uint32_t> c(n);
        std::vector<Pipe> pipes(n);
        for (size_t t = 0; t < n; ++t) {
            c[t] = rnd(4) == 0 ? UNL : rnd(6);
            pipes[t] = Pipe{c[t] == UNL ? 0u : (uint64_t) c[t] + 3u, 3u, 0u};
        }
        Exact credit(c), taken(std::vector<uint32_t>(n, 0)), dropped(std::vector<uint32_t>(n, 0));
        for (int call = 0; call < 5; ++call) {
            for (size_t t = 0; t < n; ++t) {
                const uint32_t D = rnd(8), before = credit.p[t];
                uint32_t wrote = 0;
                for (uint32_t i = 0; i < D; ++i) {
                    const bool ok = pipes[t].check_hwm();
                    CHECK(ok == fwd_credit_admits(i, before));
                    if (ok)
                        ++pipes[t].written, ++wrote;
                }
                taken.p[t] = fwd_credit_taken(D, before);
                dropped.p[t] = fwd_credit_dropped(D, before);
                credit.p[t] = fwd_credit_left(D, before);
                CHECK(taken.p[t] == wrote && dropped.p[t] == D - wrote);
                // the peer reads some: the host adds what it read
                const uint32_t got = rnd((uint32_t) (pipes[t].written - pipes[t].read) + 1u);
                pipes[t].read += got;
                if (credit.p[t] != UNL)
                    credit.p[t] += got;
                CHECK(pipes[t].hwm == 0 ? credit.p[t] == UNL
                                        : credit.p[t] == pipes[t].hwm - (pipes[t].written - pipes[t].read));
            }
        }
    }
}

int main()
{
    test_edges();
    test_near_wrap();
    test_sweep();
    if (failures)
        return 1;
    printf("fwd_credit ok\n");
    return 0;
}
