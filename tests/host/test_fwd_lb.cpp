// fwd_lb_range / fwd_lb_cur0 / fwd_lb_at / fwd_lb_pick
// (libzmq_amd/csrc/curve_fwd_lb.hpp) on the host under AddressSanitizer and
// UBSan (tests/test_fwd_lb_host.py).  grp_idx, lb_dst and lb_cur each lie in a
// heap block of exactly their size, so one element read past either end is
// reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../libzmq_amd/csrc/curve_fwd_lb.hpp"

using namespace zmqg;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
            ++failures;                                            \
        }                                                          \
    } while (0)

// a heap block of exactly v.size() words (none: one that must not be read at all)
struct Exact {
    uint32_t *p;
    size_t n;
    explicit Exact(const std::vector<uint32_t> &v) : p((uint32_t *) malloc(v.size() ? 4 * v.size() : 4)), n(v.size())
    {
        if (n)
            memcpy(p, v.data(), 4 * n);
        else { // no word of it is owned
            free(p);
            p = (uint32_t *) malloc(4) + 1;
        }
    }
    ~Exact() { free(n ? p : p - 1); }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
};

// lb_t with every write succeeding (src/lb.cpp:56-131): _pipes[_current] takes
// the part, and ++_current wraps at _active after the last part of a message
struct Lb {
    std::vector<uint32_t> pipes;
    uint32_t active, current;
    bool more;
    // the pipe the part is written to, or -1 without an active pipe
    int64_t sendpipe(bool part_more)
    {
        if (active == 0) // (:111-114)
            return -1;
        const uint32_t pipe = pipes[current]; // (:72)
        more = part_more;                     // (:118)
        if (!more && ++current >= active)     // (:119-124)
            current = 0;
        return pipe;
    }
};

// What the kernels do for one group, step by step: the group pass over the
// streams' message counts, then every message's pick.  Returns the new cursor.
static uint32_t run_group(const Exact &grp_idx, uint32_t g, uint32_t n_lb, const Exact &lb_dst, Exact &lb_cur,
                          const std::vector<uint32_t> &msgs, uint64_t n_dst, std::vector<uint32_t> &picked)
{
    const FwdLbRange r = fwd_lb_range(grp_idx.p[g], grp_idx.p[g + 1], n_lb);
    const uint32_t cur0 = fwd_lb_cur0(lb_cur.p[g], r.A);
    uint64_t before = 0;
    std::vector<uint32_t> first(msgs.size());
    for (size_t s = 0; s < msgs.size(); ++s) {
        first[s] = fwd_lb_at(cur0, before, r.A);
        before += msgs[s];
    }
    lb_cur.p[g] = fwd_lb_at(cur0, before, r.A);
    picked.clear();
    for (size_t s = 0; s < msgs.size(); ++s)
        for (uint32_t rank = 0; rank < msgs[s]; ++rank)
            picked.push_back(r.A ? fwd_lb_pick(lb_dst.p, r, fwd_lb_at(first[s], rank, r.A), n_dst) : kFwdLbNoPeer);
    return lb_cur.p[g];
}

static void test_range()
{
    FwdLbRange r = fwd_lb_range(2, 5, 10);
    CHECK(r.lo == 2 && r.A == 3);
    r = fwd_lb_range(2, 50, 10); // the upper entry above n_lb: clamped
    CHECK(r.lo == 2 && r.A == 8);
    r = fwd_lb_range(40, 50, 10); // both above
    CHECK(r.lo == 10 && r.A == 0);
    r = fwd_lb_range(0xffffffffu, 0xffffffffu, 0x7fffffffu);
    CHECK(r.lo == 0x7fffffffu && r.A == 0);
    r = fwd_lb_range(7, 3, 10); // a falling pair: empty
    CHECK(r.lo == 7 && r.A == 0);
    r = fwd_lb_range(0xffffffffu, 3, 10); // falling after the clamp
    CHECK(r.lo == 10 && r.A == 0);
    r = fwd_lb_range(4, 4, 10);
    CHECK(r.A == 0);
    r = fwd_lb_range(0, 0, 0);
    CHECK(r.lo == 0 && r.A == 0);
    r = fwd_lb_range(0, 0x7fffffffu, 0x7fffffffu);
    CHECK(r.lo == 0 && r.A == 0x7fffffffu);
}

static void test_cursor()
{
    const uint32_t As[] = {1u, 2u, 3u, 7u, 64u, 0x7fffffffu};
    for (uint32_t A : As) {
        CHECK(fwd_lb_cur0(0, A) == 0);
        CHECK(fwd_lb_cur0(A - 1, A) == A - 1);
        CHECK(fwd_lb_cur0(A, A) == 0);
        CHECK(fwd_lb_cur0(0xffffffffu, A) == (uint32_t) (0xffffffffull % A));
        CHECK(fwd_lb_at(A - 1, 1, A) == 0);
        CHECK(fwd_lb_at(0, 0, A) == 0);
    }
    CHECK(fwd_lb_cur0(0, 0) == 0 && fwd_lb_cur0(5, 0) == 0 && fwd_lb_cur0(0xffffffffu, 0) == 0);
    CHECK(fwd_lb_at(0, 12345, 0) == 0 && fwd_lb_at(0, ~0ull >> 2, 0) == 0);
    CHECK(fwd_lb_at(0, 5, 1) == 0 && fwd_lb_at(0, 0x7fffffffull, 1) == 0);
    // a cursor near 2^31 plus counts up to 2^31 - 1: a 32-bit sum would wrap
    const uint32_t A = 0x7fffffffu, pos = 0x7ffffffeu;
    CHECK(fwd_lb_at(pos, 0x7fffffffull, A) == pos);                     // a whole turn of the ring
    CHECK(fwd_lb_at(pos, 0x7ffffffeull, A) == pos - 1u);
    CHECK(fwd_lb_at(pos, 2, A) == 1u);
    CHECK(fwd_lb_at(0x7ffffff0u, 0x7fffffffull, 0x7ffffff1u) == (uint32_t) ((0x7ffffff0ull + 0x7fffffffull) % 0x7ffffff1ull));
    // (32-bit: 0x7ffffff0 + 0x7fffffff = 0xffffffef, no wrap yet; two such counts do)
    CHECK(fwd_lb_at(0x7ffffff0u, 2 * 0x7fffffffull, 0x7ffffff1u) ==
          (uint32_t) ((0x7ffffff0ull + 2 * 0x7fffffffull) % 0x7ffffff1ull));
    CHECK(fwd_lb_at(6, 0x100000000ull, 7) == (uint32_t) ((6ull + 0x100000000ull) % 7ull)); // (a truncated add gives 6)
    CHECK(fwd_lb_at(6, (1ull << 62) - 1ull, 7) == (uint32_t) ((6ull + ((1ull << 62) - 1ull)) % 7ull));
    // streams of 2^31 - 1 messages each, summed as the group pass sums them
    uint64_t before = 0;
    const uint32_t cur0 = fwd_lb_cur0(0xffffffffu, 0x7ffffffdu);
    for (int s = 0; s < 64; ++s) {
        CHECK(fwd_lb_at(cur0, before, 0x7ffffffdu) == (uint32_t) (((uint64_t) cur0 + before) % 0x7ffffffdull));
        before += 0x7fffffffull;
    }
}

static void test_pick_bounds()
{
    // three groups over five entries; the third group's range is cut by n_lb
    Exact grp_idx(std::vector<uint32_t>{0, 2, 2, 9}), lb_dst(std::vector<uint32_t>{4, 1, 7, 0xffffffffu, 2});
    const uint32_t n_lb = 5;
    FwdLbRange r = fwd_lb_range(grp_idx.p[0], grp_idx.p[1], n_lb);
    CHECK(r.A == 2 && fwd_lb_pick(lb_dst.p, r, 0, 8) == 4 && fwd_lb_pick(lb_dst.p, r, 1, 8) == 1);
    CHECK(fwd_lb_pick(lb_dst.p, r, 0, 4) == kFwdLbNoPeer); // an entry at n_dst names no destination
    r = fwd_lb_range(grp_idx.p[1], grp_idx.p[2], n_lb);
    CHECK(r.A == 0);
    r = fwd_lb_range(grp_idx.p[2], grp_idx.p[3], n_lb);
    CHECK(r.lo == 2 && r.A == 3);
    CHECK(fwd_lb_pick(lb_dst.p, r, 0, 8) == 7 && fwd_lb_pick(lb_dst.p, r, 1, 8) == kFwdLbNoPeer &&
          fwd_lb_pick(lb_dst.p, r, 2, 8) == 2); // the last word of the block
    // n_lb below the array's length: the range ends there
    r = fwd_lb_range(0, 9, 1);
    CHECK(r.A == 1 && fwd_lb_pick(lb_dst.p, r, fwd_lb_at(fwd_lb_cur0(77, r.A), 5, r.A), 8) == 4);
    // an empty table: nothing is read
    Exact none(std::vector<uint32_t>{});
    r = fwd_lb_range(3, 9, 0);
    CHECK(r.A == 0 && none.n == 0);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n)
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t) ((rng_state >> 33) % n);
}

// calls in sequence on one table, the cursor carried on the "device", against lb_t
static void test_sweep()
{
    for (int it = 0; it < 400; ++it) {
        const uint32_t A = rnd(9), n_dst = 1 + rnd(6), pad_lo = rnd(3), pad_hi = rnd(3);
        std::vector<uint32_t> dst(pad_lo + A + pad_hi);
        for (uint32_t &d : dst)
            d = rnd(n_dst + 2); // (some name no destination)
        const uint32_t n_lb = (uint32_t) dst.size();
        // group 1 of three is the one under test; its upper entry may overshoot when nothing lies behind it
        const uint32_t hi = pad_hi == 0 && rnd(2) ? 0xfffffff0u : pad_lo + A;
        Exact grp_idx(std::vector<uint32_t>{0, pad_lo, hi, n_lb}), lb_dst(dst);
        const uint32_t starts[] = {0, A ? A - 1 : 0, A, 0xffffffffu, rnd(1000)};
        Exact lb_cur(std::vector<uint32_t>{11, starts[rnd(5)], 13});
        Lb lb;
        lb.pipes.assign(dst.begin() + pad_lo, dst.begin() + pad_lo + A);
        lb.active = A;
        lb.current = fwd_lb_cur0(lb_cur.p[1], A); // (the clamp is this project's; lb_t keeps _current < _active itself)
        lb.more = false;
        for (int call = 0; call < 4; ++call) {
            std::vector<uint32_t> msgs(rnd(5));
            for (uint32_t &m : msgs)
                m = rnd(2) ? rnd(4) : rnd(3 * (A + 1));
            std::vector<uint32_t> want, got;
            for (uint32_t m : msgs)
                for (uint32_t i = 0; i < m; ++i) {
                    const uint32_t parts = 1 + rnd(3);
                    int64_t to = -2;
                    for (uint32_t k = 0; k < parts; ++k) {
                        const int64_t t = lb.sendpipe(k + 1 < parts);
                        CHECK(to == -2 || to == t); // every part of a message to one pipe
                        to = t;
                    }
                    want.push_back(to >= 0 && (uint64_t) to < n_dst ? (uint32_t) to : kFwdLbNoPeer);
                }
            const uint32_t cur = run_group(grp_idx, 1, n_lb, lb_dst, lb_cur, msgs, n_dst, got);
            CHECK(got == want);
            CHECK(cur == (A ? lb.current : 0u) && !lb.more);
            CHECK(lb_cur.p[0] == 11 && lb_cur.p[2] == 13);
        }
    }
}

int main()
{
    test_range();
    test_cursor();
    test_pick_bounds();
    test_sweep();
    if (failures)
        return 1;
    printf("fwd_lb ok\n");
    return 0;
}
