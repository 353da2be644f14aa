// DevArena / DevBuf / grown_cap (libzmq_amd/csrc/curve_devbuf.hpp) on a counting
// malloc policy that fails the k-th allocation on request.  The group below is
// built the way ensure_workspace builds the context's (curve_ctx.hpp): one
// capacity, set to 0 while its members are reserved, members of several element
// types and multipliers, a fixed-size member, members reserved only under a
// condition, one sized exactly by the call and one by the doubling policy.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../libzmq_amd/csrc/curve_devbuf.hpp"

using namespace zmqg;

#define REQUIRE(c)                                                    \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

struct CountMem {
    typedef int stream_t;
    typedef int error_t;
    static std::map<void *, size_t> live; // pointer -> bytes
    static size_t live_bytes, peak_bytes, allocs, fail_at; // fail_at: the allocation (counted from 1) that fails, 0 = none

    static int alloc_async(void **p, size_t bytes, int)
    {
        if (++allocs == fail_at)
            return 2;
        *p = malloc(bytes);
        REQUIRE(*p);
        live[*p] = bytes;
        live_bytes += bytes;
        peak_bytes = std::max(peak_bytes, live_bytes);
        return 0;
    }
    static int free_async(void *p, int)
    {
        free_now(p);
        return 0;
    }
    static void free_now(void *p)
    {
        REQUIRE(live.count(p));
        live_bytes -= live[p];
        live.erase(p);
        free(p);
    }
    static void reset()
    {
        REQUIRE(live.empty() && live_bytes == 0);
        peak_bytes = allocs = fail_at = 0;
    }
};
std::map<void *, size_t> CountMem::live;
size_t CountMem::live_bytes, CountMem::peak_bytes, CountMem::allocs, CountMem::fail_at;

typedef DevArena<CountMem> Arena;

struct Rec96 {
    char b[96];
};

struct Group {
    uint64_t cap = 0;
    DevBuf<Rec96> hot;               // [cap]
    DevBuf<uint32_t> powtab;         // [cap * 125]
    DevBuf<unsigned long long> acc;  // [cap * 5]
    DevBuf<uint8_t> flag;            // [cap]
    DevBuf<uint64_t> rec;            // [512], whatever cap is
    DevBuf<uint32_t> perm;           // [cap], only when `sorts`
    DevBuf<uint8_t, 0> temp;         // doubled from 4096, only when `sorts`
    DevBuf<unsigned long long, 0> rt; // exactly what the call needs
};

#define CHECK(expr)      \
    do {                 \
        if ((expr) != 0) \
            return -5;   \
    } while (0)

const size_t kSessions = 3;
size_t rt_need(uint64_t n) { return ((n + 255) / 256 + 2) * kSessions; }
size_t temp_need(uint64_t n) { return 4 * n; } // (1024 frames: the floor; 1025: it doubles)

int ensure(Arena &a, Group &g, uint64_t n, bool sorts)
{
    if (n > g.cap) {
        const uint64_t cap = grown_cap(g.cap, 1024, n);
        g.cap = 0;
        CHECK(g.hot.reserve(a, cap, 0));
        CHECK(g.powtab.reserve(a, cap * 125, 0));
        CHECK(g.acc.reserve(a, cap * 5, 0));
        CHECK(g.flag.reserve(a, cap, 0));
        CHECK(g.rec.reserve(a, 512, 0));
        if (sorts)
            CHECK(g.perm.reserve(a, cap, 0));
        g.cap = cap;
    }
    if (sorts)
        CHECK(g.temp.reserve(a, grown_cap(g.temp.count, 4096, temp_need(n)), 0));
    CHECK(g.rt.reserve(a, rt_need(n), 0));
    return 0;
}

// One member: {null, 0}, or an array the arena holds whose bytes cover `count`
// elements and the slack, with `count` one that a reserve asked for (the size
// for the old capacity or for the new one).
template <class T, size_t S>
void check_member(const DevBuf<T, S> &b, size_t old_count, size_t new_count, std::vector<void *> &nonnull)
{
    if (!b.p) {
        REQUIRE(b.count == 0);
        return;
    }
    REQUIRE(b.count == old_count || b.count == new_count);
    REQUIRE(CountMem::live.count(b.p) && CountMem::live[b.p] == b.count * sizeof(T) + S);
    ((volatile char *) b.p)[b.count * sizeof(T) + S - 1] = 1; // the last byte is ours (AddressSanitizer)
    nonnull.push_back(b.p);
}

// every member against the two capacities it may be sized for; the arena's
// live set is exactly the non-null members
void check_group(const Arena &a, const Group &g, uint64_t oc, uint64_t on, uint64_t nc, uint64_t nn, bool sorts)
{
    std::vector<void *> m;
    check_member(g.hot, oc, nc, m);
    check_member(g.powtab, oc * 125, nc * 125, m);
    check_member(g.acc, oc * 5, nc * 5, m);
    check_member(g.flag, oc, nc, m);
    check_member(g.rec, 512, 512, m);
    check_member(g.perm, oc, nc, m);
    check_member(g.temp, grown_cap(0, 4096, temp_need(on)), grown_cap(0, 4096, temp_need(nn)), m);
    check_member(g.rt, rt_need(on), rt_need(nn), m);
    if (!sorts)
        REQUIRE(!g.perm.p && !g.temp.p);
    std::vector<void *> held = a.held;
    std::sort(held.begin(), held.end());
    std::sort(m.begin(), m.end());
    REQUIRE(held == m);
    REQUIRE(CountMem::live.size() == m.size());
}

// after a success: the capacity, and every member sized for it
void check_grown(const Group &g, uint64_t cap, bool sorts)
{
    REQUIRE(g.cap == cap);
    REQUIRE(g.hot.count >= cap && g.powtab.count >= cap * 125 && g.acc.count >= cap * 5 && g.flag.count >= cap &&
            g.rec.count >= 512);
    REQUIRE(!sorts || g.perm.count >= cap);
}

void test_policy()
{
    REQUIRE(grown_cap(0, 1024, 8) == 1024 && grown_cap(0, 1024, 1024) == 1024 && grown_cap(1024, 1024, 1025) == 2048);
    REQUIRE(grown_cap(2048, 1024, 8) == 2048 && grown_cap(0, 64, 65) == 128 && grown_cap(0, 4096, 1) == 4096);
    REQUIRE(grown_cap(0, 65536, 65537) == 131072 && grown_cap(4096, 4096, 20000) == 32768);
    REQUIRE(grown_cap(0, 4096, 0) == 0 && grown_cap(8192, 4096, 5) == 8192); // what fits stays as it is
}

void test_grow_and_shrink(bool sorts)
{
    CountMem::reset();
    Arena a;
    Group g;
    REQUIRE(ensure(a, g, 8, sorts) == 0);
    check_grown(g, 1024, sorts);
    check_group(a, g, 1024, 8, 1024, 8, sorts);
    uint32_t *const as_pointer = g.powtab; // (a DevBuf reads as its pointer)
    REQUIRE(as_pointer == g.powtab.p);
    REQUIRE(ensure(a, g, 1025, sorts) == 0);
    check_grown(g, 2048, sorts);
    check_group(a, g, 2048, 1025, 2048, 1025, sorts);
    REQUIRE(g.rt.count == rt_need(1025)); // exactly the need
    const size_t allocs = CountMem::allocs;
    const Group before = g;
    REQUIRE(ensure(a, g, 8, sorts) == 0); // fits: nothing moves
    REQUIRE(CountMem::allocs == allocs && g.hot.p == before.hot.p && g.rt.p == before.rt.p && g.cap == 2048);
    check_group(a, g, 2048, 1025, 2048, 1025, sorts);
    a.free_all();
    REQUIRE(CountMem::live.empty() && CountMem::live_bytes == 0 && a.held.empty());
}

void test_failures(bool sorts)
{
    // the sequence without a failure: its allocations and its peak
    CountMem::reset();
    size_t growth_allocs, peak;
    {
        Arena a;
        Group g;
        REQUIRE(ensure(a, g, 1024, sorts) == 0);
        const size_t before = CountMem::allocs;
        REQUIRE(ensure(a, g, 1025, sorts) == 0);
        growth_allocs = CountMem::allocs - before;
        peak = CountMem::peak_bytes;
        a.free_all();
    }
    REQUIRE(growth_allocs == (sorts ? 7u : 5u)); // hot, powtab, acc, flag, rt, and perm, temp
    for (size_t k = 1; k <= growth_allocs; ++k) {
        CountMem::reset();
        Arena a;
        Group g;
        REQUIRE(ensure(a, g, 1024, sorts) == 0);
        CountMem::fail_at = CountMem::allocs + k;
        REQUIRE(ensure(a, g, 1025, sorts) != 0);
        // (a failure after the capacity group is a failure of temp or rt: the group itself stands)
        const size_t in_group = sorts ? 5 : 4;
        REQUIRE(g.cap == (k <= in_group ? 0u : 2048u));
        check_group(a, g, 1024, 1024, 2048, 1025, sorts);
        CountMem::fail_at = 0;
        REQUIRE(ensure(a, g, 1025, sorts) == 0);
        check_grown(g, 2048, sorts);
        check_group(a, g, 2048, 1025, 2048, 1025, sorts);
        REQUIRE(g.rt.count == rt_need(1025));
        REQUIRE(CountMem::peak_bytes <= peak);
        a.free_all();
        REQUIRE(CountMem::live.empty() && CountMem::live_bytes == 0);
    }
}

int main()
{
    test_policy();
    for (int sorts = 0; sorts < 2; ++sorts) {
        test_grow_and_shrink(sorts != 0);
        test_failures(sorts != 0);
    }
    CountMem::reset();
    printf("devbuf ok\n");
    return 0;
}
