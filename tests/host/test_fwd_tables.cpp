// fwd_table_dims / fwd_table_fill (libzmq_amd/csrc/curve_fwd_common.hpp), the
// forward calls' table of host arrays, on the host under AddressSanitizer and
// UBSan (tests/test_fwd_tables_host.py).  Every input array and the word buffer
// lie in heap blocks of exactly their size, so one word read or written past
// an end is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../libzmq_amd/csrc/curve_fwd_common.hpp"

using namespace zmqg;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
            ++failures;                                            \
        }                                                          \
    } while (0)

typedef std::vector<uint32_t> Vec;

// a heap block of exactly n words
struct Exact {
    uint32_t *p;
    size_t n;
    explicit Exact(size_t words) : p((uint32_t *) malloc(4 * words + (words ? 0 : 1))), n(words) {}
    explicit Exact(const Vec &v) : p((uint32_t *) malloc(4 * v.size() + (v.size() ? 0 : 1))), n(v.size())
    {
        if (n)
            memcpy(p, v.data(), 4 * n);
    }
    ~Exact() { free(p); }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
};

static const uint32_t kFwdLbNoGroup = ZMQG_LB_NO_GROUP;
// the modes; the call is filled in by call_of
static const FwdTableIn kStatic = {nullptr, false, false, 1u, nullptr, 0};
static const FwdTableIn kSub = {nullptr, false, true, 1u, nullptr, 0};
static const FwdTableIn kPrepend = {nullptr, false, true, 2u, nullptr, 0}; // the router's PREPEND alone
static const FwdTableIn kRoute = {nullptr, true, true, 1u, nullptr, 0};    // ROUTE, with or without PREPEND

static zmqg_forward_zmtp call_of(uint64_t S, uint64_t MF, uint64_t n_dst, const uint32_t *carry_idx,
                                 const uint32_t *route_idx, const uint32_t *route_dst)
{
    zmqg_forward_zmtp a;
    memset(&a, 0, sizeof a);
    a.n_streams = S, a.max_frames = MF, a.n_dst = n_dst;
    a.carry_idx = carry_idx, a.route_idx = route_idx, a.route_dst = route_dst;
    return a;
}

// check_n's limit: the largest count it accepts
static uint64_t count_limit()
{
    uint64_t lim = 0;
    for (int bit = 62; bit >= 0; --bit)
        if (!check_n(lim | (1ull << bit)))
            lim |= 1ull << bit;
    return lim;
}

// The table of one call against the models' formulas: pair_base of
// tests/forward_model.py ((c + MF) * d), forward_router_model.py (m * (c + MF) *
// d', d' = 1 with ROUTE) and forward_lb_model.py (m * (c + MF)); ebase over the
// routed streams only; the group lists.  carry / routes are counts per stream;
// carry empty = no carry_idx.
static void run(uint64_t MF, const Vec &carry, const Vec &routes, uint64_t n_dst, FwdTableIn mode, const Vec &sgrp,
                uint64_t G)
{
    const uint64_t S = routes.size();
    Vec cidx(1, 0), ridx(1, 0), rdst;
    for (uint64_t s = 0; s < S; ++s) {
        cidx.push_back(cidx[s] + (carry.empty() ? 0u : carry[s]));
        ridx.push_back(ridx[s] + routes[s]);
        for (uint32_t k = 0; k < routes[s]; ++k)
            rdst.push_back((uint32_t) ((s * 7 + k * 3) % n_dst));
    }
    const Exact x_cidx(cidx), x_ridx(ridx), x_rdst(rdst), x_sgrp(sgrp);
    const bool lb = !sgrp.empty();
    mode.stream_group = lb ? x_sgrp.p : nullptr;
    mode.n_groups = G;
    // (with one route slot a stream the call's route arrays are not read: none is given)
    const zmqg_forward_zmtp a = call_of(S, MF, n_dst, carry.empty() ? nullptr : x_cidx.p,
                                        mode.one_route ? nullptr : x_ridx.p, mode.one_route ? nullptr : x_rdst.p);
    mode.a = &a;
    const FwdTableIn &in = mode;
    FwdTableDims t;
    CHECK(fwd_table_dims(in, t) == 0);
    std::vector<uint64_t> base(1, 0), ebase(1, 0);
    for (uint64_t s = 0; s < S; ++s) {
        const uint64_t c = carry.empty() ? 0u : carry[s], d = mode.one_route ? 1u : routes[s];
        base.push_back(base[s] + mode.m * (c + MF) * d);
        ebase.push_back(ebase[s] + (d ? c + MF : 0u));
    }
    uint64_t SG = 0;
    for (uint32_t g : sgrp)
        SG += g != kFwdLbNoGroup;
    const uint64_t R = mode.one_route ? 0u : rdst.size(), rows = mode.with_ebase ? 4 : 3;
    CHECK(t.N == base[S] && t.EN == ebase[S] && t.R == R && t.rows == rows && t.SG == SG);
    CHECK(t.words == rows * (S + 1) + R + (lb ? S + (G + 1) + SG : 0u));
    Exact w((size_t) t.words);
    memset(w.p, 0xa5, 4 * w.n);
    fwd_table_fill(in, t, w.p);
    const FwdTab h = fwd_tab(w.p, S, t);
    CHECK(h.rdst == w.p + rows * (S + 1));
    for (uint64_t s = 0; s <= S; ++s) {
        CHECK(h.base[s] == base[s]);
        CHECK(h.cidx[s] == (carry.empty() ? 0u : cidx[s]));
        CHECK(h.ridx[s] == (mode.one_route ? s : ridx[s]));
        if (mode.with_ebase)
            CHECK(h.ebase[s] == ebase[s]);
    }
    for (uint64_t i = 0; i < R; ++i)
        CHECK(h.rdst[i] == rdst[i]);
    if (!lb)
        return;
    struct {
        const uint32_t *sgrp, *gidx, *gstr; // where the load balancer's rows lie: behind the rows, no route_dst
    } l = {w.p + rows * (S + 1), w.p + rows * (S + 1) + S, w.p + rows * (S + 1) + S + (G + 1)};
    CHECK(l.gstr + SG == w.p + t.words);
    CHECK(l.gidx[0] == 0 && l.gidx[G] == SG);
    Vec seen(S, 0);
    for (uint64_t s = 0; s < S; ++s)
        CHECK(l.sgrp[s] == sgrp[s]);
    for (uint64_t g = 0; g < G; ++g) {
        CHECK(l.gidx[g] <= l.gidx[g + 1]);
        for (uint32_t i = l.gidx[g]; i < l.gidx[g + 1]; ++i) {
            const uint32_t s = l.gstr[i];
            CHECK(s < S && sgrp[s] == g);
            CHECK(i == l.gidx[g] || l.gstr[i - 1] < s); // rising within the group
            if (s < S)
                ++seen[s];
        }
    }
    for (uint64_t s = 0; s < S; ++s)
        CHECK(seen[s] == (sgrp[s] != kFwdLbNoGroup ? 1u : 0u)); // every grouped stream once
}

static void test_shapes()
{
    const Vec none;
    run(3, none, Vec{2}, 4, kStatic, none, 0); // S = 1
    run(0, Vec{2}, Vec{1}, 1, kStatic, none, 0);
    run(2, Vec{1, 0, 3}, Vec{2, 0, 1}, 5, kStatic, none, 0); // a stream without routes in the middle
    run(2, Vec{1, 0, 3}, Vec{2, 0, 1}, 5, kSub, none, 0);
    run(2, Vec{1, 4, 3}, Vec{0, 0, 0}, 5, kSub, none, 0); // no routes at all: N = EN = 0
    run(3, Vec{0, 2, 1}, Vec{1, 0, 3}, 4, kPrepend, none, 0); // m = 2
    run(3, Vec{0, 2, 1}, Vec{1, 0, 3}, 4, kRoute, none, 0);
    run(4, none, Vec{0, 0}, 2, kRoute, none, 0);
    FwdTableIn lb1 = kRoute, lb2 = kRoute;
    lb2.m = 2;
    run(2, Vec{1, 0, 2}, Vec{0, 0, 0}, 3, lb1, Vec{kFwdLbNoGroup, kFwdLbNoGroup, kFwdLbNoGroup}, 0); // G = 0
    // G = 3: group 1 without streams, stream 2 without a group, group 2's streams not adjacent
    run(2, Vec{1, 0, 2, 0, 1}, Vec{0, 0, 0, 0, 0}, 3, lb1, Vec{2, 0, kFwdLbNoGroup, 2, 0}, 3);
    run(1, none, Vec{0, 0, 0, 0, 0}, 3, lb2, Vec{2, 0, kFwdLbNoGroup, 2, 0}, 3);
    run(1, none, Vec{0}, 1, lb2, Vec{0}, 1);
    // S = 65
    Vec carry, routes, sgrp;
    for (uint32_t s = 0; s < 65; ++s) {
        carry.push_back(s % 4);
        routes.push_back(s % 5 == 2 ? 0 : s % 3 + 1);
        sgrp.push_back(s % 9 == 4 ? kFwdLbNoGroup : (s * 5) % 7);
    }
    run(3, carry, routes, 6, kStatic, none, 0);
    run(3, carry, routes, 6, kSub, none, 0);
    run(3, carry, routes, 6, kPrepend, none, 0);
    run(3, carry, routes, 6, kRoute, none, 0);
    run(3, carry, routes, 6, lb2, sgrp, 7);
}

// -EINVAL, and the sizes left as they were (the builder has no buffer to write yet)
static void reject(uint64_t S, uint64_t MF, const Vec &cidx, const Vec &ridx, const Vec &rdst, uint64_t n_dst,
                   FwdTableIn in, int line)
{
    const Exact x_cidx(cidx), x_ridx(ridx), x_rdst(rdst);
    const zmqg_forward_zmtp a =
        call_of(S, MF, n_dst, cidx.empty() ? nullptr : x_cidx.p, x_ridx.p, rdst.empty() ? nullptr : x_rdst.p);
    in.a = &a;
    FwdTableDims t, t0;
    memset(&t, 0x5a, sizeof t);
    memcpy(&t0, &t, sizeof t);
    if (fwd_table_dims(in, t) != -EINVAL || memcmp(&t, &t0, sizeof t)) {
        printf("FAIL %s:%d not rejected\n", __FILE__, line);
        ++failures;
    }
}

static void test_rejections()
{
    const Vec none;
    reject(3, 2, none, Vec{0, 2, 1, 3}, Vec{0, 0, 0}, 4, kStatic, __LINE__);          // a falling route_idx
    reject(3, 2, Vec{0, 2, 1, 3}, Vec{0, 1, 2, 3}, Vec{0, 0, 0}, 4, kStatic, __LINE__); // a falling carry_idx
    reject(3, 2, Vec{0, 2, 1, 3}, Vec{0, 1, 2, 3}, none, 4, kRoute, __LINE__);          // (with one route slot too)
    reject(2, 2, none, Vec{1, 2, 3}, Vec{0, 0, 0}, 4, kStatic, __LINE__);              // route_idx[0] != 0
    reject(2, 2, Vec{1, 2, 3}, Vec{0, 1, 2}, Vec{0, 0}, 4, kSub, __LINE__);            // carry_idx[0] != 0
    reject(2, 2, none, Vec{0, 1, 3}, Vec{0, 4, 1}, 4, kStatic, __LINE__);              // route_dst[i] >= n_dst
    reject(2, 2, none, Vec{0, 1, 3}, Vec{0, 1, 0xffffffffu}, 4, kPrepend, __LINE__);
    reject(1, 2, none, Vec{0, 2}, none, 4, kStatic, __LINE__);                         // routes and no route_dst
    const uint64_t lim = count_limit();
    CHECK(lim == 0x7fffffffull);
    // q * d just above 2^31 - 1 (route_dst is not reached)
    reject(1, 1u << 16, none, Vec{0, 1u << 15}, none, 4, kStatic, __LINE__);
    reject(1, 0x7fffffffu / 3u + 1u, none, Vec{0, 3}, none, 4, kSub, __LINE__);
    reject(1, 1u << 30, none, Vec{0, 1}, none, 4, kPrepend, __LINE__); // (m = 2 counts)
    // N crossing the limit through the sum: two streams of (lim + 1) / 2 pairs each
    const uint32_t q = 1u << 15, d = (uint32_t) ((lim + 1) / 2 / q);
    CHECK((uint64_t) q * d * 2 == lim + 1);
    reject(2, q, none, Vec{0, d, 2 * d}, none, 4, kStatic, __LINE__);
    reject(3, (lim + 1) / 2, none, Vec{0, 0, 0, 0}, none, 4, kRoute, __LINE__); // (one route slot a stream: 3 * MF)
    // ... and the limit itself is accepted: 2^15 * 2^15 + (2^15 - 1) * (2^15 + 1) = 2^31 - 1
    {
        const Vec cidx{0, 1, 1}, ridx{0, q, 2 * q + 1};
        const Exact x_cidx(cidx), x_ridx(ridx), x_rdst(Vec(2 * q + 1, 3));
        const zmqg_forward_zmtp a = call_of(2, q - 1, 4, x_cidx.p, x_ridx.p, x_rdst.p);
        FwdTableIn in = kStatic;
        in.a = &a;
        FwdTableDims t;
        CHECK(fwd_table_dims(in, t) == 0 && t.N == lim && t.words == 3 * 3 + 2 * q + 1);
        Exact w((size_t) t.words);
        fwd_table_fill(in, t, w.p);
        CHECK(w.p[1] == (1u << 30) && w.p[2] == lim);
        const zmqg_forward_zmtp a1 = call_of(1, lim, 4, nullptr, nullptr, nullptr);
        FwdTableIn one = kRoute;
        one.a = &a1;
        CHECK(fwd_table_dims(one, t) == 0 && t.N == lim && t.EN == lim);
    }
}

static void test_search()
{
    // streams without items share their successor's entry and are passed over
    const Exact tab(Vec{0, 0, 3, 3, 3, 7, 8});
    const uint32_t want[] = {1, 1, 1, 4, 4, 4, 4, 5};
    for (uint32_t i = 0; i < 8; ++i)
        CHECK(fwd_stream_of(tab.p, 6, i) == want[i]);
    const Exact one(Vec{0, 5});
    CHECK(fwd_stream_of(one.p, 1, 0u) == 0 && fwd_stream_of(one.p, 1, 4u) == 0);
}

int main()
{
    test_shapes();
    test_rejections();
    test_search();
    if (failures)
        return 1;
    printf("fwd_tables ok\n");
    return 0;
}
