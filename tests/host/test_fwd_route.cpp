// fwd_id_view / fwd_id_less / fwd_id_equal / fwd_route_lookup
// (libzmq_amd/csrc/curve_fwd_route.hpp) on the host under AddressSanitizer and
// UBSan (tests/test_fwd_route_host.py).  The address, its staged window and
// id_bytes each lie in a heap block of exactly their size, so one byte read
// past either end is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../libzmq_amd/csrc/curve_fwd_route.hpp"

using namespace zmqg;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
            ++failures;                                            \
        }                                                          \
    } while (0)

// a heap block of exactly n bytes (n == 0: one that must not be read at all)
struct Exact {
    uint8_t *p;
    size_t n;
    explicit Exact(const std::string &s) : p((uint8_t *) malloc(s.size() ? s.size() : 1)), n(s.size())
    {
        if (n)
            memcpy(p, s.data(), n);
        else { // no byte of it is owned
            free(p);
            p = (uint8_t *) malloc(1) + 1;
        }
    }
    ~Exact() { free(n ? p : p - 1); }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
};

// a table as the call takes it; the arrays may say anything
struct Table {
    std::vector<uint64_t> off;
    std::vector<uint32_t> len, dst;
    std::string bytes;
    void add(const std::string &id, uint32_t d)
    {
        off.push_back(bytes.size()), len.push_back((uint32_t) id.size()), dst.push_back(d);
        bytes += id;
    }
};

// the lookup of `addr`, the window holding its first `win` bytes
static uint32_t look(const Table &t, const std::string &addr, uint32_t win, uint64_t n_dst = 1u << 20)
{
    Exact a(addr), w(addr.substr(0, win)), ib(t.bytes);
    FwdAddr fa;
    fa.win = w.p, fa.win_len = (uint32_t) w.n, fa.p = a.p, fa.len = (uint32_t) addr.size();
    return fwd_route_lookup(fa, t.off.size(), t.off.data(), t.len.data(), t.dst.data(), t.bytes.empty() ? nullptr : ib.p,
                            t.bytes.size(), n_dst, FwdSerialDiff());
}

static bool less_of(const std::string &id, const std::string &addr, uint32_t win)
{
    Exact a(addr), w(addr.substr(0, win)), ib(id);
    const uint64_t off = 0;
    const uint32_t len = (uint32_t) id.size();
    FwdAddr fa;
    fa.win = w.p, fa.win_len = (uint32_t) w.n, fa.p = a.p, fa.len = (uint32_t) addr.size();
    const FwdId e = fwd_id_view(0, &off, &len, ib.p, id.size());
    CHECK(!e.is_void);
    CHECK(fwd_id_equal(e, fa, FwdSerialDiff()) == (id == addr));
    return fwd_id_less(e, fa, FwdSerialDiff());
}

static uint32_t rnd_state = 12345;
static uint32_t rnd()
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

static std::string rnd_id(size_t max_len, uint32_t alphabet)
{
    std::string s(rnd() % (max_len + 1), '\0');
    for (char &c : s)
        c = (char) (rnd() % alphabet + (alphabet < 200 ? 0xf0 - alphabet : 0)); // (bytes above 0x7f: unsigned order)
    return s;
}

int main()
{
    const uint32_t wins[] = {0, 1, 4, 64, 256};
    // the ordering edge cases, every one against std::string's operator< (memcmp, then the length: blob_t's)
    {
        std::string long_a(300, '\x81'), long_b = long_a;
        long_b[299] = '\x82';
        const std::pair<std::string, std::string> cases[] = {
            {"abc", "abcd"},   {"abcd", "abc"},         {"abc", "abc"},          {"", ""},          {"", "a"},
            {"a", ""},         {"abc", "abd"},          {"abd", "abc"},          {"xbc", "abc"},    {"abc", "xbc"},
            {"\x7f", "\x80"},  {"\x80", "\x7f"},        {std::string("\0", 1), ""}, {"", std::string("\0", 1)},
            {long_a, long_b},  {long_b, long_a},        {long_a, long_a},        {long_a.substr(0, 299), long_a}};
        for (const auto &c : cases)
            for (uint32_t win : wins) {
                const std::string &a = c.first, &b = c.second;
                const bool want = a.size() < b.size() ? memcmp(a.data(), b.data(), a.size()) <= 0
                                                      : memcmp(a.data(), b.data(), b.size()) < 0;
                CHECK(less_of(a, b, win) == want);
                CHECK(want == (a < b)); // (char_traits<char> compares as unsigned char)
            }
    }
    // void entries: offset past the end, length past the end, off + len overflowing 64 bits
    {
        Exact ib(std::string("abc"));
        const uint64_t off[] = {0, 3, 4, 1, UINT64_MAX, UINT64_MAX - 1, 2};
        const uint32_t len[] = {3, 0, 0, 3, 2, 0xffffffffu, 1};
        const bool is_void[] = {false, false, true, true, true, true, false};
        for (int j = 0; j < 7; ++j) {
            const FwdId e = fwd_id_view((uint64_t) j, off, len, ib.p, 3);
            CHECK(e.is_void == is_void[j]);
            if (e.is_void)
                CHECK(e.len == 0 && e.p == nullptr);
        }
        // a void entry orders as the empty id and equals no address, the empty one included
        Exact a(std::string("")), b(std::string("a"));
        FwdAddr ea, eb;
        ea.win = ea.p = a.p, ea.win_len = ea.len = 0;
        eb.win = nullptr, eb.win_len = 0, eb.p = b.p, eb.len = 1;
        const FwdId v = fwd_id_view(2, off, len, ib.p, 3), empty = fwd_id_view(1, off, len, ib.p, 3);
        CHECK(!fwd_id_less(v, ea, FwdSerialDiff()) && fwd_id_less(v, eb, FwdSerialDiff()));
        CHECK(!fwd_id_equal(v, ea, FwdSerialDiff()) && fwd_id_equal(empty, ea, FwdSerialDiff()));
        // a null id_bytes with nothing in it
        const uint64_t o0 = 0;
        const uint32_t l0 = 0, l1 = 1;
        CHECK(!fwd_id_view(0, &o0, &l0, nullptr, 0).is_void && fwd_id_view(0, &o0, &l1, nullptr, 0).is_void);
    }
    // n_ids 0 and 1; a destination at or above n_dst; a table of void entries alone
    {
        Table t0, t1, tv;
        CHECK(look(t0, "abc", 4) == kFwdRouteUnknown && look(t0, "", 0) == kFwdRouteUnknown);
        t1.add("abc", 7);
        for (uint32_t win : wins) {
            CHECK(look(t1, "abc", win) == 7 && look(t1, "ab", win) == kFwdRouteUnknown);
            CHECK(look(t1, "abcd", win) == kFwdRouteUnknown && look(t1, "", win) == kFwdRouteUnknown);
            CHECK(look(t1, "abc", win, 8) == 7 && look(t1, "abc", win, 7) == kFwdRouteUnknown);
        }
        tv.add("abc", 1), tv.add("abd", 2);
        tv.off[0] = 7, tv.len[1] = 9; // both void now
        CHECK(look(tv, "abc", 4) == kFwdRouteUnknown && look(tv, "", 0) == kFwdRouteUnknown);
        // the empty id in the table
        Table te;
        te.add("", 3), te.add("a", 4);
        CHECK(look(te, "", 0) == 3 && look(te, "a", 1) == 4 && look(te, "b", 1) == kFwdRouteUnknown);
    }
    // a random sweep against std::map::find on sorted tables of distinct ids
    const size_t sizes[] = {0, 1, 2, 3, 63, 64, 65, 1000};
    for (size_t n : sizes)
        for (uint32_t alphabet : {2u, 3u, 256u}) {
            std::map<std::string, uint32_t> ref;
            for (int tries = 0; ref.size() < n && tries < 100000; ++tries)
                ref.insert(std::make_pair(rnd_id(alphabet == 256 ? 6 : 12, alphabet), (uint32_t) ref.size()));
            Table t;
            for (const auto &kv : ref) // (std::string orders as blob_t does: unsigned bytes, then the length)
                t.add(kv.first, kv.second);
            std::vector<std::string> probes;
            for (const auto &kv : ref) {
                probes.push_back(kv.first);
                probes.push_back(kv.first + std::string(1, '\xf0'));
                if (!kv.first.empty())
                    probes.push_back(kv.first.substr(0, kv.first.size() - 1));
                if (probes.size() > 600)
                    break;
            }
            for (int i = 0; i < 200; ++i)
                probes.push_back(rnd_id(alphabet == 256 ? 6 : 12, alphabet));
            for (const std::string &a : probes) {
                const auto it = ref.find(a);
                const uint32_t want = it == ref.end() ? kFwdRouteUnknown : it->second;
                CHECK(look(t, a, (uint32_t) (rnd() % 5)) == want);
            }
        }
    if (failures)
        return 1;
    printf("fwd_route ok\n");
    return 0;
}
