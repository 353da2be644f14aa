// fwd_prefix_match / fwd_sub_range (libzmq_amd/csrc/curve_fwd_match.hpp) on the
// host under AddressSanitizer and UBSan (tests/test_fwd_match_host.py).  The
// topic, its staged window and sub_bytes each lie in a heap block of exactly
// their size, at an odd offset of the allocation's granule where the size
// allows, so one byte read past either end is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../libzmq_amd/csrc/curve_fwd_match.hpp"

using zmqg::fwd_prefix_match;
using zmqg::fwd_sub_range;

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

// one prefix against one topic, the window holding the topic's first `win` bytes
static bool run(const std::string &topic, const std::string &prefix, uint32_t win, uint64_t lead = 1,
                uint64_t claim_past = 0)
{
    Exact t(topic), w(topic.substr(0, win));
    // sub_bytes: `lead` bytes in front so that the prefix sits at an odd offset, and nothing behind it
    Exact sb(std::string((size_t) lead, '\xAA') + prefix);
    return fwd_prefix_match(w.p, win, t.p, (uint32_t) topic.size(), lead, (uint32_t) prefix.size() + (uint32_t) claim_past,
                            sb.p, sb.n);
}

static std::string topic_of(size_t n)
{
    std::string t(n, '\0');
    for (size_t i = 0; i < n; ++i)
        t[i] = (char) ((7 * i + 1) & 0xff);
    return t;
}

int main()
{
    const size_t lens[] = {0, 1, 3, 4, 5, 63, 64, 65, 300};
    const uint32_t wins[] = {0, 1, 4, 64, 256};
    for (size_t n : lens)
        for (uint32_t win : wins)
            for (uint64_t lead : {1, 3, 7}) {
                const std::string t = topic_of(n);
                CHECK(run(t, "", win, lead));                  // the empty prefix
                CHECK(run(t, t, win, lead));                   // equal to the topic
                CHECK(!run(t, t + std::string(1, '\0'), win, lead)); // one byte longer
                if (n) {
                    std::string a = t, b = t;
                    a[n - 1] ^= (char) 0x80;
                    b[0] ^= 1;
                    CHECK(!run(t, a, win, lead));              // the last byte differs
                    CHECK(!run(t, b, win, lead));              // the first byte differs
                    CHECK(run(t, t.substr(0, n - 1), win, lead)); // one byte shorter
                    CHECK(run(t, t.substr(0, 1), win, lead));  // (two matching prefixes: each alone matches)
                }
                // sub_off + sub_len == sub_bytes_len + 1: never a match, and not read -- with a prefix
                // whose owned bytes all agree with the topic, so that only the bound can say no
                if (n)
                    CHECK(!run(t, t.substr(0, n - 1), win, lead, 1));
            }
    {
        // the offset alone past the extent, and an offset near 2^64 (no wrap-around in the check)
        Exact t(std::string("abc")), sb(std::string("abc"));
        CHECK(fwd_prefix_match(t.p, 3, t.p, 3, 0, 3, sb.p, 3));
        CHECK(fwd_prefix_match(t.p, 3, t.p, 3, 3, 0, sb.p, 3));  // the empty prefix at the very end
        CHECK(!fwd_prefix_match(t.p, 3, t.p, 3, 4, 0, sb.p, 3));
        CHECK(!fwd_prefix_match(t.p, 3, t.p, 3, 1, 3, sb.p, 3));
        CHECK(!fwd_prefix_match(t.p, 3, t.p, 3, UINT64_MAX, 2, sb.p, 3));
        CHECK(!fwd_prefix_match(t.p, 3, t.p, 3, UINT64_MAX - 1, 0xffffffffu, sb.p, 3));
        CHECK(!fwd_prefix_match(t.p, 3, t.p, 3, 0, 1, nullptr, 0));
        CHECK(fwd_prefix_match(t.p, 3, t.p, 3, 0, 0, nullptr, 0));
    }
    {
        uint32_t lo, hi;
        fwd_sub_range(2, 5, 9, lo, hi);
        CHECK(lo == 2 && hi == 5);
        fwd_sub_range(2, 50, 9, lo, hi); // above n_subs: clamped
        CHECK(lo == 2 && hi == 9);
        fwd_sub_range(0xffffffffu, 0xffffffffu, 9, lo, hi);
        CHECK(lo == 9 && hi == 9);
        fwd_sub_range(5, 2, 9, lo, hi); // falling: empty
        CHECK(lo == hi);
        fwd_sub_range(0, 3, 0, lo, hi);
        CHECK(lo == 0 && hi == 0);
    }
    if (failures)
        return 1;
    printf("fwd_match ok\n");
    return 0;
}
