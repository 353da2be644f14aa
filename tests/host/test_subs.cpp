// subs_classify / subs_slot_equal / subs_clamp (libzmq_amd/csrc/curve_subs.hpp)
// on the host under AddressSanitizer and UBSan (tests/test_subs_host.py).  Every
// payload, topic and slot lies in a heap block of exactly its size, so one byte
// read past its end is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../libzmq_amd/csrc/curve_subs.hpp"

using zmqg::subs_classify;
using zmqg::subs_clamp;
using zmqg::subs_slot_equal;

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

enum { MORE = 1, COMMAND = 2, SUBSCRIBE = 12, CANCEL = 16 };

// the verdict on payload p with msg_t flags fl: kind * 100 + skip
static uint32_t cls(const std::string &p, uint32_t fl)
{
    Exact e(p);
    uint32_t skip = 77;
    const uint32_t kind = subs_classify(e.p, (uint32_t) p.size(), fl, skip);
    return kind * 100u + skip;
}

static bool eq(const std::string &a, const std::string &b)
{
    Exact x(a), y(b);
    return subs_slot_equal(x.p, (uint32_t) a.size(), y.p, (uint32_t) b.size());
}

static std::string S(const char *s, size_t n) { return std::string(s, n); }

int main()
{
    const uint32_t none = 0, sub10 = SUBSCRIBE * 100 + 10, can7 = CANCEL * 100 + 7, sub1 = SUBSCRIBE * 100 + 1,
                   can1 = CANCEL * 100 + 1;
    // commands: by name, with the lengths around both names (0, 1, 6, 7, 9, 10)
    CHECK(cls("", COMMAND) == none);
    CHECK(cls(S("\x09", 1), COMMAND) == none);
    CHECK(cls(S("\x06", 1), COMMAND) == none);
    CHECK(cls(S("\x06" "CANCE", 6), COMMAND) == none);
    CHECK(cls(S("\x06" "CANCEL", 7), COMMAND) == can7); // the empty topic
    CHECK(cls(S("\x06" "CANCELab", 9), COMMAND) == can7);
    CHECK(cls(S("\x06" "CANCEX", 7), COMMAND) == none);
    CHECK(cls(S("\x09" "SUBSCRI", 8), COMMAND) == none);
    CHECK(cls(S("\x09" "SUBSCRIB", 9), COMMAND) == none);
    CHECK(cls(S("\x09" "SUBSCRIBE", 10), COMMAND) == sub10); // the empty topic
    CHECK(cls(S("\x09" "SUBSCRIBEtopic", 15), COMMAND) == sub10);
    CHECK(cls(S("\x09" "SUBSCRIBX", 10), COMMAND) == none);
    CHECK(cls(S("\x08" "SUBSCRIBE", 10), COMMAND) == none);
    CHECK(cls(S("\x09" "SUBSCRIBE", 10), COMMAND | MORE) == sub10);
    // other commands; a name length byte past the end
    CHECK(cls(S("\x04" "PING", 5), COMMAND) == none);
    CHECK(cls(S("\x04" "PONGxxxxxxxx", 13), COMMAND) == none);
    CHECK(cls(S("\x40" "AB", 3), COMMAND) == none);
    CHECK(cls(S("\xff", 1), COMMAND) == none);
    // a command whose first byte is 0 / 1 / 2 is no old-style subscription
    CHECK(cls(S("\x00", 1), COMMAND) == none);
    CHECK(cls(S("\x01", 1), COMMAND) == none);
    CHECK(cls(S("\x02", 1), COMMAND) == none);
    CHECK(cls(S("\x01" "abcdefghijk", 12), COMMAND) == none);
    // messages: by the first byte
    CHECK(cls("", 0) == none);
    CHECK(cls(S("\x00", 1), 0) == can1);
    CHECK(cls(S("\x01", 1), 0) == sub1);
    CHECK(cls(S("\x02", 1), 0) == none);
    CHECK(cls(S("\x01" "topic", 6), 0) == sub1);
    CHECK(cls(S("\x00" "topic", 6), MORE) == can1);
    CHECK(cls(S("\x02" "topic", 6), 0) == none);
    CHECK(cls(S("\x09" "SUBSCRIBEtopic", 15), 0) == none); // the name without the COMMAND flag: a user message
    CHECK(cls(S("\x06" "CANCEL", 7), 0) == none);

    // equality: lengths 0 .. 41 (the eight-byte steps and the tail), a difference in every position, in length only
    for (size_t n = 0; n <= 41; ++n) {
        std::string a(n, '\0');
        for (size_t i = 0; i < n; ++i)
            a[i] = (char) (i * 7 + 1);
        CHECK(eq(a, a));
        CHECK(!eq(a, a + "x"));
        CHECK(!eq(a + std::string(1, '\0'), a));
        if (n)
            CHECK(!eq(a, a.substr(0, n - 1)));
        for (size_t i = 0; i < n; ++i) {
            std::string b = a;
            b[i] = (char) (b[i] ^ 0x80);
            CHECK(!eq(a, b));
        }
    }
    // different lengths: neither side is read (a block that owns no byte)
    CHECK(!eq("", "a"));
    CHECK(eq("", ""));

    CHECK(subs_clamp(5, 8) == 5 && subs_clamp(8, 8) == 8 && subs_clamp(15, 8) == 8);
    CHECK(subs_clamp(0xffffffffu, 65536) == 65536 && subs_clamp(0xffffffffu, 0x7fffffffull) == 0x7fffffffu);

    if (failures)
        return 1;
    printf("subs ok\n");
    return 0;
}
