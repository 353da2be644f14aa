// The one-round look-back's record (libzmq_amd/csrc/curve_lbrec.hpp) on the
// host: pack / valid / value over the epoch and value corners, a zero word
// never valid, a word of another call never valid within 2^31 calls.
// Built with -fsanitize=address,undefined by tests/test_lbrec_host.py.
#include <stdint.h>
#include <stdio.h>
#include <initializer_list>

#include "../../libzmq_amd/csrc/curve_lbrec.hpp"

using namespace zmqg;

static int fails = 0;
#define EXPECT(c)                                                  \
    do {                                                           \
        if (!(c)) {                                                \
            printf("line %d: %s\n", __LINE__, #c);                 \
            ++fails;                                               \
        }                                                          \
    } while (0)

int main()
{
    const uint32_t epochs[] = {1u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    const uint64_t values[] = {0ull, 0xffffffffull, 0x100000000ull, 0xffffffffffffffffull};
    for (uint32_t e : epochs) {
        EXPECT(!lbrec_valid(0ull, e)); // zero-filled memory
        for (uint64_t v : values) {
            const uint64_t lo = lbrec_pack(e, (uint32_t) v), hi = lbrec_pack(e, (uint32_t) (v >> 32));
            EXPECT(lo != 0 && hi != 0);
            EXPECT(lbrec_valid(lo, e) && lbrec_valid(hi, e));
            EXPECT(lbrec_value(lo, hi) == v);
            // the calls around it, the call 2^31 - 1 later and earlier, and
            // a few in between: their words are not this call's
            const uint32_t others[] = {e + 1u, e - 1u, e + 2u, e + 0x7fffffffu, e - 0x7fffffffu, e + 0x40000000u,
                                       e + 12345u};
            for (uint32_t o : others) {
                EXPECT(!lbrec_valid(lo, o) && !lbrec_valid(hi, o));
                EXPECT(!lbrec_valid(lbrec_pack(o, (uint32_t) v), e));
            }
            // a half-written record: one word of this call, one stale or zero
            EXPECT(lbrec_valid(lo, e) && !lbrec_valid(lbrec_pack(e - 1u, (uint32_t) (v >> 32)), e));
            EXPECT(!lbrec_valid(0ull, e));
        }
    }
    // consecutive epochs never share a tag, across the 32-bit wrap too
    for (uint32_t e : {0xfffffffeu, 0xffffffffu, 0u, 1u, 0x7ffffffeu, 0x7fffffffu, 0x80000000u})
        EXPECT(lbrec_tag(e) != lbrec_tag(e + 1u));
    if (fails)
        return printf("%d failures\n", fails), 1;
    printf("lbrec ok\n");
    return 0;
}
