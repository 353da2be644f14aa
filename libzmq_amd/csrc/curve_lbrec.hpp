// The one-round look-back's record (k_frames_seq decode, ordered grids of at
// most kFramesBS workgroups): a workgroup's header-only nonce maximum as two
// 64-bit words, each carrying its own proof of belonging to this call --
//   bit 63      valid (a zero-filled word never validates)
//   bits 62..32 the call epoch modulo 2^31 (a word of another call does not
//               validate until 2^31 calls later)
//   bits 31..0  one half of the value (nonces use all 64 bits)
// -- so the two words are written by two relaxed stores with no wait between
// them and read in any order: no flag, no ordering between value and flag.
// Host-compilable (tests/host/test_lbrec.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZMQG_LBREC_FN __host__ __device__ inline
#else
#define ZMQG_LBREC_FN inline
#endif

namespace zmqg {

ZMQG_LBREC_FN uint32_t lbrec_tag(uint32_t epoch)
{
    return 0x80000000u | (epoch & 0x7fffffffu);
}
// one word: half = the value's low (word 0) or high (word 1) 32 bits
ZMQG_LBREC_FN uint64_t lbrec_pack(uint32_t epoch, uint32_t half)
{
    return ((uint64_t) lbrec_tag(epoch) << 32) | half;
}
ZMQG_LBREC_FN bool lbrec_valid(uint64_t word, uint32_t epoch)
{
    return (uint32_t) (word >> 32) == lbrec_tag(epoch);
}
// the value of two valid words
ZMQG_LBREC_FN uint64_t lbrec_value(uint64_t word_lo, uint64_t word_hi)
{
    return (word_hi << 32) | (word_lo & 0xffffffffull);
}

} // namespace zmqg
