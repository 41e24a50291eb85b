// pass2_swar.h — K2 pass 2 on plain 32-bit ops (flac_search16.hip
// packed_vsum): sum of v >> kv over a register of two kept int16 samples,
// three VALU per register, none of them packed 16-bit math.
//
// A half holds n (signed 16 bit); wanted is (n >> kv) ^ (n >> 15) = m ^
// (m >> 15) for m = n >> kv (arithmetic), which equals (|2m + 1| - 1) / 2.
// With s = kv - 1 (0..14):
//   * offset binary turns the arithmetic shift into a logical one:
//     (n + 2^15) >>> s = (n >> s) + 2^(15 - s), and n >> s = 2m + b;
//   * forcing bit 0 to 1 gives 2m + 1 + 2^(15 - s) (2^(15 - s) is even);
//   * |that - 2^(15 - s)| = |2m + 1|.
// On the 32-bit register: one logical shift of the whole word by s; then per
// bit of each half pass / invert / force 0 / force 1, chosen by two constant
// words (clear the s bits that came in from the upper half, invert bit
// 15 - s -- the 2^15 offset, applied after the shift --, set bit 0); then
// one v_sad_u16 against 2^(15 - s) in both halves, accumulating |2m + 1| of
// both.  A lane's sum of v >> kv is (acc - count) / 2.
//
// Host and device: the device form uses v_bitop3_b32 and v_sad_u16, the
// host form the same arithmetic in plain C++, so the identity is checked
// exhaustively on the CPU (tools/pass2_swar_check.cpp).
#ifndef ATG_PASS2_SWAR_H
#define ATG_PASS2_SWAR_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SWAR_HD __host__ __device__ inline
#else
#define SWAR_HD inline
#endif

// the per-job constants of one lane, for kv in [1, 15]
struct SwarK {
    uint32_t s;    // kv - 1: the shift
    uint32_t keep; // 1 bits: the result bit is forced (to val's bit)
    uint32_t val;  // forced value where keep is 1, inversion mask where it is 0
    uint32_t mid;  // 2^(15 - s) in both halves
};

SWAR_HD SwarK swar_consts(uint32_t kv)
{
    SwarK c;
    c.s = kv - 1u;
    c.mid = (0x8000u >> c.s) * 0x10001u;
    // bits 16 - s .. 15 of each half cleared, bit 0 set
    c.keep = (((0xFFFF0000u >> c.s) & 0xFFFFu) | 1u) * 0x10001u;
    // bit 15 - s inverted, bit 0 set
    c.val = c.mid | 0x10001u;
    return c;
}

// (x & ~keep) ^ val per bit: pass (0, 0), invert (0, 1), force 0 (1, 0),
// force 1 (1, 1)
SWAR_HD uint32_t swar_bits(uint32_t x, uint32_t keep, uint32_t val)
{
#if defined(__HIP_DEVICE_COMPILE__)
    // truth table over (x, keep, val), bit 4x + 2keep + val: 0x9A
    return __builtin_amdgcn_bitop3_b32(x, keep, val, 0x9A);
#else
    return (x & ~keep) ^ val;
#endif
}

// acc + |a.lo - b.lo| + |a.hi - b.hi| on unsigned halves
SWAR_HD uint32_t swar_sad16(uint32_t a, uint32_t b, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u16(a, b, acc);
#else
    const int32_t l = (int32_t)(a & 0xFFFFu) - (int32_t)(b & 0xFFFFu);
    const int32_t h = (int32_t)(a >> 16) - (int32_t)(b >> 16);
    return acc + (uint32_t)(l < 0 ? -l : l) + (uint32_t)(h < 0 ? -h : h);
#endif
}

// one register of two kept samples: acc + |2 m_lo + 1| + |2 m_hi + 1|
SWAR_HD uint32_t swar_step(uint32_t word, const SwarK &c, uint32_t acc)
{
    return swar_sad16(swar_bits(word >> c.s, c.keep, c.val), c.mid, acc);
}

#endif
