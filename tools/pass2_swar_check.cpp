// pass2_swar_check.cpp — host check of K2's three-op pass-2 step
// (python-audio-tools_amd/csrc/pass2_swar.h) against the reference form
// sum of (n >> kv) ^ (n >> 15) over the two halves of a register.
//
// Quiet form: kv in [1, 14]; the half under test takes all 2^16 values, in
// the low and in the high position, the other half every 251st value.
// Loud form: the halves hold bits 8..23 of a 24-bit n and the step runs with
// kv - 8, kv in [9, 14]; the reference is (n >> kv) ^ (n >> 31) on n itself
// for a few low bytes.  Also the lane form: 32 registers accumulated, then
// (acc - 64) / 2, with warm-up slots n = -1.
// Build: g++ -O2 -std=c++17 -o pass2_swar_check tools/pass2_swar_check.cpp
#include <cstdint>
#include <cstdio>

#include "../python-audio-tools_amd/csrc/pass2_swar.h"

static uint32_t ref16(uint32_t half, uint32_t kv)
{
    const int32_t n = (int16_t)half;
    return (uint32_t)((n >> kv) ^ (n >> 15));
}

static uint32_t ref24(int32_t n, uint32_t kv) { return (uint32_t)((n >> kv) ^ (n >> 31)); }

int main()
{
    uint64_t cases = 0, bad = 0;
    for (uint32_t kv = 1; kv <= 14; ++kv) {
        const SwarK c = swar_consts(kv);
        for (uint32_t a = 0; a < 65536; ++a) {
            const uint32_t ra = ref16(a, kv);
            for (uint32_t b = 0; b < 65536; b += 251) {
                const uint32_t want = ra + ref16(b, kv);
                const uint32_t lo = (swar_step(a | (b << 16), c, 0u) - 2u) >> 1;
                const uint32_t hi = (swar_step(b | (a << 16), c, 0u) - 2u) >> 1;
                cases += 2;
                if (lo != want || hi != want) {
                    if (bad < 8)
                        printf("quiet kv %u a %04x b %04x: %u / %u want %u\n", kv, a, b, lo, hi, want);
                    ++bad;
                }
            }
        }
    }
    static const uint32_t kLowBytes[] = {0x00u, 0x5Au, 0xFFu};
    for (uint32_t kv = 9; kv <= 14; ++kv) {
        const SwarK c = swar_consts(kv - 8u);
        for (uint32_t a = 0; a < 65536; ++a) {
            for (uint32_t lb : kLowBytes) {
                // n: 24-bit signed with bits 8..23 = a
                const int32_t na = (int32_t)((uint32_t)(int32_t)(int16_t)a << 8 | lb);
                const uint32_t ra = ref24(na, kv);
                for (uint32_t b = 0; b < 65536; b += 251) {
                    const int32_t nb = (int32_t)((uint32_t)(int32_t)(int16_t)b << 8 | (lb ^ 0xA5u));
                    const uint32_t want = ra + ref24(nb, kv);
                    const uint32_t lo = (swar_step(a | (b << 16), c, 0u) - 2u) >> 1;
                    const uint32_t hi = (swar_step(b | (a << 16), c, 0u) - 2u) >> 1;
                    cases += 2;
                    if (lo != want || hi != want) {
                        if (bad < 16)
                            printf("loud kv %u a %04x b %04x: %u / %u want %u\n", kv, a, b, lo, hi, want);
                        ++bad;
                    }
                }
            }
        }
    }
    // the lane form: 64 samples in 32 registers, the first `warm` forced to -1
    uint32_t x = 12345u;
    for (uint32_t kv = 1; kv <= 15; ++kv) {
        const SwarK c = swar_consts(kv);
        for (int rep = 0; rep < 2000; ++rep) {
            const int warm = rep % 13;
            uint32_t acc = 0, want = 0;
            for (int t = 0; t < 32; ++t) {
                uint32_t h[2];
                for (int q = 0; q < 2; ++q) {
                    x = x * 1664525u + 1013904223u;
                    // full-scale and small values alternate between repetitions
                    h[q] = (rep & 1) ? (x >> 16) : (uint32_t)(int32_t)((int32_t)(x >> 24) - 128) & 0xFFFFu;
                    if (2 * t + q < warm)
                        h[q] = 0xFFFFu;
                    want += ref16(h[q], kv);
                }
                acc = swar_step(h[0] | (h[1] << 16), c, acc);
            }
            ++cases;
            if (((acc - 64u) >> 1) != want) {
                if (bad < 24)
                    printf("lane kv %u rep %d: %u want %u\n", kv, rep, (acc - 64u) >> 1, want);
                ++bad;
            }
        }
    }
    printf("cases %llu bad %llu\n", (unsigned long long)cases, (unsigned long long)bad);
    return bad ? 1 : 0;
}
