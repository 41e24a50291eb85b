// bits_lsb.h — the LSB-first bit reader of the TTA and WavPack decoders: one
// lane walks bytes [pos, end) of a buffer through a 64-bit accumulator.
// Bytes outside the range never reach the accumulator, so a neighbour's
// bytes never reach the decoder.  How a word is fetched is the template
// parameter's:
//
//   LsbReader<false>  an aligned word load, unconditionally.  For ranges every
//                     word of which lies inside the buffer (the buffer's
//                     length is a multiple of 4 and the range starts in it).
//   LsbReader<true>   an aligned word where the whole word lies below `limit`
//                     (the buffer's length), the range's bytes one at a time
//                     otherwise.
//
// Compiles for the host alone as well (tools/bits_crc_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LSB_HD __host__ __device__ __forceinline__
#else
#define LSB_HD inline
#endif

template <bool LIMITED> struct LsbReader {
    const uint8_t *data; // the buffer, 4-byte aligned
    uint64_t pos, end;   // next byte to load, end of the range (byte indices)
    uint64_t limit = 0;  // LIMITED: the buffer's length
    uint64_t acc = 0;    // loaded bits, next bit at bit 0
    uint32_t have = 0;   // valid bits in acc

    LSB_HD void refill()
    {
        while (have <= 32u && pos < end) {
            const uint64_t base = pos & ~3ull;        // pos's aligned word
            const uint32_t skip = (uint32_t)pos & 3u; // bytes below pos in the word
            const uint64_t left = end - pos;          // bytes still in range
            uint32_t nb = 4u - skip;                  // bytes this word offers
            if ((uint64_t)nb > left)
                nb = (uint32_t)left;
            uint32_t v;
            if (!LIMITED || base + 4u <= limit) {
                v = *(const uint32_t *)(data + base) >> (8u * skip);
            } else {
                v = 0;
                for (uint32_t k = 0; k < nb; ++k)
                    v |= (uint32_t)data[pos + k] << (8u * k);
            }
            if (nb < 4u)
                v &= (1u << (8u * nb)) - 1u;
            acc |= (uint64_t)v << have;
            have += 8u * nb;
            pos += nb;
        }
    }
    // a run of 1 bits ended by a 0 bit; false when the range ends first
    LSB_HD bool unary(uint32_t &count)
    {
        count = 0;
        for (;;) {
            refill();
            if (have == 0)
                return false;
            const uint64_t inv = ~acc;
            const uint32_t ones = inv ? (uint32_t)__builtin_ctzll(inv) : 64u;
            if (ones < have) {
                count += ones;
                acc = (acc >> ones) >> 1; // ones + 1 may be 64
                have -= ones + 1u;
                return true;
            }
            count += have;
            acc = 0;
            have = 0;
        }
    }
    LSB_HD bool bits(uint32_t n, uint32_t &v) // n <= 32
    {
        refill();
        if (have < n)
            return false;
        v = n ? (uint32_t)(acc & ((1ull << n) - 1ull)) : 0u;
        acc >>= n;
        have -= n;
        return true;
    }
};
