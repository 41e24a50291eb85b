// shn_common.h — what the Shorten encoder and decoder share: the command
// numbers and field widths of the format, the MSB-first bit access both
// sides use on the device, and a host-side bit writer for the parts of a
// file the host writes (header, VERBATIM commands, trailer).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace shn {

enum : uint32_t {
    FN_DIFF0 = 0,
    FN_DIFF1 = 1,
    FN_DIFF2 = 2,
    FN_DIFF3 = 3,
    FN_QUIT = 4,
    FN_BLOCKSIZE = 5,
    FN_BITSHIFT = 6,
    FN_QLPC = 7,
    FN_ZERO = 8,
    FN_VERBATIM = 9
};
constexpr uint32_t kCommandSize = 2, kEnergySize = 3, kLpcCountSize = 2, kLpcCoeffSize = 5,
                   kVerbatimChunkSize = 5, kVerbatimByteSize = 8, kShiftSize = 2;

// bits of unsigned(c) holding v (c < 32): the zero run, the stop bit, c bits
__host__ __device__ inline uint32_t unsigned_bits(uint32_t c, uint32_t v)
{
    return (v >> c) + 1u + c;
}
// bits of long(v)
__host__ __device__ inline uint32_t long_bits(uint32_t v)
{
    if (!v)
        return 4u;
    uint32_t n = 0;
    for (uint32_t t = v; t; t >>= 1)
        ++n;
    return unsigned_bits(2, n) + 1u + n;
}

// ------------------------------------------------------------ device input
// The 32-bit big-endian word `wi` of an image of `nbytes` bytes that starts
// 4-byte aligned at `img`; bytes past the end read as zero and no byte past
// the end is touched.
__device__ __forceinline__ uint32_t be_word(const uint8_t *__restrict__ img, uint64_t nbytes,
                                            uint64_t wi)
{
    const uint64_t b = wi * 4u;
    if (b + 4u <= nbytes)
        return __builtin_bswap32(*reinterpret_cast<const uint32_t *>(img + b));
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4u; ++k)
        if (b + k < nbytes)
            v |= (uint32_t)img[b + k] << (24u - 8u * k);
    return v;
}

// the 32 bits that start at bit `pos` (zero past the end)
__device__ __forceinline__ uint32_t peek32(const uint8_t *__restrict__ img, uint64_t nbytes,
                                           uint64_t pos)
{
    const uint64_t wi = pos >> 5;
    const uint32_t sh = (uint32_t)pos & 31u;
    const uint32_t a = be_word(img, nbytes, wi);
    if (!sh)
        return a;
    return (a << sh) | (be_word(img, nbytes, wi + 1) >> (32u - sh));
}

// A reader over one image.  A read that needs a bit past the end sets `bad`
// (the reference's I/O error) and every later read returns zero.
struct Bits {
    const uint8_t *img;
    uint64_t nbytes, nbits, pos;
    bool bad;
    __device__ void open(const uint8_t *p, uint64_t n, uint64_t at)
    {
        img = p;
        nbytes = n;
        nbits = n * 8u;
        pos = at;
        bad = false;
    }
    __device__ uint32_t read(uint32_t count) // count <= 32
    {
        if (bad || !count)
            return 0;
        if (pos + count > nbits) {
            bad = true;
            return 0;
        }
        const uint32_t v = peek32(img, nbytes, pos) >> (32u - count);
        pos += count;
        return v;
    }
    __device__ uint32_t unary()
    {
        uint32_t run = 0;
        while (!bad) {
            if (pos >= nbits) {
                bad = true;
                break;
            }
            const uint32_t v = peek32(img, nbytes, pos);
            if (v) {
                const uint32_t lz = (uint32_t)__clz((int)v);
                run += lz;
                pos += lz + 1u;
                if (pos > nbits)
                    bad = true;
                return run;
            }
            run += 32u;
            pos += 32u;
        }
        return 0;
    }
    // read_unsigned(): run << c | low, wrapped to 32 bits; c <= 32
    __device__ uint32_t uns(uint32_t c)
    {
        const uint32_t msb = unary();
        const uint32_t lsb = read(c);
        return (c < 32u ? msb << c : 0u) | lsb;
    }
    __device__ int32_t sgn(uint32_t c)
    {
        const uint32_t u = uns(c + 1u);
        return (u & 1u) ? (int32_t)(0u - (u >> 1) - 1u) : (int32_t)(u >> 1);
    }
    // skip one unsigned(c) code
    __device__ void skip(uint32_t c)
    {
        (void)unary();
        if (bad)
            return;
        if (pos + c > nbits)
            bad = true;
        else
            pos += c;
    }
};

// The same codes through a 64-bit window, for a lane that walks many codes of
// a run the index pass has already bounded: one word load per 32 bits in
// place of two per field.  Words past the end read as zero, and a zero run
// that reaches the end stops there.
struct Window {
    const uint8_t *img;
    uint64_t nbytes, nbits, pos, next;
    uint64_t buf;  // the bits from pos on, the first in bit 63
    uint32_t have; // valid bits in buf
    __device__ void fill()
    {
        if (have <= 32u) {
            buf |= (uint64_t)be_word(img, nbytes, next++) << (32u - have);
            have += 32u;
        }
    }
    __device__ void drop(uint32_t n) // n <= 32 <= have
    {
        buf <<= n;
        have -= n;
        pos += n;
    }
    __device__ void open(const uint8_t *p, uint64_t n, uint64_t at)
    {
        img = p;
        nbytes = n;
        nbits = n * 8u;
        pos = at & ~31ull;
        next = at >> 5;
        buf = 0;
        have = 0;
        fill();
        drop((uint32_t)at & 31u);
    }
    __device__ uint32_t read(uint32_t count) // count <= 32
    {
        if (!count)
            return 0;
        fill();
        const uint32_t v = (uint32_t)(buf >> (64u - count));
        drop(count);
        return v;
    }
    __device__ uint32_t unary()
    {
        uint32_t run = 0;
        for (;;) {
            fill();
            const uint32_t top = (uint32_t)(buf >> 32);
            if (top) {
                const uint32_t lz = (uint32_t)__clz((int)top);
                drop(lz + 1u);
                return run + lz;
            }
            if (pos >= nbits)
                return run;
            run += 32u;
            drop(32u);
        }
    }
    __device__ uint32_t uns(uint32_t c)
    {
        const uint32_t msb = unary();
        const uint32_t lsb = read(c);
        return (c < 32u ? msb << c : 0u) | lsb;
    }
    __device__ int32_t sgn(uint32_t c)
    {
        const uint32_t u = uns(c + 1u);
        return (u & 1u) ? (int32_t)(0u - (u >> 1) - 1u) : (int32_t)(u >> 1);
    }
};

// ----------------------------------------------------------- device output
// OR the low nb (1..32) bits of v into a zeroed MSB-first stream at bit pos
__device__ __forceinline__ void put_bits(uint32_t *__restrict__ out, uint64_t pos, uint32_t v,
                                         uint32_t nb)
{
    const uint64_t w = pos >> 5;
    const uint32_t sh = (uint32_t)pos & 31u;
    if (sh + nb <= 32u) {
        const uint32_t x = v << (32u - sh - nb);
        if (x)
            atomicOr(out + w, __builtin_bswap32(x));
    } else {
        const uint32_t hi = v >> (sh + nb - 32u);
        const uint32_t lo = v << (64u - sh - nb);
        if (hi)
            atomicOr(out + w, __builtin_bswap32(hi));
        if (lo)
            atomicOr(out + w + 1, __builtin_bswap32(lo));
    }
}
// unsigned(c) holding v at pos (c <= 31); the zero run needs no write
__device__ __forceinline__ uint64_t put_unsigned(uint32_t *__restrict__ out, uint64_t pos,
                                                 uint32_t c, uint32_t v)
{
    pos += v >> c;
    put_bits(out, pos, (1u << c) | (v & ((1u << c) - 1u)), c + 1u);
    return pos + c + 1u;
}
__device__ __forceinline__ uint64_t put_long(uint32_t *__restrict__ out, uint64_t pos, uint32_t v)
{
    if (!v) {
        pos = put_unsigned(out, pos, 2, 0);
        return put_unsigned(out, pos, 0, 0);
    }
    const uint32_t n = 32u - (uint32_t)__clz((int)v);
    pos = put_unsigned(out, pos, 2, n);
    // n can be 32: the stop bit, then the value
    put_bits(out, pos, 1u, 1u);
    put_bits(out, pos + 1u, v, n);
    return pos + 1u + n;
}

// -------------------------------------------------------- host bit writer
struct HostBits {
    std::vector<uint8_t> bytes;
    uint64_t nbits = 0;
    void write(uint32_t count, uint32_t value)
    {
        for (uint32_t k = count; k-- > 0;) {
            if ((nbits & 7u) == 0)
                bytes.push_back(0);
            if ((value >> k) & 1u)
                bytes.back() |= (uint8_t)(0x80u >> (nbits & 7u));
            ++nbits;
        }
    }
    void zeros(uint64_t count)
    {
        for (; count; --count)
            write(1, 0);
    }
    void uns(uint32_t c, uint32_t v)
    {
        zeros(c < 32u ? v >> c : 0u);
        write(1, 1);
        write(c, v);
    }
    void lng(uint32_t v)
    {
        if (!v) {
            uns(2, 0);
            uns(0, 0);
            return;
        }
        uint32_t n = 0;
        for (uint32_t t = v; t; t >>= 1)
            ++n;
        uns(2, n);
        uns(n, v);
    }
    void verbatim(const uint8_t *p, uint32_t n)
    {
        uns(kCommandSize, FN_VERBATIM);
        uns(kVerbatimChunkSize, n);
        for (uint32_t i = 0; i < n; ++i)
            uns(kVerbatimByteSize, p[i]);
    }
};

} // namespace shn
