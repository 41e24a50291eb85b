// crc_common.h — what the MSB-first CRCs of the containers share (FLAC's
// CRC-8 0x07 and CRC-16 0x8005, Ogg's CRC-32 0x04C11DB7; init 0, no final
// xor): the host builders of the byte, slicing and "advance by 2^m zero
// bytes" tables, the device loop that applies one advance matrix, and the
// unaligned big-endian word load the slicing loops feed on.  Compiles for the
// host alone as well (tools/bits_crc_check.cpp).
//
// A CRC is linear over GF(2): appending zero bytes to a message multiplies
// the state by a fixed W x W bit matrix.  adv[m] holds that matrix for 2^m
// zero bytes as its W column images (adv[m][i] = the state 1 << i advanced),
// so crc(A || B) = advance(crc(A), |B|) ^ crc(B), with advance() one matrix
// per set bit of |B|.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CRC_HD __host__ __device__ __forceinline__
#define CRC_UNROLL _Pragma("unroll")
#else
#define CRC_HD inline
#define CRC_UNROLL
#endif

// state c through one advance matrix (its BITS column images at `col`)
template <int BITS, typename T>
CRC_HD uint32_t crc_advance(const T *col, uint32_t c)
{
    uint32_t r = 0;
    CRC_UNROLL
    for (int i = 0; i < BITS; ++i)
        r ^= ((c >> i) & 1u) ? (uint32_t)col[i] : 0u;
    return r;
}

#if defined(__HIPCC__)
// big-endian 32 bits at absolute byte b of the buffer: two aligned loads,
// word indices clamped to `last`
__device__ __forceinline__ uint32_t be32_at(const uint32_t *w, uint64_t last, uint64_t b)
{
    const uint64_t i = b >> 2;
    const uint32_t x = __builtin_bswap32(w[i < last ? i : last]);
    const uint32_t r = (uint32_t)(b & 3u);
    if (!r)
        return x;
    const uint32_t y = __builtin_bswap32(w[i + 1 < last ? i + 1 : last]);
    return (x << (8u * r)) | (y >> (32u - 8u * r));
}
#endif

// ---- host builders.  T is the element type the consumer stores (uint8_t,
// uint16_t or uint32_t; values are below 2^W whichever it is).

// t[k * 256 + b], k < K: the CRC (width W, polynomial `poly`) of byte b
// followed by k zero bytes -- the byte table (K = 1) or slicing-by-K tables
template <int W, typename T>
inline void crc_build_tables(uint32_t poly, T *t, int K)
{
    const uint32_t top = 1u << (W - 1), mask = (top - 1u) | top;
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t c = b << (W - 8);
        for (int i = 0; i < 8; ++i)
            c = (c & top) ? (c << 1) ^ poly : c << 1;
        t[b] = (T)(c & mask);
    }
    for (int k = 1; k < K; ++k)
        for (uint32_t b = 0; b < 256; ++b) {
            const uint32_t p = t[(k - 1) * 256 + b];
            t[k * 256 + b] = (T)(((p << 8) ^ t[p >> (W - 8)]) & mask);
        }
}

// out = the matrix a applied twice (W column images each)
template <int W, typename T>
inline void crc_square(const T *a, T *out)
{
    for (int i = 0; i < W; ++i)
        out[i] = (T)crc_advance<W>(a, a[i]);
}

// adv[m * W + i], m < M: the state 1 << i after 2^m zero bytes.  adv[0] is
// one zero byte through the byte table t0; adv[m] = adv[m - 1] applied twice.
template <int W, typename T0, typename T>
inline void crc_build_advance(const T0 *t0, T *adv, int M)
{
    const uint32_t top = 1u << (W - 1), mask = (top - 1u) | top;
    for (int i = 0; i < W; ++i) {
        const uint32_t c = 1u << i;
        adv[i] = (T)(((c << 8) ^ t0[c >> (W - 8)]) & mask);
    }
    for (int m = 1; m < M; ++m)
        crc_square<W>(adv + (m - 1) * W, adv + m * W);
}
