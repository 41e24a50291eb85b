// tta_common.h — arithmetic shared by the True Audio encoder and decoder
// (tta_encode.hip, tta_decode.hip): the adaptive Rice state, the hybrid
// filter's history, and CRC-32 in a form a workgroup can compute in parallel.
//
// Everything is integer.  Where the reference computes in `int` and lets the
// value wrap (the eight tap products and their sum, encoders/tta.c:352-359,
// decoders/tta.c:589-596), the arithmetic here is explicit uint32_t, so the
// wrap is defined and identical.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tta {

// one TTA frame of a batch (encoder: n PCM frames at pcm_start; decoder: the
// payload at data + byte_off, payload_bytes long, followed by its CRC-32)
struct Frame {
    uint64_t pcm_start;   // first PCM frame (encoder input / decoder output)
    uint64_t sbase;       // first sample of the frame's channel-major scratch
    uint64_t byte_off;    // first payload byte in the output / input buffer
    uint64_t chain0;      // index of the frame's channel-0 chain
    uint32_t n;           // PCM frames
    uint32_t reserved;
    uint32_t payload;     // decoder: payload bytes (frame size - 4)
    uint16_t channels;
    uint8_t hshift;       // hybrid filter shift: 9 at 16 bits, else 10
    uint8_t pshift;       // fixed prediction shift: 4 at 8 bits, else 5
};

// ---- Rice parameter adaption (encoders/tta.c:227-244, decoders/tta.c:482-496)
struct Rice {
    uint32_t k0 = 10, k1 = 10, sum0 = 1u << 14, sum1 = 1u << 14;
};

__host__ __device__ __forceinline__ void rice_adapt(uint32_t &k, uint32_t &sum, uint32_t v)
{
    sum += v - (uint32_t)((int32_t)sum >> 4);
    if (k > 0 && (int32_t)sum < (int32_t)(1u << ((k + 4) & 31)))
        k -= 1;
    else if ((int32_t)sum > (int32_t)(1u << ((k + 5) & 31)))
        k += 1;
}

// ---- the hybrid filter's state: taps qm, sign steps dx, history dl
struct Hybrid {
    int32_t qm[8], dx[8], dl[8];
    __host__ __device__ __forceinline__ void reset()
    {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            qm[j] = dx[j] = dl[j] = 0;
    }
    // taps follow the sign of the previous residual
    __host__ __device__ __forceinline__ void adapt(int32_t prev_residual)
    {
        const int32_t sg = (prev_residual > 0) - (prev_residual < 0);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            qm[j] = (int32_t)((uint32_t)qm[j] + (uint32_t)(sg * dx[j]));
    }
    // (round + sum dl qm) >> shift, the products and the sum wrapping at 32 bits
    __host__ __device__ __forceinline__ int32_t predict(uint32_t shift) const
    {
        uint32_t sum = 1u << (shift - 1);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            sum += (uint32_t)dl[j] * (uint32_t)qm[j];
        return (int32_t)sum >> shift;
    }
    // shift the history in the value the decoder will also know (p / f)
    __host__ __device__ __forceinline__ void push(int32_t v)
    {
        dx[0] = dx[1];
        dx[1] = dx[2];
        dx[2] = dx[3];
        dx[3] = dx[4];
        dx[4] = dl[4] >= 0 ? 1 : -1;
        dx[5] = dl[5] >= 0 ? 2 : -2;
        dx[6] = dl[6] >= 0 ? 2 : -2;
        dx[7] = dl[7] >= 0 ? 4 : -4;
        dl[0] = dl[1];
        dl[1] = dl[2];
        dl[2] = dl[3];
        dl[3] = dl[4];
        const uint32_t a = (uint32_t)v - (uint32_t)dl[7];   // p - dl7
        const uint32_t b = a - (uint32_t)dl[6];             // -dl6 + (p - dl7)
        dl[4] = (int32_t)(b - (uint32_t)dl[5]);
        dl[5] = (int32_t)b;
        dl[6] = (int32_t)a;
        dl[7] = v;
    }
};

// x - ((x 2^s - x) >> s) needs 64 bits for the product (encoders/tta.c:301-303)
__host__ __device__ __forceinline__ int32_t fixed_term(int32_t prev, uint32_t s)
{
    const int64_t v = (int64_t)((uint64_t)(int64_t)prev << s) - (int64_t)prev;
    return (int32_t)(v >> s);
}

// ---- CRC-32 (reflected 0xEDB88320, init and final xor 0xFFFFFFFF)
//
// A register holds a polynomial over GF(2), bit 31 the coefficient of x^0.
// Feeding n bytes to a register r leaves  r x^(8n) + crc0(bytes)  (mod P), so
// a message cut into pieces is the xor of every piece's crc0 advanced by the
// bytes after it, plus the initial register advanced by the whole length.
constexpr uint32_t kCrcPoly = 0xEDB88320u;

__host__ __device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m)
            p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

// x^(8 n) mod P
__host__ __device__ __forceinline__ uint32_t crc_xpow_bytes(uint64_t n)
{
    uint32_t r = 0x80000000u;  // x^0
    uint32_t sq = 0x00800000u; // x^8
    for (; n; n >>= 1) {
        if (n & 1u)
            r = crc_mul(r, sq);
        sq = crc_mul(sq, sq);
    }
    return r;
}

__host__ __device__ __forceinline__ uint32_t crc_byte_entry(uint32_t b)
{
    for (int k = 0; k < 8; ++k)
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    return b;
}

#ifdef __HIPCC__
constexpr int kCrcThreads = 256;

// CRC-32 of data[0, len) by one workgroup of kCrcThreads threads; every
// thread gets the result.  tab[256] and red[kCrcThreads] are LDS.
__device__ inline uint32_t crc32_block(const uint8_t *__restrict__ data, uint64_t len,
                                       uint32_t *tab, uint32_t *red)
{
    const uint32_t tid = threadIdx.x;
    tab[tid] = crc_byte_entry(tid);
    __syncthreads();
    const uint64_t per = (len + kCrcThreads - 1) / kCrcThreads;
    const uint64_t a = (uint64_t)tid * per < len ? (uint64_t)tid * per : len;
    const uint64_t b = a + per < len ? a + per : len;
    uint32_t r = 0;
    for (uint64_t i = a; i < b; ++i)
        r = tab[(r ^ data[i]) & 0xFFu] ^ (r >> 8);
    uint32_t term = (b > a) ? crc_mul(r, crc_xpow_bytes(len - b)) : 0u;
    if (tid == 0)
        term ^= crc_mul(0xFFFFFFFFu, crc_xpow_bytes(len));
    red[tid] = term;
    __syncthreads();
    for (uint32_t s = kCrcThreads / 2; s; s >>= 1) {
        if (tid < s)
            red[tid] ^= red[tid + s];
        __syncthreads();
    }
    const uint32_t out = red[0] ^ 0xFFFFFFFFu;
    __syncthreads();
    return out;
}
#endif

} // namespace tta
