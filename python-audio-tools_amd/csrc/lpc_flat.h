// lpc_flat.h — where K1's autocorrelation may use a fused multiply-add.
//
// The Tukey(0.5) window of tukey() (engine.hip; reference
// flacenc_window_signal, flac.c:1139-1161) is assigned the literal 1.0 for
// window1 < n <= window2.  There the windowed sample x[n] = (double)s[n] * 1.0
// is the integer sample itself, and a product x[n-L] * x[n] of two such
// samples of at most 26 bits is an integer below 2^52: exact in fp64.  For an
// exact product fma(a, b, acc) = RN(a*b + acc) = RN(RN(a*b) + acc), the bits
// the reference's rounded multiply and rounded add give.
//
// Both operands of every product must be flat: sample n may use the FMA only
// when w[n - lags .. n] are all 1.0 (lags = the accumulators' largest lag).
// One tapered operand makes the product inexact and the fused form differ.
//
// The range comes from the literal assignment only.  The cosine branches may
// also round to 1.0 (N = 57: w[14] == 1.0 with 14 <= window1); such samples
// stay outside, so the range is never wider than the table's run of ones.
// tools/lpc_flat_check.cpp checks it against the table for every N.
//
// Shared by device and host code (plain C++, no HIP types).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LPC_FLAT_FN __host__ __device__ inline
#else
#define LPC_FLAT_FN inline
#endif

// widest candidate (side channel's extra bit included) whose products of two
// flat samples stay exact: 2 * 26 = 52 bits of magnitude
#define LPC_FLAT_MAX_BITS 26u

struct LpcFlatRange {
    uint32_t lo, hi; // samples n in [lo, hi) may use the FMA; lo >= hi: none
};

LPC_FLAT_FN LpcFlatRange lpc_flat_range(uint32_t N, uint32_t lags)
{
    LpcFlatRange r = {0u, 0u};
    if (N < 2u)
        return r;
    // tukey()'s own expressions
    const double alpha = 0.5;
    const unsigned window1 = (unsigned)(alpha * (N - 1)) / 2;
    const unsigned window2 = (unsigned)((N - 1) * (1.0 - (alpha / 2.0)));
    // w[n] is the literal 1.0 for n in [window1 + 1, window2]
    r.lo = window1 + 1u + lags;
    r.hi = window2 + 1u;
    if (r.hi > N)
        r.hi = N;
    if (r.lo >= r.hi)
        r.lo = r.hi = 0u;
    return r;
}

// a group of `count` samples starting at j0 lies wholly inside the range
LPC_FLAT_FN bool lpc_flat_group(const LpcFlatRange &r, uint32_t j0, uint32_t count)
{
    return j0 >= r.lo && j0 + count <= r.hi;
}
