// pcm_rows.h — the PCM side of a row kernel, shared by pcm_chain.hip,
// pcm_tensor.hip and pcm_compare.hip: an atg_pcm_view (int16 or int32 at any
// sample offset, behind a pointer that need not be 16-byte aligned) is read
// in aligned 16-byte units, one workgroup per tile of a ragged row table, and
// interleaved samples go out in 16-byte stores.  The host part compiles
// without HIP; tools/pcm_rows_check.cpp runs it under the host sanitizers.
// Out of this on purpose: pcm_compare.hip's Chunk, whose register-indexed
// phases are its own access pattern, and each file's size limits.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/atgpu.h"

#if defined(__HIPCC__)
#define PR_HD __host__ __device__ __forceinline__
typedef unsigned int Unit __attribute__((ext_vector_type(4))); // 16 bytes
typedef const __attribute__((address_space(1))) Unit *Units;   // in global memory

// Units [u0, u0 + nu) of p, nu <= kDeep * kBlock + 1, each handed to
// use(unit, j) by the lane that loaded it.  A lane has all its loads in flight
// before its first use; the one unit an odd phase adds goes through lane 0.
template <int kDeep, uint32_t kBlock, class Use>
__device__ __forceinline__ void pcm_load_units(const void *p, uint64_t u0, uint32_t nu, Use use)
{
    Unit v[kDeep];
#pragma unroll
    for (int d = 0; d < kDeep; ++d) {
        const uint32_t j = threadIdx.x + d * kBlock;
        v[d] = j < nu ? ((Units)p)[u0 + j] : Unit{0, 0, 0, 0};
    }
#pragma unroll
    for (int d = 0; d < kDeep; ++d) {
        const uint32_t j = threadIdx.x + d * kBlock;
        if (j < nu)
            use(v[d], j);
    }
    if (threadIdx.x == 0 && nu > kDeep * kBlock)
        use(((Units)p)[u0 + kDeep * kBlock], kDeep * kBlock);
}

// A lane's 8 (int16) or 4 (int32) samples x[], samples q .. of a tile of
// n_out that starts at sample o0 of `out`, o0 + q on a 16-byte boundary: one
// non-temporal store, so a wave writes 1 KiB without a gap; the row's last
// group, when short, sample by sample, so nothing past the row is written.
template <int FOUT>
__device__ __forceinline__ void pcm_store_group(const int32_t *x, void *out, uint64_t o0,
                                                uint32_t q, uint32_t n_out)
{
    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef typename std::conditional<FOUT == ATG_PCM_S16, int16_t, int32_t>::type T;
    constexpr uint32_t G = 16 / sizeof(T);
    T *dst = (T *)out + o0 + q;
    if (q + G <= n_out) {
        v4i w = {x[0], x[1], x[2], x[3]};
        if constexpr (FOUT == ATG_PCM_S16) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = (x[2 * k] & 0xFFFF) | (int)((uint32_t)x[2 * k + 1] << 16);
        }
        __builtin_nontemporal_store(w, (v4i *)dst);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < G; ++j)
            if (q + j < n_out)
                dst[j] = (T)x[j];
    }
}
#else
#define PR_HD inline
#endif

// The aligned units [u0, u0 + nu) that hold frames [fa, fa + nf), nf > 0, of
// a row of ch channels whose first sample is sample lo from the aligned
// pointer; the first of those samples is sample `skew` of unit u0.  `per` is
// the samples of a unit: 8 for int16, 4 for int32.
struct PcmUnits {
    uint64_t u0;
    uint32_t nu, skew;
};
PR_HD PcmUnits pcm_units(uint64_t lo, uint64_t fa, uint32_t nf, uint32_t ch, uint32_t per)
{
    const uint64_t a = lo + fa * ch, b = a + (uint64_t)nf * ch; // b > a
    const uint64_t u0 = a / per;
    return {u0, (uint32_t)((b - 1) / per + 1 - u0), (uint32_t)(a - u0 * per)};
}

inline bool pcm_known_format(uint32_t f) { return f == ATG_PCM_S16 || f == ATG_PCM_S32; }
inline uint32_t pcm_sample_size(uint32_t f) { return f == ATG_PCM_S32 ? 4 : 2; }
inline bool pcm_misaligned(const atg_pcm_view &v)
{
    return (uintptr_t)v.d_pcm & (pcm_sample_size(v.format) - 1);
}

// A view as a kernel addresses it: p is d_pcm rounded down to 16 bytes, lo
// the index from p of the source's first sample.
struct PcmSplit {
    const void *p;
    uint64_t lo;
};
inline PcmSplit pcm_split(const atg_pcm_view &v)
{
    const uintptr_t addr = (uintptr_t)v.d_pcm;
    return {(const void *)(addr & ~(uintptr_t)15),
            (addr & 15u) / pcm_sample_size(v.format) + v.sample_offset};
}

inline std::string at_row(uint32_t i, const char *what)
{
    return "row " + std::to_string(i) + ": " + what;
}

// The refusals of row i's source where a view takes no window; Slot is
// host_common.h's ErrSlot.
template <class Slot> atg_status pcm_check_view(Slot &err, uint32_t i, const atg_pcm_view &v)
{
    const char *bad = !pcm_known_format(v.format) ? "unknown source format"
                      : v.window_offset != 0      ? "window_offset must be 0"
                      : v.src_frames && !v.d_pcm  ? "d_pcm is NULL with src_frames > 0"
                      : pcm_misaligned(v)         ? "d_pcm is not aligned to its sample size"
                                                  : nullptr;
    return bad ? err.fail(ATG_ERR_INVALID, at_row(i, bad)) : ATG_OK;
}

// Do two of the non-empty [start, end) ranges share an element?  Sorts them.
inline bool pcm_ranges_overlap(std::vector<std::pair<uint64_t, uint64_t>> &ranges)
{
    std::sort(ranges.begin(), ranges.end());
    for (size_t k = 1; k < ranges.size(); ++k)
        if (ranges[k].first < ranges[k - 1].second)
            return true;
    return false;
}

// A call's device table: the rows that have work, each with the number of
// its first tile (Row::tile0) in the call's one list of tiles.
template <class Row> struct PcmRowTable {
    std::vector<Row> rows;
    uint64_t tiles = 0;
    void add(Row r, uint64_t n_tiles)
    {
        r.tile0 = tiles;
        tiles += n_tiles;
        rows.push_back(r);
    }
    template <class Slot> atg_status check(Slot &err) const // does a grid hold the tiles?
    {
        if (tiles > 0x7FFFFFFFull)
            return err.fail(ATG_ERR_UNSUPPORTED, "more than 2^31 - 1 tiles in one call");
        return ATG_OK;
    }
};
