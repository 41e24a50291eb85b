// pcm_bytes.h — the per-lane bodies and the run/tile index arithmetic of
// pcm_bytes.hip, as host + device inline functions: the kernels call them
// with (blockIdx, threadIdx), tools/pcm_bytes_check.cpp walks the same
// (tile, lane) grid on the CPU over exactly-sized heap buffers.
//
// A packed sample is B = 1..3 bytes, little or big endian, signed or
// unsigned (unsigned: value = raw - 2^(8B-1)); the ten layouts are the
// reference's FrameList_get_char_to_int_converter / int_to_char set
// (src/pcm.c, src/pcmconv.c).  The integer side is interleaved int32 or
// int16.  Work is a table of runs {byte_offset, samples, sample_offset}; a
// run is cut into tiles of kPbTile samples and a workgroup takes one tile.
//
// Memory contract (the functions below hold it, the checker proves it):
//   unpack reads the packed bytes as aligned dwords, and only dwords that
//     hold at least one byte of the run; the tail of a run (samples % N)
//     is read bytewise.  It writes whole 16-byte groups of N samples, so a
//     run's sample_offset must be a multiple of N (16 / sizeof sample).
//   pack   writes aligned 16-byte units that lie wholly inside the run's
//     packed range, and the bytes before the first and after the last such
//     unit one at a time: never a byte outside the range, and no
//     read-modify-write.  It reads only the run's own samples.
//   every index is 64-bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PB_HD __host__ __device__ __forceinline__
#define PB_UNROLL _Pragma("unroll")
#else
#define PB_HD inline
#define PB_UNROLL
#endif

constexpr uint32_t kPbTile = 4096; // samples per tile
constexpr uint32_t kPbBlock = 256; // lanes per tile; at least 32 (pack's edges)

// a run as the kernels see it
struct PbRun {
    uint64_t byte_offset, samples, sample_offset;
    uint64_t tile0; // first tile of the run in the launch's tile list
};

struct alignas(16) PbVec16 {
    uint32_t d[4];
};

template <int B, bool BE, bool SGN> struct PbLayout {
    static constexpr int kShift = 32 - 8 * B;
    // raw: the sample's bytes in memory order, the first in bits 0..7; bits
    // above 8B may hold anything
    static PB_HD int32_t decode(uint32_t raw)
    {
        const uint32_t top = BE ? __builtin_bswap32(raw) : raw << kShift;
        if (SGN)
            return (int32_t)top >> kShift;
        return (int32_t)(top >> kShift) - (int32_t)(1u << (8 * B - 1));
    }
    // -> the B bytes in memory order in bits 0..8B-1, zero above: the value
    // (plus 2^(8B-1) when unsigned) masked to 8B bits, as FrameList.to_bytes
    static PB_HD uint32_t encode(int32_t v)
    {
        const uint32_t u = (uint32_t)v + (SGN ? 0u : 1u << (8 * B - 1));
        return BE ? __builtin_bswap32(u << kShift) : (u << kShift) >> kShift;
    }
};

// the low dword of (hi:lo) >> sh, sh in {0, 8, 16, 24}
static PB_HD uint32_t pb_funnel(uint32_t lo, uint32_t hi, uint32_t sh)
{
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
}

static PB_HD uint64_t pb_min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
static PB_HD uint64_t pb_max64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// the run whose tiles hold launch tile `tile`: the last with tile0 <= tile
// (runs without tiles share the tile0 of the run after them)
static PB_HD uint32_t pb_run_of_tile(const PbRun *runs, uint32_t n, uint64_t tile)
{
    uint32_t l = 0, r = n;
    while (r - l > 1) {
        const uint32_t m = l + ((r - l) >> 1);
        if (runs[m].tile0 <= tile)
            l = m;
        else
            r = m;
    }
    return l;
}

// ---------------------------------------------------------------- unpack

static PB_HD uint64_t pb_unpack_tiles(uint64_t samples)
{
    return samples / kPbTile + (samples % kPbTile ? 1 : 0);
}

// N = 16 / sizeof(T) samples from the N * B bytes at byte address `addr` of
// `bytes` (any alignment) to the 16-byte aligned dst
template <int B, bool BE, bool SGN, typename T>
static PB_HD void pb_unpack_unit(const uint8_t *bytes, uint64_t addr, T *dst)
{
    constexpr int N = 16 / (int)sizeof(T);
    constexpr int K = N * B / 4; // dwords of packed data: 1, 2, 3 or 4
    static_assert(N * B % 4 == 0, "a unit is whole dwords");
    const uint32_t *w = reinterpret_cast<const uint32_t *>(bytes + (addr & ~(uint64_t)3));
    const uint32_t sh = ((uint32_t)addr & 3u) * 8u;
    // a[]: the unit's bytes moved down to byte 0.  The dword after the last
    // is touched only when the unit reaches into it.
    uint32_t a[K];
    uint32_t lo = w[0];
    PB_UNROLL
    for (int i = 0; i < K; ++i) {
        const uint32_t hi = (i + 1 < K || sh) ? w[i + 1] : 0u;
        a[i] = pb_funnel(lo, hi, sh);
        lo = hi;
    }
    int32_t v[N];
    PB_UNROLL
    for (int j = 0; j < N; ++j) {
        constexpr int kB = B;
        const int q = j * kB / 4, r = j * kB % 4;
        uint32_t raw = a[q] >> (8 * r);
        if (r + kB > 4)
            raw |= a[q + 1] << (32 - 8 * r);
        v[j] = PbLayout<B, BE, SGN>::decode(raw);
    }
    PbVec16 o;
    if (sizeof(T) == 4) {
        PB_UNROLL
        for (int j = 0; j < 4; ++j)
            o.d[j] = (uint32_t)v[j];
    } else {
        PB_UNROLL
        for (int j = 0; j < 4; ++j)
            o.d[j] = ((uint32_t)v[2 * j % N] & 0xFFFFu) | ((uint32_t)v[(2 * j + 1) % N] << 16);
    }
    *reinterpret_cast<PbVec16 *>(dst) = o;
}

// what lane `lane` of `block` does in tile `tile_in_run` of run r
template <int B, bool BE, bool SGN, typename T>
static PB_HD void pb_unpack_lane(const uint8_t *bytes, T *pcm, const PbRun &r,
                                 uint64_t tile_in_run, uint32_t lane, uint32_t block)
{
    constexpr uint32_t N = 16 / (uint32_t)sizeof(T);
    const uint64_t s_begin = tile_in_run * kPbTile;
    const uint64_t s_end = pb_min64(s_begin + kPbTile, r.samples);
    for (uint64_t s = s_begin + (uint64_t)lane * N; s < s_end; s += (uint64_t)block * N) {
        if (s + N <= s_end) {
            pb_unpack_unit<B, BE, SGN, T>(bytes, r.byte_offset + s * B, pcm + r.sample_offset + s);
        } else {
            // the run's last samples % N, one at a time
            for (uint64_t t = s; t < s_end; ++t) {
                const uint8_t *p = bytes + r.byte_offset + t * B;
                uint32_t raw = p[0];
                if (B > 1)
                    raw |= (uint32_t)p[B > 1 ? 1 : 0] << 8;
                if (B > 2)
                    raw |= (uint32_t)p[B > 2 ? 2 : 0] << 16;
                pcm[r.sample_offset + t] = (T)PbLayout<B, BE, SGN>::decode(raw);
            }
        }
    }
}

// ------------------------------------------------------------------ pack

// aligned 16-byte units wholly inside the run's packed range [p0, p1)
template <int B> static PB_HD uint64_t pb_pack_units(const PbRun &r)
{
    const uint64_t p0 = r.byte_offset, p1 = p0 + r.samples * B;
    const uint64_t u0 = (p0 + 15) & ~(uint64_t)15, u1 = p1 & ~(uint64_t)15;
    return u1 > u0 ? (u1 - u0) / 16 : 0;
}

// a tile of pack is kPbTile samples' worth of units; a run that has samples
// has at least one tile, which also writes its edge bytes
template <int B> static PB_HD uint64_t pb_pack_tiles(const PbRun &r)
{
    constexpr uint64_t UT = (uint64_t)kPbTile * B / 16;
    if (!r.samples)
        return 0;
    const uint64_t u = pb_pack_units<B>(r);
    return u ? (u + UT - 1) / UT : 1;
}

// the 16 bytes at packed position `rel` (from the run's first byte) to dst16
// (16-byte aligned); src is the run's first sample
template <int B, bool BE, bool SGN, typename T>
static PB_HD void pb_pack_unit(const T *src, uint64_t rel, uint8_t *dst16)
{
    constexpr int M = (16 + 2 * (B - 1)) / B; // samples a unit can touch: 16, 9, 6
    const uint64_t s0 = rel / B;
    const uint32_t phase = (uint32_t)(rel % B); // bytes of sample s0 before the unit
    // c[]: samples s0 .. s0+M-1 packed from byte 0
    uint32_t c[5] = {0u, 0u, 0u, 0u, 0u};
    PB_UNROLL
    for (int i = 0; i < M; ++i) {
        constexpr int kB = B;
        const int q = i * kB / 4, sh = i * kB % 4;
        // sample s0 + i is read only if one of its bytes is in the unit
        const bool need = (uint32_t)(i * kB) < phase + 16u;
        const uint32_t raw = need ? PbLayout<B, BE, SGN>::encode((int32_t)src[s0 + i]) : 0u;
        c[q] |= raw << (8 * sh);
        if (sh + kB > 4)
            c[q + 1] |= raw >> (32 - 8 * sh);
    }
    PbVec16 o;
    PB_UNROLL
    for (int i = 0; i < 4; ++i)
        o.d[i] = pb_funnel(c[i], c[i + 1], 8u * phase);
    *reinterpret_cast<PbVec16 *>(dst16) = o;
}

// one byte of the packed image, at position `rel` of the run
template <int B, bool BE, bool SGN, typename T>
static PB_HD void pb_pack_byte(const T *src, uint64_t rel, uint8_t *dst)
{
    const uint32_t raw = PbLayout<B, BE, SGN>::encode((int32_t)src[rel / B]);
    *dst = (uint8_t)(raw >> (8u * (uint32_t)(rel % B)));
}

template <int B, bool BE, bool SGN, typename T>
static PB_HD void pb_pack_lane(const T *pcm, uint8_t *bytes, const PbRun &r, uint64_t tile_in_run,
                               uint32_t lane, uint32_t block)
{
    constexpr uint64_t UT = (uint64_t)kPbTile * B / 16;
    const T *src = pcm + r.sample_offset;
    const uint64_t p0 = r.byte_offset, p1 = p0 + r.samples * B;
    const uint64_t u0 = (p0 + 15) & ~(uint64_t)15, u1 = p1 & ~(uint64_t)15;
    const uint64_t n_units = u1 > u0 ? (u1 - u0) / 16 : 0;
    const uint64_t u_end = pb_min64((tile_in_run + 1) * UT, n_units);
    for (uint64_t u = tile_in_run * UT + lane; u < u_end; u += block)
        pb_pack_unit<B, BE, SGN, T>(src, u0 + 16 * u - p0, bytes + u0 + 16 * u);
    if (tile_in_run == 0 && lane < 32) {
        // [p0, head_end) before the first unit, [tail_begin, p1) after the
        // last: at most 15 bytes each, all of a run that holds no unit
        const uint64_t head_end = pb_min64(u0, p1);
        const uint64_t tail_begin = pb_max64(u1, head_end);
        const uint64_t b = lane < 16 ? p0 + lane : tail_begin + (lane - 16);
        if (b < (lane < 16 ? head_end : p1))
            pb_pack_byte<B, BE, SGN, T>(src, b - p0, bytes + b);
    }
}
