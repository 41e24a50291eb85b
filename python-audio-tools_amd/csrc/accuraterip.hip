// accuraterip.hip — AccurateRip v1/v2 checksums of a batch of CD tracks, and
// v1 at every drive read offset in [-K, K] (trackverify -R; the reference's
// audiotools._accuraterip.ChecksumV1 / ChecksumV2).
//
// Arithmetic.  A track is stereo 16-bit.  Frame i (from 1) has the value
//     w = (uint16(right) << 16) | uint16(left)
// and the index g = index0 + i.  It counts when start <= g <= end, with
// start = 5 CD frames' worth of PCM frames on a first track (else 0) and
// end = (uint32)(total - that skip) on a last track (else total).  The cast
// wraps when the track is shorter than the skip, so nothing is cut then.
//     v1 = sum w * g                      (mod 2^32)
//     v2 = sum lo32(w * g) + hi32(w * g)  (mod 2^32, the product in 64 bits)
//
// Pass 1 (k_ar_tiles) streams the included frames once.  The buffer is cut
// into tiles of kTile frames aligned in absolute position, a track's range
// covers a run of tiles, and workgroups walk the batch's tiles grid-stride:
// which track a tile belongs to is a binary search over the tracks' first
// tile numbers, so three long tracks spread over the machine as 1024 do.
// A lane reads aligned 16-byte groups and keeps three uint32 sums: of the
// values, of the products' low words, of their high words.  They are reduced
// over the wave by shuffles, over the workgroup through LDS, and stored per
// tile; pass 2 (k_ar_tracks) adds a track's tiles.  Integer sums mod 2^32 do
// not depend on the order, so the results are the same for every schedule.
//
// Offset sweep (k_ar_sweep).  At offset k frame i is read from position
// pcm_offset + k + i - 1, silence outside the track's readable region.  With
// j = i + k the included frames are j in [a + k, b + k] and
//     v1(k) = sum w_j * (index0 + j)  -  k * sum w_j
// so with F and G the prefix sums of w_j * (index0 + j) and of w_j
//     v1(k) = [F(b+k) - F(a-1+k)] - k * [G(b+k) - G(a-1+k)]
//           = v1(0) + D_F(k) - k * (S(0) + D_G(k)),
//     D_X(k) = [X(b+k) - X(b)] - [X(a-1+k) - X(a-1)].
// D is a running sum over the 2K frames around each of the two edges, one
// workgroup scan per side of zero; the track itself is not read again.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/atgpu.h"
#include "host_common.h"
#include "table_search.h"
#include "wave.h"

namespace {

thread_local ErrSlot g_ar_err;
#define AHIP(expr) ATG_HIP_TRY(g_ar_err, expr, #expr)

constexpr uint32_t kTile = 4096;  // PCM frames per tile
constexpr uint32_t kBlock = 256;
constexpr uint32_t kMaxBlocks = 2048;
constexpr uint32_t kMaxOffset = 65535;

// what the kernels know of a track
struct ArTrack {
    long long pos0;       // buffer position of frame 1 (pcm_offset, may be < 0)
    long long a, b;       // included frames a..b (1-based); a = 1, b = 0 when none
    uint64_t lo, hi;      // readable region [lo, hi) in buffer positions
    uint64_t rd0, rd1;    // positions pass 1 reads: included and readable
    uint64_t tile0;       // first tile of the track in the batch's tile list
    uint64_t first_tile;  // rd0 / kTile
    uint32_t index0;
    uint32_t pad;
};

struct ArCtx {
    DevBuf tracks, tiles, sums, sweep;
};
DeviceContexts<ArCtx> g_ctxs;

template <int FMT> struct Pcm;
template <> struct Pcm<ATG_PCM_S32> {
    static constexpr uint32_t kGroup = 2; // frames per 16-byte load
    static __device__ __forceinline__ uint32_t pack(int l, int r)
    {
        return ((uint32_t)r << 16) | ((uint32_t)l & 0xFFFFu);
    }
    static __device__ __forceinline__ void group(const void *pcm, uint64_t p, uint32_t (&w)[4])
    {
        const int4 v = *reinterpret_cast<const int4 *>((const int32_t *)pcm + 2 * p);
        w[0] = pack(v.x, v.y);
        w[1] = pack(v.z, v.w);
    }
    static __device__ __forceinline__ uint32_t one(const void *pcm, uint64_t p)
    {
        const int2 v = *reinterpret_cast<const int2 *>((const int32_t *)pcm + 2 * p);
        return pack(v.x, v.y);
    }
};
template <> struct Pcm<ATG_PCM_S16> {
    static constexpr uint32_t kGroup = 4;
    // little-endian: left in the low half, right in the high half already
    static __device__ __forceinline__ void group(const void *pcm, uint64_t p, uint32_t (&w)[4])
    {
        const uint4 v = *reinterpret_cast<const uint4 *>((const uint32_t *)pcm + p);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
    }
    static __device__ __forceinline__ uint32_t one(const void *pcm, uint64_t p)
    {
        return ((const uint32_t *)pcm)[p];
    }
};

struct Sums {
    uint32_t s, lo, hi;
    __device__ __forceinline__ void add(uint32_t w, uint32_t g)
    {
        const uint64_t prod = (uint64_t)w * g;
        s += w;
        lo += (uint32_t)prod;
        hi += (uint32_t)(prod >> 32);
    }
};

// the track whose tile run holds batch tile `tile`
__device__ __forceinline__ uint32_t track_of_tile(const ArTrack *tr, uint32_t n, uint64_t tile)
{
    return last_le(tr, n, tile, &ArTrack::tile0);
}

// pass 1: per-tile sums (x = values, y = low words, z = high words)
template <int FMT>
__global__ __launch_bounds__(kBlock) void k_ar_tiles(const void *__restrict__ pcm,
                                                     const ArTrack *__restrict__ tr, uint32_t n,
                                                     uint64_t n_tiles, uint4 *__restrict__ out)
{
    constexpr uint32_t G = Pcm<FMT>::kGroup;
    constexpr uint32_t kRounds = kTile / (G * kBlock);
    __shared__ uint32_t red[3][kBlock / 64];
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t t = track_of_tile(tr, n, tile);
        const uint64_t rd0 = tr[t].rd0, rd1 = tr[t].rd1;
        // index of the frame at position p: index0 + (p - pos0 + 1)
        const uint32_t bias = tr[t].index0 + 1u - (uint32_t)tr[t].pos0;
        const uint64_t base = (tr[t].first_tile + (tile - tr[t].tile0)) * kTile;
        Sums acc = {0, 0, 0};
#pragma unroll
        for (uint32_t r = 0; r < kRounds; ++r) {
            const uint64_t p = base + (uint64_t)(r * kBlock + threadIdx.x) * G;
            if (p >= rd0 && p + G <= rd1) {
                uint32_t w[4];
                Pcm<FMT>::group(pcm, p, w);
#pragma unroll
                for (uint32_t f = 0; f < G; ++f)
                    acc.add(w[f], (uint32_t)p + f + bias);
            } else if (p + G > rd0 && p < rd1) {
                for (uint32_t f = 0; f < G; ++f)
                    if (p + f >= rd0 && p + f < rd1)
                        acc.add(Pcm<FMT>::one(pcm, p + f), (uint32_t)p + f + bias);
            }
        }
        acc.s = wave_sum_u32(acc.s);
        acc.lo = wave_sum_u32(acc.lo);
        acc.hi = wave_sum_u32(acc.hi);
        if ((threadIdx.x & 63) == 0) {
            red[0][threadIdx.x >> 6] = acc.s;
            red[1][threadIdx.x >> 6] = acc.lo;
            red[2][threadIdx.x >> 6] = acc.hi;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint4 o = {0, 0, 0, 0};
            for (uint32_t w = 0; w < kBlock / 64; ++w) {
                o.x += red[0][w];
                o.y += red[1][w];
                o.z += red[2][w];
            }
            out[tile] = o;
        }
        __syncthreads();
    }
}

// pass 2: a track's tiles added up; x = v1, y = v2, z = sum of values
__global__ __launch_bounds__(kBlock) void k_ar_tracks(const ArTrack *__restrict__ tr, uint32_t n,
                                                      uint64_t n_tiles,
                                                      const uint4 *__restrict__ tiles,
                                                      uint4 *__restrict__ sums)
{
    __shared__ uint32_t red[3][kBlock / 64];
    const uint32_t t = blockIdx.x;
    const uint64_t t0 = tr[t].tile0, t1 = t + 1 < n ? tr[t + 1].tile0 : n_tiles;
    uint32_t s = 0, lo = 0, hi = 0;
    for (uint64_t i = t0 + threadIdx.x; i < t1; i += kBlock) {
        const uint4 v = tiles[i];
        s += v.x;
        lo += v.y;
        hi += v.z;
    }
    s = wave_sum_u32(s);
    lo = wave_sum_u32(lo);
    hi = wave_sum_u32(hi);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s;
        red[1][threadIdx.x >> 6] = lo;
        red[2][threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        s = lo = hi = 0;
        for (uint32_t w = 0; w < kBlock / 64; ++w) {
            s += red[0][w];
            lo += red[1][w];
            hi += red[2][w];
        }
        sums[t] = uint4{lo, lo + hi, s, 0};
    }
}

// the value at 1-based frame coordinate j of track T (silence outside the
// region) and its product with the index there
template <int FMT>
__device__ __forceinline__ void edge_term(const void *pcm, const ArTrack &T, long long j,
                                          uint32_t &w, uint32_t &wg)
{
    const long long p = T.pos0 + j - 1;
    w = 0;
    if (p >= 0 && (uint64_t)p >= T.lo && (uint64_t)p < T.hi)
        w = Pcm<FMT>::one(pcm, (uint64_t)p);
    wg = w * (T.index0 + (uint32_t)j);
}

// sweep: blockIdx.y = 0 writes k = 0 .. K, 1 writes k = -1 .. -K
template <int FMT>
__global__ __launch_bounds__(kBlock) void k_ar_sweep(const void *__restrict__ pcm,
                                                     const ArTrack *__restrict__ tr,
                                                     const uint4 *__restrict__ sums, uint32_t K,
                                                     uint32_t *__restrict__ out)
{
    __shared__ uint32_t wtot[2][kBlock / 64];
    const ArTrack T = tr[blockIdx.x];
    const uint4 base = sums[blockIdx.x];
    const bool neg = blockIdx.y != 0;
    uint32_t *row = out + (uint64_t)blockIdx.x * (2 * K + 1) + K; // row[k]
    if (!neg && threadIdx.x == 0)
        row[0] = base.x;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t run_f = 0, run_g = 0; // D_F, D_G up to the last chunk
    for (uint32_t m0 = 1; m0 <= K; m0 += kBlock) {
        const uint32_t m = m0 + threadIdx.x;
        uint32_t df = 0, dg = 0;
        if (m <= K) {
            uint32_t wb, fb, wa, fa;
            // k = +m adds frame b+m and drops a-1+m; k = -m drops b-m+1, adds a-m
            edge_term<FMT>(pcm, T, neg ? T.b - m + 1 : T.b + m, wb, fb);
            edge_term<FMT>(pcm, T, neg ? T.a - m : T.a - 1 + m, wa, fa);
            df = neg ? fa - fb : fb - fa;
            dg = neg ? wa - wb : wb - wa;
        }
        // inclusive scan over the workgroup
        df = wave_incl_scan_u32(df, (int)lane);
        dg = wave_incl_scan_u32(dg, (int)lane);
        if (lane == 63) {
            wtot[0][wave] = df;
            wtot[1][wave] = dg;
        }
        __syncthreads();
        uint32_t cf = run_f, cg = run_g, tf = 0, tg = 0;
        for (uint32_t w = 0; w < kBlock / 64; ++w) {
            if (w < wave) {
                cf += wtot[0][w];
                cg += wtot[1][w];
            }
            tf += wtot[0][w];
            tg += wtot[1][w];
        }
        run_f += tf;
        run_g += tg;
        __syncthreads();
        if (m <= K) {
            const uint32_t k = neg ? 0u - m : m;
            const uint32_t v = base.x + (cf + df) - k * (base.z + cg + dg);
            if (neg)
                row[-(long long)m] = v;
            else
                row[m] = v;
        }
    }
}

atg_status check_args(const void *pcm, int format, const atg_ar_track *tracks, uint32_t n,
                      uint32_t max_offset, const atg_ar_result *results,
                      const uint32_t *offset_v1)
{
    if (n && (!pcm || !tracks || !results))
        return g_ar_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (format != ATG_PCM_S16 && format != ATG_PCM_S32)
        return g_ar_err.fail(ATG_ERR_INVALID, "unknown PCM format");
    if (max_offset > kMaxOffset)
        return g_ar_err.fail(ATG_ERR_UNSUPPORTED, "max_offset above 65535");
    if (n && max_offset && !offset_v1)
        return g_ar_err.fail(ATG_ERR_INVALID, "offset_v1 is NULL with max_offset > 0");
    for (uint32_t t = 0; t < n; ++t) {
        const atg_ar_track &a = tracks[t];
        if (!a.sample_rate)
            return g_ar_err.fail(ATG_ERR_INVALID, "sample rate must be > 0");
        if (!a.pcm_frames || !a.total_pcm_frames)
            return g_ar_err.fail(ATG_ERR_INVALID, "total PCM frames must be > 0");
        if (a.lo_frame > a.hi_frame)
            return g_ar_err.fail(ATG_ERR_INVALID, "lo_frame above hi_frame");
        if (a.pcm_frames >= (1ull << 32) || a.index0 + a.pcm_frames >= (1ull << 32))
            return g_ar_err.fail(ATG_ERR_INVALID, "index0 + pcm_frames does not fit 32 bits");
        if (a.hi_frame >= (1ull << 62) || a.pcm_offset >= (1ll << 62) ||
            a.pcm_offset <= -(1ll << 62))
            return g_ar_err.fail(ATG_ERR_INVALID, "frame position out of range");
    }
    return ATG_OK;
}

// the track as the kernels see it; tile0 is filled in by the caller
ArTrack plan_track(const atg_ar_track &a)
{
    const uint32_t skip = a.sample_rate / 75 * 5;
    const uint64_t start = (a.flags & ATG_AR_FIRST) ? skip : 0;
    // the reference's cast to unsigned: wraps for a last track shorter than the skip
    const uint64_t end = (a.flags & ATG_AR_LAST) ? (uint32_t)(a.total_pcm_frames - skip)
                                                 : a.total_pcm_frames;
    const uint64_t g0 = std::max<uint64_t>((uint64_t)a.index0 + 1, start);
    const uint64_t g1 = std::min<uint64_t>((uint64_t)a.index0 + a.pcm_frames, end);
    ArTrack T = {};
    T.pos0 = a.pcm_offset;
    T.lo = a.lo_frame;
    T.hi = a.hi_frame;
    T.index0 = a.index0;
    T.a = 1;
    T.b = 0;
    if (g0 <= g1) {
        T.a = (long long)(g0 - a.index0);
        T.b = (long long)(g1 - a.index0);
        // positions of frames a..b, cut to the region
        const long long p0 = std::max<long long>(T.pos0 + T.a - 1, (long long)T.lo);
        const long long p1 = std::min<long long>(T.pos0 + T.b, (long long)T.hi);
        if (p0 < p1) {
            T.rd0 = (uint64_t)p0;
            T.rd1 = (uint64_t)p1;
        }
    }
    T.first_tile = T.rd0 / kTile;
    return T;
}

uint64_t track_tiles(const ArTrack &T)
{
    return T.rd1 > T.rd0 ? (T.rd1 + kTile - 1) / kTile - T.first_tile : 0;
}

template <int FMT>
void launch_all(const void *d_pcm, const ArTrack *d_tr, uint32_t n, uint64_t n_tiles,
                uint4 *d_tiles, uint4 *d_sums, uint32_t K, uint32_t *d_sweep, hipStream_t s)
{
    if (n_tiles)
        hipLaunchKernelGGL(k_ar_tiles<FMT>, dim3((uint32_t)std::min<uint64_t>(n_tiles, kMaxBlocks)),
                           dim3(kBlock), 0, s, d_pcm, d_tr, n, n_tiles, d_tiles);
    hipLaunchKernelGGL(k_ar_tracks, dim3(n), dim3(kBlock), 0, s, d_tr, n, n_tiles,
                       (const uint4 *)d_tiles, d_sums);
    if (K)
        hipLaunchKernelGGL(k_ar_sweep<FMT>, dim3(n, 2), dim3(kBlock), 0, s, d_pcm, d_tr,
                           (const uint4 *)d_sums, K, d_sweep);
}

} // namespace

extern "C" {

const char *atg_accuraterip_last_error(void) { return g_ar_err.msg.c_str(); }

atg_status atg_accuraterip_device(const void *d_pcm, int format, const atg_ar_track *tracks,
                                  uint32_t n, uint32_t max_offset, atg_ar_result *results,
                                  uint32_t *offset_v1, void *stream)
{
    atg_status st = check_args(d_pcm, format, tracks, n, max_offset, results, offset_v1);
    if (st != ATG_OK)
        return st;
    if (n && ((uintptr_t)d_pcm & 15u))
        return g_ar_err.fail(ATG_ERR_INVALID, "d_pcm must be 16-byte aligned");
    if (!n)
        return ATG_OK;
    hipStream_t s = (hipStream_t)stream;
    DeviceContexts<ArCtx>::Held held; // where the PCM is
    if ((st = g_ctxs.hold(d_pcm, g_ar_err, held)) != ATG_OK)
        return st;
    ArCtx &c = *held;
    std::vector<ArTrack> tr(n);
    uint64_t n_tiles = 0;
    for (uint32_t t = 0; t < n; ++t) {
        tr[t] = plan_track(tracks[t]);
        tr[t].tile0 = n_tiles;
        n_tiles += track_tiles(tr[t]);
    }
    const uint64_t width = 2ull * max_offset + 1;
    AHIP(c.tracks.ensure(sizeof(ArTrack) * n));
    AHIP(c.tiles.ensure(sizeof(uint4) * std::max<uint64_t>(n_tiles, 1)));
    AHIP(c.sums.ensure(sizeof(uint4) * n));
    if (max_offset)
        AHIP(c.sweep.ensure(sizeof(uint32_t) * width * n));
    AHIP(hipMemcpyAsync(c.tracks.p, tr.data(), sizeof(ArTrack) * n, hipMemcpyHostToDevice, s));
    if (format == ATG_PCM_S32)
        launch_all<ATG_PCM_S32>(d_pcm, (const ArTrack *)c.tracks.p, n, n_tiles, (uint4 *)c.tiles.p,
                                (uint4 *)c.sums.p, max_offset, (uint32_t *)c.sweep.p, s);
    else
        launch_all<ATG_PCM_S16>(d_pcm, (const ArTrack *)c.tracks.p, n, n_tiles, (uint4 *)c.tiles.p,
                                (uint4 *)c.sums.p, max_offset, (uint32_t *)c.sweep.p, s);
    AHIP(hipGetLastError());
    std::vector<uint4> sums(n);
    AHIP(hipMemcpyAsync(sums.data(), c.sums.p, sizeof(uint4) * n, hipMemcpyDeviceToHost, s));
    if (max_offset)
        AHIP(hipMemcpyAsync(offset_v1, c.sweep.p, sizeof(uint32_t) * width * n,
                            hipMemcpyDeviceToHost, s));
    AHIP(hipStreamSynchronize(s));
    for (uint32_t t = 0; t < n; ++t) {
        results[t].v1 = sums[t].x;
        results[t].v2 = sums[t].y;
        results[t].status = 0;
        results[t].reserved = 0;
    }
    if (!max_offset && offset_v1)
        for (uint32_t t = 0; t < n; ++t)
            offset_v1[t] = sums[t].x;
    return ATG_OK;
}

atg_status atg_accuraterip_host(int device, const void *pcm, int format,
                                uint64_t pcm_frames_total, const atg_ar_track *tracks, uint32_t n,
                                uint32_t max_offset, atg_ar_result *results, uint32_t *offset_v1)
{
    atg_status st = check_args(pcm, format, tracks, n, max_offset, results, offset_v1);
    if (st != ATG_OK)
        return st;
    for (uint32_t t = 0; t < n; ++t)
        if (tracks[t].hi_frame > pcm_frames_total)
            return g_ar_err.fail(ATG_ERR_INVALID, "hi_frame beyond the PCM buffer");
    if (!n)
        return ATG_OK;
    if ((st = use_device(device, g_ar_err)) != ATG_OK)
        return st;
    const size_t bytes = (size_t)pcm_frames_total * (format == ATG_PCM_S32 ? 8 : 4);
    DevTemp d;
    ATG_HIP_TRY(g_ar_err, d.alloc(std::max<size_t>(bytes, 16)),
                "hipMalloc(&d, std::max<size_t>(bytes, 16))");
    if (bytes)
        ATG_HIP_TRY(g_ar_err, hipMemcpy(d.p, pcm, bytes, hipMemcpyHostToDevice), "hipMemcpy");
    return atg_accuraterip_device(d.p, format, tracks, n, max_offset, results, offset_v1, nullptr);
}

uint32_t atg_accuraterip_tile_frames(void) { return kTile; }

} // extern "C"
