// aob_decode.hip — DVD-Audio titles on the device: AOB sector demux and the
// packed-PCM codec (the reference's src/decoders/aob.c and aobpcm.c).
//
// An AOB file is a run of independent 2048-byte sectors, so nothing here
// walks serially through a file:
//   sectors  one lane per sector of the whole batch parses its pack header
//            and walks its packets (aob_walk_sector, aob_common.h) and
//            writes one 16-byte record.
//   layout   one workgroup per title: first bad sector (minimum reduction),
//            exclusive 64-bit prefix sum of the payload lengths before it,
//            and the title's result from its first sector's record.
//   pcm      gather and un-swizzle fused.  The output is cut into tiles of
//            kAobTileChunks chunks (two frames each); workgroups walk the
//            tiles grid-stride, find a tile's title by search over the runs'
//            first tile numbers and its first source sector by search in the
//            prefix table, stage the tile's stream bytes in LDS from aligned
//            16-byte reads of the sectors (a chunk may straddle any number
//            of sectors), then every lane makes one 16-byte store of
//            samples cut out of the staged bytes through the layout's
//            inverse byte order.  The AOB bytes are read once and the PCM
//            written once; no contiguous payload buffer exists.
// Streaming, no reuse: the roofline is HBM bandwidth over AOB bytes read
// plus PCM bytes written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/atgpu.h"
#include "aob_common.h"
#include "aob_passes.h"
#include "host_common.h"
#include "table_search.h"
#include "wave.h"

namespace {

thread_local ErrSlot g_aob_err;
#define AHIP(expr) ATG_HIP_TRY(g_aob_err, expr, #expr)

constexpr uint32_t kMaxBlocks = 4096;
constexpr int kStages = 3;
const char *const kStageNames[kStages] = {"sectors", "layout", "pcm"};

thread_local StageTimes<kStages> g_aob_times;

// a title with PCM to write: its tiles are [tile0, next run's tile0)
struct AobRun {
    uint64_t byte_offset, sample_offset, chunks, tile0;
    uint32_t sec0, n_valid, channels, bytes_per_sample;
};

__constant__ AobInverse24 c_inv24 = aob_inverse24();

__global__ __launch_bounds__(kAobBlock) void k_aob_layout(const AobTitle *__restrict__ titles,
                                                          const atg_aob_sector *__restrict__ sectors,
                                                          AobPrefix *__restrict__ prefix,
                                                          atg_aob_result *__restrict__ results)
{
    const AobTitle t = titles[blockIdx.x];
    uint32_t bad;
    uint64_t carry;
    aob_layout_title(t, sectors + t.sec0, prefix + t.sec0, &bad, &carry);
    if (threadIdx.x == 0)
        results[blockIdx.x] = aob_title_result(sectors + t.sec0, t.n_sectors, bad, carry);
}

// sample n of the tile from its staged stream bytes
template <typename T>
__device__ __forceinline__ T aob_sample16(const uint8_t *stage, uint32_t n)
{
    return (T)(int16_t)(((uint32_t)stage[2 * n] << 8) | stage[2 * n + 1]);
}

template <typename T>
__global__ __launch_bounds__(kAobBlock) void k_aob_pcm(const uint8_t *__restrict__ bytes,
                                                       const atg_aob_sector *__restrict__ sectors,
                                                       const AobPrefix *__restrict__ prefix,
                                                       const AobRun *__restrict__ runs,
                                                       uint32_t n_runs, uint64_t n_tiles,
                                                       T *__restrict__ out)
{
    constexpr uint32_t G = 16 / sizeof(T); // samples per 16-byte store
    __shared__ uint4 s_stage4[kAobStageBytes / 16];
    __shared__ uint8_t s_inv[kAobMaxChunk];
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_stage4);
    const uint32_t tid = threadIdx.x;

    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const AobRun r = runs[last_le(runs, n_runs, tile, &AobRun::tile0)];
        const uint32_t B = r.bytes_per_sample, per = 2 * r.channels, chunk = B * per;
        const uint64_t c0 = (tile - r.tile0) * kAobTileChunks;
        const uint32_t nc = (uint32_t)min((uint64_t)kAobTileChunks, r.chunks - c0);
        const uint64_t b0 = c0 * chunk, b1 = b0 + (uint64_t)nc * chunk;
        const AobPrefix *pre = prefix + r.sec0;
        const atg_aob_sector *sec = sectors + r.sec0;

        if (B == 3 && tid < chunk)
            s_inv[tid] = c_inv24.at[r.channels - 1][tid];

        // stage stream bytes [b0, b1): half a workgroup per sector, a lane
        // per aligned 16-byte unit of it
        const uint32_t unit = tid % kAobUnits, ua = unit * 16;
        for (uint32_t s = last_le(pre, r.n_valid, b0, &AobPrefix::start) + tid / kAobUnits;
             s < r.n_valid; s += kAobBlock / kAobUnits) {
            const uint64_t p = pre[s].start;
            if (p >= b1)
                break;
            const uint32_t off = sec[s].payload_offset, len = sec[s].payload_length;
            const uint64_t a = max(p, b0), e = min(p + len, b1);
            if (a >= e)
                continue;
            // the sector's bytes [sa, se) go to stage[dst ...]
            const uint32_t sa = off + (uint32_t)(a - p), se = off + (uint32_t)(e - p);
            if (ua + 16 <= sa || ua >= se)
                continue;
            const uint4 v = *reinterpret_cast<const uint4 *>(
                bytes + r.byte_offset + (uint64_t)s * kAobSector + ua);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const int32_t dst = (int32_t)(a - b0) + (int32_t)ua - (int32_t)sa;
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k)
                if (ua + k >= sa && ua + k < se)
                    stage[dst + (int32_t)k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
        __syncthreads();

        const uint32_t n_samples = nc * per;
        T *dst = out + r.sample_offset + c0 * per;
        for (uint32_t g = tid; g * G < n_samples; g += kAobBlock) {
            const uint32_t n0 = g * G;
            alignas(16) T v[G];
            if (B == 2) {
#pragma unroll
                for (uint32_t k = 0; k < G; ++k)
                    v[k] = n0 + k < n_samples ? aob_sample16<T>(stage, n0 + k) : (T)0;
            } else {
                uint32_t c = n0 / per, j = n0 - c * per;
#pragma unroll
                for (uint32_t k = 0; k < G; ++k) {
                    T x = 0;
                    if (n0 + k < n_samples) {
                        const uint8_t *ch = stage + c * chunk;
                        const uint32_t lo = ch[s_inv[3 * j]], mid = ch[s_inv[3 * j + 1]];
                        const int32_t hi = (int8_t)ch[s_inv[3 * j + 2]];
                        x = (T)(hi * 65536 + (int32_t)((mid << 8) | lo));
                    }
                    v[k] = x;
                    if (++j == per) {
                        j = 0;
                        ++c;
                    }
                }
            }
            if (n0 + G <= n_samples) {
                *reinterpret_cast<uint4 *>(dst + n0) = *reinterpret_cast<const uint4 *>(v);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < G; ++k)
                    if (n0 + k < n_samples)
                        dst[n0 + k] = v[k];
            }
        }
        __syncthreads(); // the next tile overwrites the stage
    }
}

// per device: the tables and the events that time the passes
struct AobCtx {
    DevBuf titles, sectors, prefix, results, runs;
    hipEvent_t ev[kStages + 1] = {};
};
DeviceContexts<AobCtx> g_ctxs;

atg_status check_args(bool aligned, const void *bytes, uint64_t bytes_cap,
                      const atg_aob_title *titles, uint32_t n, int format,
                      const atg_aob_result *results, uint64_t *n_sectors)
{
    return aob_check_args(g_aob_err, aligned, bytes, bytes_cap, titles, n, format, results,
                          n_sectors);
}

// sample offsets for `format`, each title on a 16-byte boundary
uint64_t lay_out(atg_aob_result *results, uint32_t n, int format)
{
    const uint64_t group = format == ATG_PCM_S16 ? 8 : 4;
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        results[i].sample_offset = pos;
        pos += (results[i].good_frames * results[i].channels + group - 1) / group * group;
    }
    return pos;
}

// the sector and layout passes on a held context.  Records ev[0..2].
atg_status scan_locked(AobCtx &c, const void *d_bytes, const atg_aob_title *titles, uint32_t n,
                       uint64_t n_sectors, int format, atg_aob_result *results,
                       uint64_t *total_samples, hipStream_t s)
{
    ATG_HIP_TRY(g_aob_err, ensure_events(c.ev), "hipEventCreate(&e)");
    std::vector<AobTitle> tab(n);
    uint32_t sec0 = 0;
    for (uint32_t i = 0; i < n; ++i) {
        tab[i] = {titles[i].byte_offset, titles[i].n_sectors, sec0};
        sec0 += titles[i].n_sectors;
    }
    AHIP(c.titles.ensure(sizeof(AobTitle) * n));
    AHIP(c.sectors.ensure(sizeof(atg_aob_sector) * n_sectors));
    AHIP(c.prefix.ensure(sizeof(AobPrefix) * n_sectors));
    AHIP(c.results.ensure(sizeof(atg_aob_result) * n));
    AHIP(hipMemcpyAsync(c.titles.p, tab.data(), sizeof(AobTitle) * n, hipMemcpyHostToDevice, s));
    AHIP(hipEventRecord(c.ev[0], s));
    if (n_sectors) {
        const uint32_t blocks = (uint32_t)std::min<uint64_t>(
            (n_sectors + kAobBlock - 1) / kAobBlock, kMaxBlocks);
        hipLaunchKernelGGL(k_aob_sectors, dim3(blocks), dim3(kAobBlock), 0, s,
                           (const uint8_t *)d_bytes, (const AobTitle *)c.titles.p, n,
                           (uint32_t)n_sectors, (atg_aob_sector *)c.sectors.p);
        AHIP(hipGetLastError());
    }
    AHIP(hipEventRecord(c.ev[1], s));
    hipLaunchKernelGGL(k_aob_layout, dim3(n), dim3(kAobBlock), 0, s, (const AobTitle *)c.titles.p,
                       (const atg_aob_sector *)c.sectors.p, (AobPrefix *)c.prefix.p,
                       (atg_aob_result *)c.results.p);
    AHIP(hipGetLastError());
    AHIP(hipEventRecord(c.ev[2], s));
    AHIP(hipMemcpyAsync(results, c.results.p, sizeof(atg_aob_result) * n, hipMemcpyDeviceToHost,
                        s));
    AHIP(hipStreamSynchronize(s));
    const uint64_t total = lay_out(results, n, format);
    if (total_samples)
        *total_samples = total;
    return ATG_OK;
}

void take_times(AobCtx &c, int stages)
{
    for (int k = 0; k < stages; ++k)
        if (hipEventElapsedTime(&g_aob_times.ms[k], c.ev[k], c.ev[k + 1]) != hipSuccess)
            g_aob_times.ms[k] = 0.f;
    g_aob_times.n = stages;
}

} // namespace

extern "C" {

const char *atg_aob_last_error(void) { return g_aob_err.msg.c_str(); }

uint32_t atg_aob_tile_frames(void) { return 2 * kAobTileChunks; }

int atg_aob_kernel_times(const char **names, float *ms, int cap)
{
    return copy_times(kStageNames, g_aob_times.ms, g_aob_times.n, names, ms, cap);
}

atg_status atg_aob_scan_device(const void *d_bytes, uint64_t bytes_cap,
                               const atg_aob_title *titles, uint32_t n_titles,
                               atg_pcm_format format, atg_aob_result *results,
                               uint64_t *total_samples, atg_aob_sector *sectors,
                               uint64_t sectors_cap, void *stream)
{
    uint64_t n_sectors = 0;
    atg_status st =
        check_args(true, d_bytes, bytes_cap, titles, n_titles, (int)format, results, &n_sectors);
    if (st != ATG_OK)
        return st;
    if (sectors && sectors_cap < n_sectors)
        return g_aob_err.fail(ATG_ERR_CAPACITY, "sectors_cap is below the batch's sector count");
    if (total_samples)
        *total_samples = 0;
    if (!n_titles)
        return ATG_OK;
    DeviceContexts<AobCtx>::Held c;
    if ((st = g_ctxs.hold(d_bytes, g_aob_err, c)) != ATG_OK)
        return st;
    hipStream_t s = (hipStream_t)stream;
    st = scan_locked(*c, d_bytes, titles, n_titles, n_sectors, (int)format, results,
                     total_samples, s);
    if (st != ATG_OK)
        return st;
    take_times(*c, 2);
    if (sectors && n_sectors)
        AHIP(hipMemcpy(sectors, c->sectors.p, sizeof(atg_aob_sector) * n_sectors,
                       hipMemcpyDeviceToHost));
    return ATG_OK;
}

atg_status atg_aob_decode_device(const void *d_bytes, uint64_t bytes_cap,
                                 const atg_aob_title *titles, uint32_t n_titles, void *d_pcm,
                                 atg_pcm_format format, uint64_t pcm_cap_samples,
                                 atg_aob_result *results, void *stream)
{
    uint64_t n_sectors = 0;
    atg_status st =
        check_args(true, d_bytes, bytes_cap, titles, n_titles, (int)format, results, &n_sectors);
    if (st != ATG_OK)
        return st;
    if (n_titles && pcm_cap_samples && !d_pcm)
        return g_aob_err.fail(ATG_ERR_INVALID, "NULL argument");
    if ((uintptr_t)d_pcm & 15u)
        return g_aob_err.fail(ATG_ERR_INVALID, "d_pcm must be 16-byte aligned");
    if (!n_titles)
        return ATG_OK;
    DeviceContexts<AobCtx>::Held c;
    if ((st = g_ctxs.hold(d_bytes, g_aob_err, c)) != ATG_OK)
        return st;
    hipStream_t s = (hipStream_t)stream;
    uint64_t total = 0;
    st = scan_locked(*c, d_bytes, titles, n_titles, n_sectors, (int)format, results, &total, s);
    if (st != ATG_OK)
        return st;
    take_times(*c, 2);
    if (total > pcm_cap_samples)
        return g_aob_err.fail(ATG_ERR_CAPACITY, "pcm_cap_samples is below the batch's samples");
    std::vector<AobRun> runs;
    uint64_t n_tiles = 0;
    uint32_t sec0 = 0;
    for (uint32_t i = 0; i < n_titles; ++i) {
        const atg_aob_result &r = results[i];
        if (r.good_frames) {
            if (format == ATG_PCM_S16 && r.bits_per_sample != 16)
                return g_aob_err.fail(ATG_ERR_INVALID,
                                      "ATG_PCM_S16 cannot hold a 24-bit title");
            const uint64_t chunks = r.good_frames / 2;
            runs.push_back({titles[i].byte_offset, r.sample_offset, chunks, n_tiles, sec0,
                            r.stop_sector, r.channels, r.bits_per_sample / 8});
            n_tiles += (chunks + kAobTileChunks - 1) / kAobTileChunks;
        }
        sec0 += titles[i].n_sectors;
    }
    if (!runs.empty()) {
        AHIP(c->runs.ensure(sizeof(AobRun) * runs.size()));
        AHIP(hipMemcpyAsync(c->runs.p, runs.data(), sizeof(AobRun) * runs.size(),
                            hipMemcpyHostToDevice, s));
    }
    AHIP(hipEventRecord(c->ev[2], s));
    if (!runs.empty()) {
        const dim3 grid((uint32_t)std::min<uint64_t>(n_tiles, kMaxBlocks)), block(kAobBlock);
        if (format == ATG_PCM_S16)
            hipLaunchKernelGGL(k_aob_pcm<int16_t>, grid, block, 0, s, (const uint8_t *)d_bytes,
                               (const atg_aob_sector *)c->sectors.p,
                               (const AobPrefix *)c->prefix.p, (const AobRun *)c->runs.p,
                               (uint32_t)runs.size(), n_tiles, (int16_t *)d_pcm);
        else
            hipLaunchKernelGGL(k_aob_pcm<int32_t>, grid, block, 0, s, (const uint8_t *)d_bytes,
                               (const atg_aob_sector *)c->sectors.p,
                               (const AobPrefix *)c->prefix.p, (const AobRun *)c->runs.p,
                               (uint32_t)runs.size(), n_tiles, (int32_t *)d_pcm);
        AHIP(hipGetLastError());
    }
    AHIP(hipEventRecord(c->ev[3], s));
    AHIP(hipStreamSynchronize(s));
    if (hipEventElapsedTime(&g_aob_times.ms[2], c->ev[2], c->ev[3]) != hipSuccess)
        g_aob_times.ms[2] = 0.f;
    g_aob_times.n = 3;
    return ATG_OK;
}

atg_status atg_aob_decode_host(int device, const void *bytes, uint64_t n_bytes,
                               const atg_aob_title *titles, uint32_t n_titles, void *pcm,
                               atg_pcm_format format, uint64_t pcm_cap_samples,
                               atg_aob_result *results)
{
    uint64_t n_sectors = 0;
    atg_status st =
        check_args(false, bytes, n_bytes, titles, n_titles, (int)format, results, &n_sectors);
    if (st != ATG_OK)
        return st;
    if (n_titles && pcm_cap_samples && !pcm)
        return g_aob_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (!n_titles)
        return ATG_OK;
    if ((st = use_device(device, g_aob_err)) != ATG_OK)
        return st;
    const uint64_t ssize = format == ATG_PCM_S16 ? 2 : 4;
    DevTemp d_bytes, d_pcm;
    ATG_HIP_TRY(g_aob_err, d_bytes.alloc(std::max<uint64_t>(n_bytes, 16)),
                "hipMalloc(&d_bytes, std::max<uint64_t>(n_bytes, 16))");
    hipError_t e = d_pcm.alloc(std::max<uint64_t>(pcm_cap_samples * ssize, 16));
    if (e == hipSuccess)
        e = hipMemcpy(d_bytes.p, bytes, n_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        st = atg_aob_decode_device(d_bytes.p, n_bytes, titles, n_titles, d_pcm.p, format,
                                   pcm_cap_samples, results, nullptr);
        // only the titles' own sample ranges are written
        for (uint32_t i = 0; st == ATG_OK && e == hipSuccess && i < n_titles; ++i) {
            const uint64_t n = results[i].good_frames * results[i].channels;
            if (n)
                e = hipMemcpy((char *)pcm + results[i].sample_offset * ssize,
                              (const char *)d_pcm.p + results[i].sample_offset * ssize,
                              n * ssize, hipMemcpyDeviceToHost);
        }
    }
    if (e != hipSuccess)
        return g_aob_err.fail(ATG_ERR_DEVICE, std::string("staging: ") + hipGetErrorString(e));
    return st;
}

} // extern "C"
