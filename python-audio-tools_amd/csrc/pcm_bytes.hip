// pcm_bytes.hip — packed PCM bytes <-> interleaved integer PCM on the device,
// for every layout the reference's FrameList(bytes, ...) / to_bytes knows:
// 1, 2 or 3 bytes per sample, little or big endian, signed or unsigned.
// It takes the host unpack (numpy, one FrameList at a time) and the int32
// upload of 1- to 3-byte samples out of the path of 24-bit, 8-bit and
// big-endian input: AIFF, Sun AU and 24-bit WAVE go up as they are on disk.
//
// The work is a table of runs {byte_offset, samples, sample_offset}; one
// launch does a batch of tracks.  A run is cut into tiles of kPbTile
// samples, workgroups walk the launch's tiles grid-stride and find a tile's
// run by binary search over the runs' first tile numbers, so one long track
// fills the machine as a thousand short ones do.
//
// Unpack: a lane makes one 16-byte store (4 int32 or 8 int16) from 4 to 16
// packed bytes at any byte address: aligned dword loads, funnelled down by
// the address's low two bits, then each sample cut out at a compile-time
// position.  The kernels are templated on the layout, so the per-sample
// code has no branch.  A run's last samples % N go one at a time.
// Pack: a lane writes one aligned 16-byte unit of the packed image from the
// 6 to 16 samples that touch it; the bytes of a run before its first and
// after its last whole unit are written singly by the run's first tile.
//
// The bodies and the index arithmetic are in pcm_bytes.h with the memory
// contract; tools/pcm_bytes_check.cpp runs them on the CPU under the host
// sanitizers.  Streaming, no reuse: the roofline is HBM bandwidth over
// packed + integer bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/atgpu.h"
#include "host_common.h"
#include "pcm_bytes.h"
#include "pcm_files.h"

namespace {

thread_local ErrSlot g_pb_err;

constexpr uint32_t kMaxBlocks = 4096;

thread_local StageTimes<1> g_pb_times; // one entry, named after the last call
thread_local const char *g_pb_name = nullptr;

DeviceContexts<TableCtx> g_ctxs; // per device: the run table

template <int B, bool BE, bool SGN, typename T>
__global__ __launch_bounds__(kPbBlock) void k_pcm_unpack(const uint8_t *__restrict__ bytes,
                                                         T *__restrict__ pcm,
                                                         const PbRun *__restrict__ runs,
                                                         uint32_t n, uint64_t n_tiles)
{
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const PbRun r = runs[pb_run_of_tile(runs, n, tile)];
        pb_unpack_lane<B, BE, SGN, T>(bytes, pcm, r, tile - r.tile0, threadIdx.x, kPbBlock);
    }
}

template <int B, bool BE, bool SGN, typename T>
__global__ __launch_bounds__(kPbBlock) void k_pcm_pack(const T *__restrict__ pcm,
                                                       uint8_t *__restrict__ bytes,
                                                       const PbRun *__restrict__ runs, uint32_t n,
                                                       uint64_t n_tiles)
{
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const PbRun r = runs[pb_run_of_tile(runs, n, tile)];
        pb_pack_lane<B, BE, SGN, T>(pcm, bytes, r, tile - r.tile0, threadIdx.x, kPbBlock);
    }
}

struct Launch {
    bool pack;
    const void *src;
    void *dst;
    const PbRun *runs;
    uint32_t n;
    uint64_t n_tiles;
    hipStream_t s;
};

template <int B, bool BE, bool SGN, typename T> void launch_one(const Launch &l)
{
    const dim3 grid((uint32_t)std::min<uint64_t>(l.n_tiles, kMaxBlocks)), block(kPbBlock);
    if (l.pack)
        hipLaunchKernelGGL((k_pcm_pack<B, BE, SGN, T>), grid, block, 0, l.s, (const T *)l.src,
                           (uint8_t *)l.dst, l.runs, l.n, l.n_tiles);
    else
        hipLaunchKernelGGL((k_pcm_unpack<B, BE, SGN, T>), grid, block, 0, l.s,
                           (const uint8_t *)l.src, (T *)l.dst, l.runs, l.n, l.n_tiles);
}

template <int B, typename T> void launch_layout(const Launch &l, bool be, bool sgn)
{
    if (B == 1) // one byte has no order
        return sgn ? launch_one<B, false, true, T>(l) : launch_one<B, false, false, T>(l);
    if (be)
        return sgn ? launch_one<B, true, true, T>(l) : launch_one<B, true, false, T>(l);
    return sgn ? launch_one<B, false, true, T>(l) : launch_one<B, false, false, T>(l);
}

void launch(const Launch &l, atg_pcm_layout lay, atg_pcm_format format)
{
    const bool be = lay.big_endian != 0, sgn = lay.is_signed != 0;
    if (format == ATG_PCM_S16) {
        if (lay.bytes_per_sample == 1)
            launch_layout<1, int16_t>(l, be, sgn);
        else
            launch_layout<2, int16_t>(l, be, sgn);
    } else if (lay.bytes_per_sample == 1) {
        launch_layout<1, int32_t>(l, be, sgn);
    } else if (lay.bytes_per_sample == 2) {
        launch_layout<2, int32_t>(l, be, sgn);
    } else {
        launch_layout<3, int32_t>(l, be, sgn);
    }
}

uint64_t pack_tiles(uint32_t B, const PbRun &r)
{
    return B == 1 ? pb_pack_tiles<1>(r) : B == 2 ? pb_pack_tiles<2>(r) : pb_pack_tiles<3>(r);
}

// every check that needs no GPU.  aligned == true: the device entries'
// alignment rules; the host entries stage into buffers that hold them.
atg_status check_args(bool pack, bool aligned, const void *bytes, uint64_t bytes_cap,
                      atg_pcm_layout lay, const atg_pcm_run *runs, uint32_t n, const void *pcm,
                      int format, uint64_t pcm_cap)
{
    if (n && (!bytes || !runs || !pcm))
        return g_pb_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (format != ATG_PCM_S16 && format != ATG_PCM_S32)
        return g_pb_err.fail(ATG_ERR_INVALID, "unknown PCM format");
    if (lay.bytes_per_sample < 1 || lay.bytes_per_sample > 3)
        return g_pb_err.fail(ATG_ERR_INVALID, "bytes_per_sample must be 1, 2 or 3");
    if (format == ATG_PCM_S16 && lay.bytes_per_sample == 3)
        return g_pb_err.fail(ATG_ERR_INVALID, "ATG_PCM_S16 cannot hold 3 bytes per sample");
    const uint64_t ssize = format == ATG_PCM_S16 ? 2 : 4, group = 16 / ssize;
    if (aligned && n) {
        if ((uintptr_t)bytes & 15u)
            return g_pb_err.fail(ATG_ERR_INVALID, "the packed buffer must be 16-byte aligned");
        if (!pack && (bytes_cap & 15u))
            return g_pb_err.fail(ATG_ERR_INVALID, "bytes_cap must be a multiple of 16");
        if ((uintptr_t)pcm & (pack ? ssize - 1 : 15u))
            return g_pb_err.fail(ATG_ERR_INVALID, pack ? "d_pcm is not aligned to its samples"
                                                       : "d_pcm must be 16-byte aligned");
    }
    if (!pack)
        for (uint32_t i = 0; i < n; ++i)
            if (runs[i].samples && runs[i].sample_offset % group)
                return g_pb_err.fail(ATG_ERR_INVALID,
                                     "sample_offset must put the run on a 16-byte boundary");
    const uint64_t B = lay.bytes_per_sample;
    for (uint32_t i = 0; i < n; ++i) {
        const atg_pcm_run &r = runs[i];
        if (r.byte_offset > bytes_cap || r.samples > (bytes_cap - r.byte_offset) / B)
            return g_pb_err.fail(ATG_ERR_CAPACITY, "a run's packed range passes bytes_cap");
        if (r.sample_offset > pcm_cap || r.samples > pcm_cap - r.sample_offset)
            return g_pb_err.fail(ATG_ERR_CAPACITY, "a run's sample range passes pcm_cap_samples");
    }
    return ATG_OK;
}

atg_status run_device(bool pack, const void *d_bytes, uint64_t bytes_cap, atg_pcm_layout lay,
                      const atg_pcm_run *runs, uint32_t n, const void *d_pcm, int format,
                      uint64_t pcm_cap, void *stream)
{
    atg_status st = check_args(pack, true, d_bytes, bytes_cap, lay, runs, n, d_pcm, format, pcm_cap);
    if (st != ATG_OK)
        return st;
    std::vector<PbRun> tab;
    tab.reserve(n);
    uint64_t n_tiles = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!runs[i].samples)
            continue;
        PbRun r = {runs[i].byte_offset, runs[i].samples, runs[i].sample_offset, n_tiles};
        n_tiles += pack ? pack_tiles(lay.bytes_per_sample, r) : pb_unpack_tiles(r.samples);
        tab.push_back(r);
    }
    if (tab.empty())
        return ATG_OK;
    hipStream_t s = (hipStream_t)stream;
    DeviceContexts<TableCtx>::Held held;
    if ((st = g_ctxs.hold(d_pcm, g_pb_err, held)) != ATG_OK)
        return st;
    float ms = 0.f;
    st = timed_launch(held->table, held->ev, tab, s, g_pb_err, &ms, [&](const PbRun *d_runs) {
        const Launch l = {pack,
                          pack ? d_pcm : d_bytes,
                          const_cast<void *>(pack ? d_bytes : d_pcm),
                          d_runs,
                          (uint32_t)tab.size(),
                          n_tiles,
                          s};
        launch(l, lay, (atg_pcm_format)format);
    });
    if (st == ATG_OK && ms >= 0.f) {
        g_pb_times = {{ms}, 1};
        g_pb_name = pack ? "pack" : "unpack";
    }
    return st;
}

// the ranges [first, second) the runs cover on one side, merged where they
// touch; unit = bytes per element
std::vector<std::pair<uint64_t, uint64_t>> covered(const atg_pcm_run *runs, uint32_t n, bool packed,
                                                   uint64_t unit)
{
    std::vector<std::pair<uint64_t, uint64_t>> v;
    for (uint32_t i = 0; i < n; ++i)
        if (runs[i].samples) {
            const uint64_t a = packed ? runs[i].byte_offset : runs[i].sample_offset * unit;
            v.emplace_back(a, a + runs[i].samples * unit);
        }
    std::sort(v.begin(), v.end());
    std::vector<std::pair<uint64_t, uint64_t>> out;
    for (const auto &r : v) {
        if (!out.empty() && r.first <= out.back().second)
            out.back().second = std::max(out.back().second, r.second);
        else
            out.push_back(r);
    }
    return out;
}

atg_status run_host(bool pack, int device, const void *bytes, uint64_t n_bytes, atg_pcm_layout lay,
                    const atg_pcm_run *runs, uint32_t n, const void *pcm, int format,
                    uint64_t pcm_cap)
{
    atg_status st = check_args(pack, false, bytes, n_bytes, lay, runs, n, pcm, format, pcm_cap);
    if (st != ATG_OK)
        return st;
    bool any = false;
    for (uint32_t i = 0; i < n; ++i)
        any = any || runs[i].samples;
    if (!any)
        return ATG_OK;
    if ((st = use_device(device, g_pb_err)) != ATG_OK)
        return st;
    const uint64_t ssize = format == ATG_PCM_S16 ? 2 : 4;
    const uint64_t cap16 = (n_bytes + 15) & ~(uint64_t)15;
    DevTemp d_bytes, d_pcm;
    ATG_HIP_TRY(g_pb_err, d_bytes.alloc(std::max<uint64_t>(cap16, 16)),
                "hipMalloc(&d_bytes, std::max<uint64_t>(cap16, 16))");
    hipError_t e = d_pcm.alloc(std::max<uint64_t>(pcm_cap * ssize, 16));
    // in: the runs' ranges of the source side; out: those of the other side
    const void *src = pack ? pcm : bytes;
    void *d_src = pack ? d_pcm.p : d_bytes.p, *d_dst = pack ? d_bytes.p : d_pcm.p;
    void *dst = const_cast<void *>(pack ? bytes : pcm);
    if (e == hipSuccess)
        for (const auto &r : covered(runs, n, !pack, pack ? ssize : lay.bytes_per_sample))
            if (e == hipSuccess)
                e = hipMemcpy((char *)d_src + r.first, (const char *)src + r.first,
                              r.second - r.first, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        st = pack ? atg_pcm_pack_device(d_pcm.p, (atg_pcm_format)format, pcm_cap, lay, runs, n,
                                        d_bytes.p, cap16, nullptr)
                  : atg_pcm_unpack_device(d_bytes.p, cap16, lay, runs, n, d_pcm.p,
                                          (atg_pcm_format)format, pcm_cap, nullptr);
        if (st == ATG_OK)
            for (const auto &r : covered(runs, n, pack, pack ? lay.bytes_per_sample : ssize))
                if (e == hipSuccess)
                    e = hipMemcpy((char *)dst + r.first, (const char *)d_dst + r.first,
                                  r.second - r.first, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess)
        return g_pb_err.fail(ATG_ERR_DEVICE, std::string("staging: ") + hipGetErrorString(e));
    return st;
}

} // namespace

extern "C" {

const char *atg_pcm_bytes_last_error(void) { return g_pb_err.msg.c_str(); }

uint32_t atg_pcm_bytes_tile_samples(void) { return kPbTile; }

int atg_pcm_bytes_kernel_times(const char **names, float *ms, int cap)
{
    return copy_times(&g_pb_name, g_pb_times.ms, g_pb_times.n, names, ms, cap);
}

atg_status atg_pcm_unpack_device(const void *d_bytes, uint64_t bytes_cap, atg_pcm_layout layout,
                                 const atg_pcm_run *runs, uint32_t n_runs, void *d_pcm,
                                 atg_pcm_format format, uint64_t pcm_cap_samples, void *stream)
{
    return run_device(false, d_bytes, bytes_cap, layout, runs, n_runs, d_pcm, (int)format,
                      pcm_cap_samples, stream);
}

atg_status atg_pcm_pack_device(const void *d_pcm, atg_pcm_format format, uint64_t pcm_cap_samples,
                               atg_pcm_layout layout, const atg_pcm_run *runs, uint32_t n_runs,
                               void *d_bytes, uint64_t bytes_cap, void *stream)
{
    return run_device(true, d_bytes, bytes_cap, layout, runs, n_runs, d_pcm, (int)format,
                      pcm_cap_samples, stream);
}

atg_status atg_pcm_unpack_host(int device, const void *bytes, uint64_t n_bytes,
                               atg_pcm_layout layout, const atg_pcm_run *runs, uint32_t n_runs,
                               void *pcm, atg_pcm_format format, uint64_t pcm_cap_samples)
{
    return run_host(false, device, bytes, n_bytes, layout, runs, n_runs, pcm, (int)format,
                    pcm_cap_samples);
}

atg_status atg_pcm_pack_host(int device, const void *pcm, atg_pcm_format format,
                             uint64_t pcm_cap_samples, atg_pcm_layout layout,
                             const atg_pcm_run *runs, uint32_t n_runs, void *bytes,
                             uint64_t n_bytes)
{
    return run_host(true, device, bytes, n_bytes, layout, runs, n_runs, pcm, (int)format,
                    pcm_cap_samples);
}

int atg_aiff_read_info(const uint8_t *data, uint64_t len, atg_aiff_info *info)
{
    return atg_aiff_parse(data, len, info);
}

int atg_au_read_info(const uint8_t *data, uint64_t len, atg_au_info *info)
{
    return atg_au_parse(data, len, info);
}

} // extern "C"
