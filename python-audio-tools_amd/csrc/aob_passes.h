// aob_passes.h — the two passes every DVD-Audio codec starts with, shared by
// aob_decode.hip (packed PCM) and mlp_decode.hip (MLP): the sector pass and
// the per-title layout (first bad sector, 64-bit prefix sum of the payload
// lengths before it).  Device code; each translation unit gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include "aob_common.h"
#include "host_common.h"
#include "table_search.h"
#include "wave.h"

namespace {

// a title on the device: its sectors are rows [sec0, sec0 + n_sectors) of
// the sector and prefix tables
struct AobTitle {
    uint64_t byte_offset;
    uint32_t n_sectors;
    uint32_t sec0;
};

struct AobPrefix {
    uint64_t start; // payload bytes of the title before this sector
};

__global__ __launch_bounds__(kAobBlock) void k_aob_sectors(const uint8_t *__restrict__ bytes,
                                                           const AobTitle *__restrict__ titles,
                                                           uint32_t n_titles, uint32_t n_sectors,
                                                           atg_aob_sector *__restrict__ sectors)
{
    for (uint32_t g = blockIdx.x * kAobBlock + threadIdx.x; g < n_sectors;
         g += gridDim.x * kAobBlock) {
        const AobTitle t = titles[last_le(titles, n_titles, g, &AobTitle::sec0)];
        const atg_aob_sector r =
            aob_walk_sector(bytes + t.byte_offset + (uint64_t)(g - t.sec0) * kAobSector);
        static_assert(sizeof(atg_aob_sector) == 16, "one 16-byte store per record");
        *reinterpret_cast<uint4 *>(sectors + g) = *reinterpret_cast<const uint4 *>(&r);
    }
}

// One workgroup of kAobBlock threads per title: writes the prefix rows of the
// sectors before the first bad one and gives every thread that sector's
// index (n_sectors when none is bad) and the payload bytes before it.
__device__ __forceinline__ void aob_layout_title(const AobTitle &t,
                                                 const atg_aob_sector *__restrict__ sec,
                                                 AobPrefix *__restrict__ pre, uint32_t *first_bad,
                                                 uint64_t *payload_bytes)
{
    constexpr uint32_t kWaves = kAobBlock / 64;
    __shared__ uint32_t s_bad[kWaves];
    __shared__ uint64_t s_sum[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;

    // a lane's sectors ascend, so its first bad one is its lowest
    uint32_t bad = t.n_sectors;
    for (uint32_t i = tid; i < t.n_sectors; i += kAobBlock)
        if (sec[i].status) {
            bad = i;
            break;
        }
    bad = wave_min_u32(bad);
    if (lane == 0)
        s_bad[wave] = bad;
    __syncthreads();
    bad = s_bad[0];
    for (uint32_t w = 1; w < kWaves; ++w)
        bad = min(bad, s_bad[w]);

    uint64_t carry = 0;
    for (uint32_t base = 0; base < bad; base += kAobBlock) {
        const uint32_t i = base + tid;
        const uint64_t v = i < bad ? sec[i].payload_length : 0;
        const uint64_t incl = wave_incl_scan_u64(v, (int)lane);
        __syncthreads(); // the previous round's s_sum has been read
        if (lane == 63)
            s_sum[wave] = incl;
        __syncthreads();
        uint64_t before = 0, total = 0;
        for (uint32_t w = 0; w < kWaves; ++w) {
            before += w < wave ? s_sum[w] : 0;
            total += s_sum[w];
        }
        if (i < bad)
            pre[i].start = carry + before + incl - v;
        carry += total;
    }
    *first_bad = bad;
    *payload_bytes = carry;
}

// every check that needs no GPU.  aligned == true: the device entries'
// alignment rules; the host entry stages into buffers that hold them.
inline atg_status aob_check_args(ErrSlot &err, bool aligned, const void *bytes, uint64_t bytes_cap,
                                 const atg_aob_title *titles, uint32_t n, int format,
                                 const void *results, uint64_t *n_sectors)
{
    if (n && (!bytes || !titles || !results))
        return err.fail(ATG_ERR_INVALID, "NULL argument");
    if (format != ATG_PCM_S16 && format != ATG_PCM_S32)
        return err.fail(ATG_ERR_INVALID, "unknown PCM format");
    if (aligned && n && ((uintptr_t)bytes & 15u))
        return err.fail(ATG_ERR_INVALID, "the AOB buffer must be 16-byte aligned");
    if (n > ATG_AOB_MAX_TITLES)
        return err.fail(ATG_ERR_UNSUPPORTED, "more than ATG_AOB_MAX_TITLES titles");
    if (bytes_cap > ATG_AOB_MAX_BATCH_BYTES)
        return err.fail(ATG_ERR_UNSUPPORTED, "more than ATG_AOB_MAX_BATCH_BYTES bytes");
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const atg_aob_title &t = titles[i];
        if (t.byte_offset & 15u)
            return err.fail(ATG_ERR_INVALID, "byte_offset must be a multiple of 16");
        if (t.n_sectors > ATG_AOB_MAX_TITLE_SECTORS)
            return err.fail(ATG_ERR_UNSUPPORTED,
                                  "a title of more than ATG_AOB_MAX_TITLE_SECTORS sectors");
        if (t.byte_offset > bytes_cap ||
            t.n_sectors > (bytes_cap - t.byte_offset) / ATG_AOB_SECTOR_BYTES)
            return err.fail(ATG_ERR_CAPACITY, "a title's sectors pass bytes_cap");
        total += t.n_sectors;
    }
    if (total > 0x7FFFFFFFull)
        return err.fail(ATG_ERR_UNSUPPORTED, "more than 2^31 - 1 sectors in one batch");
    *n_sectors = total;
    return ATG_OK;
}

} // namespace
