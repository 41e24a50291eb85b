// dither.hip — the dither bits of a batch conversion, made in device memory:
// one launch fills a ragged table of runs with the bytes of a counter-based
// generator, so pcm_chain.hip reads its dither buffer as it always did and no
// random byte is drawn or uploaded on the host.
//
// The source (include/atgpu_dither.h) is Philox4x32-10.  A block is the 16
// bytes of one counter value: counter = (block index, stream), key = seed.
// Any block stands alone, so a run may start at any block of any stream.
//
// Tiles.  A run is cut into tiles of kTileBlocks blocks.  The call's tiles
// form one list, a workgroup takes one, and its run is a binary search over
// the runs' first tiles (table_search.h).  A lane makes kPer whole blocks,
// kBlock blocks apart, and writes each with one 16-byte store: a wave's store
// covers 1 KiB without a gap, and the kPer Philox chains of a lane are
// independent, so their multiplies overlap.
//
// Cost.  A block is 10 rounds of two 32 x 32 -> 64-bit products and four
// XORs, and two key additions per round: 20 products per 16 bytes.  The
// products are the only instructions that do not run at the full VALU rate;
// profiles/dither_bench.json holds the fill's rate beside a memset's.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/atgpu.h"
#include "host_common.h"
#include "pcm_rows.h"
#include "table_search.h"

namespace {

thread_local ErrSlot g_di_err;

constexpr uint32_t kBlock = 256;
constexpr uint32_t kPer = 4;                     // blocks of a lane
constexpr uint32_t kTileBlocks = kBlock * kPer;  // 16 KiB of a workgroup

const char *const kStageNames[1] = {"fill"};
thread_local StageTimes<1> g_di_times;

struct DitherRow {
    uint64_t stream;
    uint64_t block0; // the run's first block of the stream
    uint64_t blocks;
    uint64_t unit0;  // the run's first 16-byte unit of the output
    uint64_t tile0;  // the run's first tile in the call's list
};

DeviceContexts<TableCtx> g_ctxs;

constexpr uint32_t kMul0 = 0xD2511F53u, kMul1 = 0xCD9E8D57u;
constexpr uint32_t kKey0 = 0x9E3779B9u, kKey1 = 0xBB67AE85u;

// Philox4x32-10 of counter (c0, c1, c2, c3) under key (k0, k1)
__device__ __forceinline__ Unit philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                       uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)kMul0 * c0, p1 = (uint64_t)kMul1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += kKey0;
        k1 += kKey1;
    }
    return Unit{c0, c1, c2, c3};
}

__global__ __launch_bounds__(kBlock) void k_dither_fill(const DitherRow *__restrict__ rows,
                                                        uint32_t n, uint32_t key0, uint32_t key1,
                                                        Unit *__restrict__ out)
{
    const uint64_t tile = blockIdx.x;
    const uint32_t i = last_le(rows, n, tile, &DitherRow::tile0);
    const DitherRow R = rows[i];
    const uint64_t base = (tile - R.tile0) * kTileBlocks;
    const uint32_t s0 = (uint32_t)R.stream, s1 = (uint32_t)(R.stream >> 32);
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r) {
        const uint64_t b = base + r * kBlock + threadIdx.x; // block of the run
        if (b < R.blocks) {
            const uint64_t ctr = R.block0 + b;
            out[R.unit0 + b] = philox((uint32_t)ctr, (uint32_t)(ctr >> 32), s0, s1, key0, key1);
        }
    }
}

// ---------------------------------------------------------------- host side

std::string at_run(uint32_t i, const char *what)
{
    return "run " + std::to_string(i) + ": " + what;
}

// every refusal, before any GPU call
atg_status check_args(const atg_dither_run *runs, uint32_t n, const void *d_out, uint64_t out_cap)
{
    if (n && !runs)
        return g_di_err.fail(ATG_ERR_INVALID, "runs is NULL");
    if ((uintptr_t)d_out & 15)
        return g_di_err.fail(ATG_ERR_INVALID, "d_out is not 16-byte aligned");
    bool any = false;
    std::vector<std::pair<uint64_t, uint64_t>> ranges; // output [start, end) in bytes
    for (uint32_t i = 0; i < n; ++i) {
        const atg_dither_run &r = runs[i];
        if (r.byte_offset & 15)
            return g_di_err.fail(ATG_ERR_INVALID,
                                 at_run(i, "byte_offset is not on a 16-byte boundary"));
        if (!r.blocks)
            continue;
        any = true;
        if (r.first_block > UINT64_MAX - (r.blocks - 1))
            return g_di_err.fail(ATG_ERR_INVALID, at_run(i, "first_block + blocks passes 2^64"));
        if (r.byte_offset > out_cap || r.blocks > (out_cap - r.byte_offset) / 16)
            return g_di_err.fail(ATG_ERR_CAPACITY, at_run(i, "output range passes out_cap"));
        ranges.push_back({r.byte_offset, r.byte_offset + 16 * r.blocks});
    }
    if (any && !d_out)
        return g_di_err.fail(ATG_ERR_INVALID, "d_out is NULL");
    if (pcm_ranges_overlap(ranges))
        return g_di_err.fail(ATG_ERR_INVALID, "output runs overlap");
    return ATG_OK;
}

} // namespace

extern "C" {

const char *atg_dither_last_error(void) { return g_di_err.msg.c_str(); }

uint32_t atg_dither_tile_blocks(void) { return kTileBlocks; }

atg_status atg_dither_fill_device(const atg_dither_run *runs, uint32_t n_runs, uint64_t seed,
                                  void *d_out, uint64_t out_cap, void *stream)
{
    atg_status st = check_args(runs, n_runs, d_out, out_cap);
    if (st != ATG_OK)
        return st;
    PcmRowTable<DitherRow> tab;
    for (uint32_t i = 0; i < n_runs; ++i) {
        const atg_dither_run &r = runs[i];
        if (!r.blocks)
            continue;
        const DitherRow row = {r.stream, r.first_block, r.blocks, r.byte_offset / 16, 0};
        // blocks <= out_cap / 16 < 2^60: the sum cannot wrap
        tab.add(row, (r.blocks + kTileBlocks - 1) / kTileBlocks);
    }
    if (tab.rows.empty())
        return ATG_OK;
    if ((st = tab.check(g_di_err)) != ATG_OK)
        return st;
    DeviceContexts<TableCtx>::Held held; // the device that holds the output
    if ((st = g_ctxs.hold(d_out, g_di_err, held)) != ATG_OK)
        return st;
    hipStream_t s = (hipStream_t)stream;
    const auto launch = [&](const DitherRow *d_rows) {
        hipLaunchKernelGGL(k_dither_fill, dim3((uint32_t)tab.tiles), dim3(kBlock), 0, s, d_rows,
                           (uint32_t)tab.rows.size(), (uint32_t)seed, (uint32_t)(seed >> 32),
                           (Unit *)d_out);
    };
    float ms = 0.f;
    st = timed_launch(held->table, held->ev, tab.rows, s, g_di_err, &ms, launch);
    if (st == ATG_OK)
        g_di_times = {{ms}, ms >= 0.f};
    return st;
}

int atg_dither_kernel_times(const char **names, float *ms, int cap)
{
    return copy_times(kStageNames, g_di_times.ms, g_di_times.n, names, ms, cap);
}

} // extern "C"
