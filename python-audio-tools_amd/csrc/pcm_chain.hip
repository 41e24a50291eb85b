// pcm_chain.hip — the PCM converter chain of a batch conversion, one launch
// for a ragged table of tracks.  A row reads a source view (int16 or int32,
// at any sample offset), applies a channel operation and then a
// bits-per-sample operation, and writes its own range of the output (int16
// or int32).  Rows of one call may differ in every parameter.
//
//   MAP              output channel k = input channel map[k], or silence
//                    (ReorderedPCMReader, RemaskedPCMReader, the mono -> N
//                    duplication of PCMConverter)
//   DOWNMIX          k_pcm_downmix of pcm_convert.hip: the 6-slot layout from
//                    the channel mask, fp64 without contraction, round, clamp
//   AVERAGE          int64 sum / channels, C truncation
//   DOWNMIX_AVERAGE  Averager(Downmixer(x)): the downmix's rounding and clamp
//                    come before the average of its two channels
//   bits             up: x << s; down: (x >> s) ^ dither bit, the bits MSB
//                    first from one byte stream, consumed per 4096-frame read
//                    of this stage's input, channel by channel within a read
//                    (bps_one of pcm_convert.hip, per row)
//
// Tiles.  A row is cut into tiles of tile_frames frames, a multiple of 8 with
// tile_frames * max(in, out channels) <= kTile, so a tile's output starts on a
// 16-byte boundary of the row's output and its input fits the LDS.  The
// batch's tiles form one list, a workgroup takes one, and its row is a binary
// search over the rows' first tiles (table_search.h).
//
// Loads (pcm_rows.h, as the store).  The source is addressed in samples from
// its pointer rounded down to 16 bytes.  The workgroup loads the aligned
// 16-byte units that cover the tile's input samples -- each holds a sample of
// the row -- into the LDS as they are, every lane's loads issued before its
// first LDS write.  A lane then picks the samples of its output samples out
// of the LDS by address, so the source's phase within a unit never indexes a
// register, and there is one code path per (input format, output format).
//
// Stores.  A lane converts the 8 (int16) or 4 (int32) output samples of one
// 16-byte non-temporal store, so a wave's store writes 1 KiB without a gap:
// a row's output starts on a 16-byte boundary and a tile on a multiple of 8
// samples.  The last group of a row, when short, goes sample by sample.  The
// rounds of a tile (two for int16 output, four for int32) are unrolled: the
// dither byte loads of all of them are in flight together, where a loop
// serialised them behind the barrier (0.85 -> 0.97 of k_pcm_bps's bytes per
// second on its own shape, profiles/pcm_chain_bench.json).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/atgpu.h"
#include "host_common.h"
#include "pcm_rows.h"
#include "table_search.h"

#pragma clang fp contract(off)

namespace {

thread_local ErrSlot g_ch_err;

constexpr uint32_t kTile = 4096; // samples of a tile, on its wider side
constexpr uint32_t kBlock = 256;
constexpr uint32_t kMaxChannels = 8;
constexpr uint32_t kSilent = 15; // a map nibble
constexpr uint32_t kOpIdentity = 4; // in the device table: a MAP that changes nothing
constexpr uint64_t kLimit = 1ull << 62;

const char *const kStageNames[1] = {"chain"};
thread_local StageTimes<1> g_ch_times;

struct ChainRow {
    PcmSplit src;     // the source: its aligned pointer and first sample
    uint64_t frames;
    uint64_t out0;    // index in the output of the row's first sample
    uint64_t tile0;   // the row's first tile in the batch's list
    uint64_t bit0;    // the row's first dither bit
    uint32_t tile_frames;
    uint32_t mask;    // DOWNMIX: which of the 6 slots the input fills, in order
    uint32_t map;     // MAP: nibble k = input channel of output k, or kSilent
    uint8_t ic, oc, op, fmt;
    uint8_t in_bps, out_bps, pad[2];
};

DeviceContexts<TableCtx> g_ctxs;

constexpr uint32_t kLdsUnits = kTile / 4 + 1; // int32 input at any phase

// sample i of the staged units
template <int FIN> __device__ __forceinline__ int32_t staged(const Unit *lds, uint32_t i)
{
    if (FIN == ATG_PCM_S32)
        return ((const int32_t *)lds)[i];
    return (int32_t)((const int16_t *)lds)[i];
}

// Downmixer_read for one frame whose first sample is staged sample i
template <int FIN>
__device__ __forceinline__ void downmix_frame(const Unit *lds, uint32_t i, uint32_t mask,
                                              uint32_t bps, int32_t *left, int32_t *right)
{
    int32_t six[6];
#pragma unroll
    for (uint32_t m = 0; m < 6; ++m) {
        if (mask & (1u << m))
            six[m] = staged<FIN>(lds, i++);
        else
            six[m] = 0;
    }
    const double REAR_GAIN = 0.6, CENTER_GAIN = 0.7;
    const int32_t smin = -(1 << (bps - 1)), smax = (1 << (bps - 1)) - 1;
    const double mono_rear = 0.7 * (double)(six[4] + six[5]);
    const int32_t l = (int32_t)round((double)six[0] + REAR_GAIN * mono_rear +
                                     CENTER_GAIN * (double)six[2]);
    const int32_t r = (int32_t)round((double)six[1] - REAR_GAIN * mono_rear +
                                     CENTER_GAIN * (double)six[2]);
    *left = l > smax ? smax : (l < smin ? smin : l);
    *right = r > smax ? smax : (r < smin ? smin : r);
}

// Where a tile's dither bits lie.  The tile's first frame is frame fa4 of a
// 4096-frame read of the row; that read has clen0 frames and the next clen1;
// the read's first bit is bit `lead` of bytes[0].
struct DitherTile {
    const uint8_t *bytes;
    uint32_t lead, fa4, clen0, clen1;
    __device__ __forceinline__ DitherTile(const ChainRow &R, uint64_t fa, const uint8_t *dither)
    {
        fa4 = (uint32_t)(fa & 4095u);
        const uint64_t read0 = fa - fa4, left = R.frames - read0;
        clen0 = left < 4096u ? (uint32_t)left : 4096u;
        clen1 = left - clen0 < 4096u ? (uint32_t)(left - clen0) : 4096u;
        const uint64_t b0 = R.bit0 + read0 * R.oc;
        bytes = dither + (b0 >> 3);
        lead = (uint32_t)(b0 & 7u);
    }
};

// One tile: frames [fa, fb) of row R, whose input is staged from staged
// sample `skew` on.
template <int FIN, int FOUT>
__device__ __forceinline__ void convert_tile(const ChainRow &R, uint64_t fa, uint64_t fb,
                                             uint32_t skew, const Unit *lds, void *out,
                                             const uint8_t *__restrict__ dither)
{
    // a lane takes the G output samples of one 16-byte store (pcm_store_group)
    constexpr int G = FOUT == ATG_PCM_S16 ? 8 : 4;
    const uint32_t ic = R.ic, oc = R.oc, nf = (uint32_t)(fb - fa);
    const uint32_t n_out = nf * oc;
    const DitherTile bits(R, fa, dither);
    const uint64_t o0 = R.out0 + fa * oc; // a multiple of 8 past the row's start
    // a fixed number of rounds, unrolled: the rounds' dither loads overlap
#pragma unroll
    for (uint32_t round = 0; round < kTile / (kBlock * G); ++round) {
        const uint32_t q = (round * kBlock + threadIdx.x) * G;
        if (q >= n_out)
            break;
        int32_t x[G];
        // ---- the channel operation
        if (R.op == kOpIdentity) {
            // MAP that changes nothing: the lane's samples lie together
#pragma unroll
            for (int j = 0; j < G; ++j)
                x[j] = q + j < n_out ? staged<FIN>(lds, skew + q + j) : 0;
        } else if (R.op == ATG_CHAIN_MAP) {
            uint32_t f = q / oc, c = q - f * oc;
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const uint32_t m = (R.map >> (4 * c)) & 15u;
                x[j] = (f < nf && m != kSilent) ? staged<FIN>(lds, skew + f * ic + m) : 0;
                if (++c == oc) {
                    c = 0;
                    ++f;
                }
            }
        } else if (R.op == ATG_CHAIN_DOWNMIX) {
#pragma unroll
            for (int j = 0; j < G / 2; ++j) {
                const uint32_t f = q / 2 + j;
                x[2 * j] = x[2 * j + 1] = 0;
                if (f < nf)
                    downmix_frame<FIN>(lds, skew + f * ic, R.mask, R.in_bps, &x[2 * j],
                                       &x[2 * j + 1]);
            }
        } else if (R.op == ATG_CHAIN_AVERAGE) {
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const uint32_t f = q + j;
                int64_t acc = 0;
                if (f < nf)
                    for (uint32_t c = 0; c < ic; ++c)
                        acc += staged<FIN>(lds, skew + f * ic + c);
                x[j] = (int32_t)(acc / (int64_t)ic);
            }
        } else { // ATG_CHAIN_DOWNMIX_AVERAGE
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const uint32_t f = q + j;
                int32_t l = 0, r = 0;
                if (f < nf)
                    downmix_frame<FIN>(lds, skew + f * ic, R.mask, R.in_bps, &l, &r);
                x[j] = (int32_t)(((int64_t)l + (int64_t)r) / 2);
            }
        }
        // ---- the bits-per-sample operation, on frames of oc channels
        if (R.out_bps > R.in_bps) {
#pragma unroll
            for (int j = 0; j < G; ++j)
                x[j] = (int32_t)((uint32_t)x[j] << (R.out_bps - R.in_bps));
        } else if (R.out_bps < R.in_bps) {
            // bps_one's bit index in 32 bits: a tile is at most 4096 frames, so
            // it meets at most two 4096-frame reads, and a sample's bit lies
            // less than 2 * 4096 * 8 bits past the first one's first bit
            const uint32_t s = R.in_bps - R.out_bps;
            uint32_t f = q / oc, c = q - f * oc;
#pragma unroll
            for (int j = 0; j < G; ++j) {
                if (f < nf) {
                    const uint32_t in = bits.fa4 + f; // frame within the first read, or past it
                    const uint32_t rel = in < 4096u ? c * bits.clen0 + in
                                                    : 4096u * oc + c * bits.clen1 + (in - 4096u);
                    const uint32_t t = bits.lead + rel;
                    const int32_t bit = (bits.bytes[t >> 3] >> (7 - (t & 7))) & 1;
                    x[j] = (x[j] >> s) ^ bit;
                }
                if (++c == oc) {
                    c = 0;
                    ++f;
                }
            }
        }
        pcm_store_group<FOUT>(x, out, o0, q, n_out);
    }
}

template <int FIN, int FOUT>
__device__ __forceinline__ void run_tile(const ChainRow &R, uint64_t fa, uint64_t fb, Unit *lds,
                                         void *out, const uint8_t *__restrict__ dither)
{
    constexpr uint32_t kPer = FIN == ATG_PCM_S32 ? 4 : 8;
    const PcmUnits u = pcm_units(R.src.lo, fa, (uint32_t)(fb - fa), R.ic, kPer);
    pcm_load_units<kTile / kPer / kBlock, kBlock>(R.src.p, u.u0, u.nu,
                                                  [lds](Unit v, uint32_t j) { lds[j] = v; });
    __syncthreads();
    convert_tile<FIN, FOUT>(R, fa, fb, u.skew, lds, out, dither);
}

template <int FOUT>
__global__ __launch_bounds__(kBlock) void k_pcm_chain(const ChainRow *__restrict__ rows,
                                                      uint32_t n, void *out,
                                                      const uint8_t *__restrict__ dither)
{
    __shared__ Unit lds[kLdsUnits];
    const uint64_t tile = blockIdx.x;
    const uint32_t i = last_le(rows, n, tile, &ChainRow::tile0);
    const ChainRow R = rows[i];
    const uint64_t fa = (tile - R.tile0) * R.tile_frames;
    const uint64_t fb = fa + R.tile_frames < R.frames ? fa + R.tile_frames : R.frames;
    if (fa >= fb)
        return;
    if (R.fmt == ATG_PCM_S32)
        run_tile<ATG_PCM_S32, FOUT>(R, fa, fb, lds, out, dither);
    else
        run_tile<ATG_PCM_S16, FOUT>(R, fa, fb, lds, out, dither);
}

// ---------------------------------------------------------------- host side

uint32_t default_mask(uint32_t ch)
{
    // Downmixer_read's invented masks (pcmconverter.c:256-290)
    static const uint32_t m[7] = {0x0, 0x4, 0x3, 0x7, 0x33, 0x37, 0x3F};
    return ch <= 6 ? m[ch] : 0x3F;
}

uint32_t tile_frames_of(uint32_t ic, uint32_t oc) { return 8u * (kTile / (8u * std::max(ic, oc))); }

bool reduces(const atg_pcm_chain_row &r) { return r.out_bps < r.in_bps; }

// every refusal, before any GPU call
atg_status check_args(const atg_pcm_chain_row *rows, uint32_t n, const void *d_out,
                      int out_format, uint64_t out_cap_samples, const void *d_dither,
                      uint64_t dither_bytes)
{
    if (n && !rows)
        return g_ch_err.fail(ATG_ERR_INVALID, "rows is NULL");
    if (out_format != ATG_PCM_S16 && out_format != ATG_PCM_S32)
        return g_ch_err.fail(ATG_ERR_INVALID, "unknown output format");
    const uint32_t out_size = out_format == ATG_PCM_S32 ? 4 : 2;
    bool any_out = false, any_dither = false;
    std::vector<std::pair<uint64_t, uint64_t>> ranges; // output [start, end)
    for (uint32_t i = 0; i < n; ++i) {
        const atg_pcm_chain_row &r = rows[i];
        if (r.in_channels < 1 || r.in_channels > kMaxChannels || r.out_channels < 1 ||
            r.out_channels > kMaxChannels)
            return g_ch_err.fail(ATG_ERR_INVALID, at_row(i, "channel count outside 1..8"));
        if (r.in_bps < 1 || r.in_bps > 24 || r.out_bps < 1 || r.out_bps > 24)
            return g_ch_err.fail(ATG_ERR_INVALID, at_row(i, "bits per sample outside 1..24"));
        switch (r.channel_op) {
        case ATG_CHAIN_MAP:
            for (uint32_t k = 0; k < r.out_channels; ++k)
                if (r.map[k] != ATG_CHAIN_SILENT && r.map[k] >= r.in_channels)
                    return g_ch_err.fail(ATG_ERR_INVALID,
                                         at_row(i, "map names an input channel the row lacks"));
            break;
        case ATG_CHAIN_DOWNMIX:
        case ATG_CHAIN_DOWNMIX_AVERAGE: {
            if (r.out_channels != (r.channel_op == ATG_CHAIN_DOWNMIX ? 2u : 1u))
                return g_ch_err.fail(ATG_ERR_INVALID,
                                     at_row(i, "out_channels does not fit the channel operation"));
            const uint32_t mask = r.channel_mask ? r.channel_mask : default_mask(r.in_channels);
            uint32_t bits = 0;
            for (uint32_t m = mask & 0x3F; m; m >>= 1)
                bits += m & 1u;
            if (bits > r.in_channels)
                return g_ch_err.fail(ATG_ERR_INVALID,
                                     at_row(i, "channel mask names more channels than present"));
            break;
        }
        case ATG_CHAIN_AVERAGE:
            if (r.out_channels != 1)
                return g_ch_err.fail(ATG_ERR_INVALID,
                                     at_row(i, "out_channels does not fit the channel operation"));
            break;
        default:
            return g_ch_err.fail(ATG_ERR_INVALID, at_row(i, "unknown channel operation"));
        }
        if (out_format == ATG_PCM_S16 && r.out_bps > 16)
            return g_ch_err.fail(ATG_ERR_INVALID,
                                 at_row(i, "S16 output with more than 16 bits per sample"));
        const atg_pcm_view &v = r.src;
        if (const atg_status st = pcm_check_view(g_ch_err, i, v))
            return st;
        if (v.src_frames >= kLimit / kMaxChannels || v.sample_offset >= kLimit ||
            r.out_offset >= kLimit || r.dither_bit0 >= kLimit)
            return g_ch_err.fail(ATG_ERR_INVALID, at_row(i, "a size or offset is 2^59 or more"));
        if (r.out_offset * out_size % 16)
            return g_ch_err.fail(ATG_ERR_INVALID,
                                 at_row(i, "out_offset is not on a 16-byte boundary"));
        const uint64_t n_out = v.src_frames * r.out_channels;
        if (!n_out)
            continue;
        any_out = true;
        if (r.out_offset + n_out > out_cap_samples)
            return g_ch_err.fail(ATG_ERR_CAPACITY, at_row(i, "output range passes out_cap_samples"));
        ranges.push_back({r.out_offset, r.out_offset + n_out});
        if (reduces(r)) {
            any_dither = true;
            if (r.dither_bit0 + n_out > dither_bytes * 8 || dither_bytes >= kLimit / 8)
                return g_ch_err.fail(ATG_ERR_INVALID,
                                     at_row(i, "dither range passes dither_bytes"));
        }
    }
    if (any_out && !d_out)
        return g_ch_err.fail(ATG_ERR_INVALID, "d_out is NULL");
    if ((uintptr_t)d_out & 15)
        return g_ch_err.fail(ATG_ERR_INVALID, "d_out is not 16-byte aligned");
    if (any_dither && !d_dither)
        return g_ch_err.fail(ATG_ERR_INVALID, "d_dither is NULL with a row that reduces bits");
    if (pcm_ranges_overlap(ranges))
        return g_ch_err.fail(ATG_ERR_INVALID, "output rows overlap");
    return ATG_OK;
}

// the device table of the rows that have output
void plan(const atg_pcm_chain_row *rows, uint32_t n, PcmRowTable<ChainRow> &tab)
{
    for (uint32_t i = 0; i < n; ++i) {
        const atg_pcm_chain_row &r = rows[i];
        if (!r.src.src_frames)
            continue;
        ChainRow c = {};
        c.src = pcm_split(r.src);
        c.frames = r.src.src_frames;
        c.out0 = r.out_offset;
        c.bit0 = r.dither_bit0;
        c.tile_frames = tile_frames_of(r.in_channels, r.out_channels);
        c.mask = (r.channel_mask ? r.channel_mask : default_mask(r.in_channels)) & 0x3Fu;
        for (uint32_t k = 0; k < kMaxChannels; ++k) {
            const uint32_t m = k < r.out_channels && r.map[k] != ATG_CHAIN_SILENT ? r.map[k]
                                                                                : kSilent;
            c.map |= m << (4 * k);
        }
        c.ic = (uint8_t)r.in_channels;
        c.oc = (uint8_t)r.out_channels;
        c.op = (uint8_t)r.channel_op;
        if (r.channel_op == ATG_CHAIN_MAP && r.in_channels == r.out_channels) {
            bool same = true;
            for (uint32_t k = 0; k < r.out_channels; ++k)
                same = same && r.map[k] == k;
            if (same)
                c.op = (uint8_t)kOpIdentity;
        }
        c.fmt = (uint8_t)r.src.format;
        c.in_bps = (uint8_t)r.in_bps;
        c.out_bps = (uint8_t)r.out_bps;
        tab.add(c, (c.frames + c.tile_frames - 1) / c.tile_frames);
    }
}

} // namespace

extern "C" {

const char *atg_pcm_chain_last_error(void) { return g_ch_err.msg.c_str(); }

uint32_t atg_pcm_chain_tile_samples(void) { return kTile; }

atg_status atg_pcm_chain_device(const atg_pcm_chain_row *rows, uint32_t n_rows, void *d_out,
                                atg_pcm_format out_format, uint64_t out_cap_samples,
                                const uint8_t *d_dither, uint64_t dither_bytes, void *stream)
{
    atg_status st = check_args(rows, n_rows, d_out, (int)out_format, out_cap_samples, d_dither,
                               dither_bytes);
    if (st != ATG_OK)
        return st;
    PcmRowTable<ChainRow> tab;
    plan(rows, n_rows, tab);
    if (tab.rows.empty())
        return ATG_OK;
    if ((st = tab.check(g_ch_err)) != ATG_OK)
        return st;
    DeviceContexts<TableCtx>::Held held; // the device that holds the output
    if ((st = g_ctxs.hold(d_out, g_ch_err, held)) != ATG_OK)
        return st;
    hipStream_t s = (hipStream_t)stream;
    const auto kernel =
        out_format == ATG_PCM_S16 ? k_pcm_chain<ATG_PCM_S16> : k_pcm_chain<ATG_PCM_S32>;
    const auto launch = [&](const ChainRow *d_rows) {
        hipLaunchKernelGGL(kernel, dim3((uint32_t)tab.tiles), dim3(kBlock), 0, s, d_rows,
                           (uint32_t)tab.rows.size(), d_out, d_dither);
    };
    float ms = 0.f;
    st = timed_launch(held->table, held->ev, tab.rows, s, g_ch_err, &ms, launch);
    if (st == ATG_OK)
        g_ch_times = {{ms}, ms >= 0.f};
    return st;
}

atg_status atg_pcm_chain_host(int device, const atg_pcm_chain_row *rows, uint32_t n_rows,
                              void *out, atg_pcm_format out_format, uint64_t out_cap_samples,
                              const uint8_t *dither, uint64_t dither_bytes)
{
    // the same refusals, on the host pointers: (void *)16 stands for "some
    // aligned output" so that only the caller's own arguments are judged
    atg_status st = check_args(rows, n_rows, out ? (void *)16 : nullptr, (int)out_format,
                               out_cap_samples, dither, dither_bytes);
    if (st != ATG_OK)
        return st;
    if ((st = use_device(device, g_ch_err)) != ATG_OK)
        return st;
    // Every source goes up at its host address modulo 16, so the kernel meets
    // the phase the caller laid out.
    std::vector<atg_pcm_chain_row> drows(rows, rows + n_rows);
    std::vector<uint64_t> at(n_rows, 0);
    uint64_t in_bytes = 0;
    for (uint32_t i = 0; i < n_rows; ++i) {
        const atg_pcm_view &v = rows[i].src;
        const uint64_t size = v.format == ATG_PCM_S32 ? 4 : 2;
        const uintptr_t first = (uintptr_t)v.d_pcm + v.sample_offset * size;
        at[i] = in_bytes + (first & 15u);
        in_bytes = (at[i] + v.src_frames * rows[i].in_channels * size + 15) / 16 * 16;
    }
    const uint64_t out_bytes = out_cap_samples * (out_format == ATG_PCM_S32 ? 4 : 2);
    DevTemp di, dout, dd;
    if (di.alloc(in_bytes ? in_bytes : 16) != hipSuccess ||
        dout.alloc(out_bytes ? out_bytes : 16) != hipSuccess ||
        dd.alloc(dither_bytes ? dither_bytes : 16) != hipSuccess)
        return g_ch_err.fail(ATG_ERR_NOMEM, "device allocation failed");
    bool ok = true;
    for (uint32_t i = 0; i < n_rows && ok; ++i) {
        const atg_pcm_view &v = rows[i].src;
        const uint64_t size = v.format == ATG_PCM_S32 ? 4 : 2;
        const uint64_t bytes = v.src_frames * rows[i].in_channels * size;
        drows[i].src.d_pcm = (const uint8_t *)di.p + at[i];
        drows[i].src.sample_offset = 0;
        if (bytes)
            ok = hipMemcpy((uint8_t *)di.p + at[i],
                           (const uint8_t *)v.d_pcm + v.sample_offset * size, bytes,
                           hipMemcpyHostToDevice) == hipSuccess;
    }
    // the output goes up first and comes back whole: what the kernel leaves
    // alone the caller gets back as it was
    if (ok && out_bytes)
        ok = hipMemcpy(dout.p, out, out_bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && dither_bytes)
        ok = hipMemcpy(dd.p, dither, dither_bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok)
        st = g_ch_err.fail(ATG_ERR_DEVICE, "copy to device failed");
    if (st == ATG_OK)
        st = atg_pcm_chain_device(drows.data(), n_rows, dout.p, out_format, out_cap_samples,
                                  dither_bytes ? (const uint8_t *)dd.p : nullptr, dither_bytes,
                                  nullptr);
    if (st == ATG_OK && out_bytes &&
        hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost) != hipSuccess)
        st = g_ch_err.fail(ATG_ERR_DEVICE, "copy from device failed");
    return st;
}

int atg_pcm_chain_kernel_times(const char **names, float *ms, int cap)
{
    return copy_times(kStageNames, g_ch_times.ms, g_ch_times.n, names, ms, cap);
}

} // extern "C"
