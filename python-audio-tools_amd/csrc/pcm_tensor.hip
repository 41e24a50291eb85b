// pcm_tensor.hip — the library's PCM rows to and from what a tensor program
// holds, one launch for a ragged table of rows either way.
//
//   to tensor    a source view (int16 or int32, at any sample offset) of
//                interleaved frames -> `channels` planar runs of float16 /
//                float32 / float64 / int32 elements, sample / 2^(bits-1), the
//                run zero-filled from the row's length to pad_frames
//                (FrameList.to_float, src/pcm.c:599-615)
//   from tensor  the runs -> interleaved int16 or int32 samples,
//                (int)(x * 2^(bits-1)) with the cast of cvttsd2si, clamped
//                (FloatFrameList.to_int, src/pcm.c:1198-1227)
//
// Tiles.  A row is cut into tiles of kTileFrames frames whatever its channel
// count; the batch's tiles form one list, a workgroup takes one, and its row
// is a binary search over the rows' first tiles (table_search.h).  kTileFrames
// is a multiple of 8, so a tile's interleaved output starts on a 16-byte
// boundary of its row's.
//
// The transposition goes through the LDS as one plane of int32 samples per
// channel, kPlane apart.  Within its plane a channel's frames lie shifted by
// the phase of that channel's run against the 16-byte units of the tensor
// buffer: element e of a unit is dword e of a group of G = 16 / sizeof(element)
// plane positions.  So the planar side of either kernel moves whole aligned
// groups (ds_read_b128 / ds_write_b128, one 16-byte global access, a wave's
// 64 lanes 1 KiB without a gap), and only the interleaved side addresses the
// LDS sample by sample.  kPlane is 4 modulo 32 dwords: the channels an
// interleaved 16-byte unit holds (two planes four apart for 8 channels, four
// planes for 4, alternating for 2) fall on different banks.  On the
// interleaved side a lane holds the 2, 4 or 8 frames of its unit, so lanes
// lie that many dwords apart in a plane and meet a bank as many times; a
// dword of padding after every 32 removes that and was measured to change
// nothing, so the planes stay plain.  The dynamic LDS is
// sized by the call's largest channel count, so a stereo batch keeps the CU's
// waves.
//
// Ends.  A run may start at any element.  A group that lies whole inside the
// tile's part of the run is one 16-byte access; the first and last group of a
// tile, when they are not, go element by element, so nothing outside a run is
// read or written.  The PCM side is pcm_rows.h's: aligned 16-byte units that
// hold a sample of the row, the last short group sample by sample.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/atgpu.h"
#include "host_common.h"
#include "pcm_rows.h"
#include "table_search.h"

#pragma clang fp contract(off)

namespace {

thread_local ErrSlot g_pt_err;

constexpr uint32_t kTileFrames = 1024;
constexpr uint32_t kBlock = 256;
constexpr uint32_t kMaxChannels = 8;
// a plane: a tile's frames behind a phase of at most 7, rounded up to 4
// modulo 32 dwords
constexpr uint32_t kPlane = 1060;
constexpr uint64_t kLimit = 1ull << 59;
static_assert(kPlane >= kTileFrames + 8 && kPlane % 32 == 4, "plane padding");

const char *const kStageNames[2] = {"to_tensor", "from_tensor"};
// the calling thread's last launch: which of the two, and its time
thread_local StageTimes<1> g_pt_times;
thread_local int g_pt_which = 0;

struct ToRow {
    PcmSplit src;     // the source: its aligned pointer and first sample
    uint64_t frames, pad;
    uint64_t e0;      // element index, from the aligned output base, of channel 0's run
    uint64_t cstride;
    uint64_t tile0;   // the row's first tile in the batch's list
    uint8_t ch, bps, fmt, reserved[5];
};

struct FromRow {
    uint64_t e0;      // element index, from the aligned input base, of channel 0's run
    uint64_t cstride, frames;
    uint64_t out0;    // index in the output of the row's first sample
    uint64_t tile0;
    uint8_t ch, bps, reserved[6];
};

DeviceContexts<TableCtx> g_ctxs;

template <int DT> struct Elem;
template <> struct Elem<ATG_TENSOR_F16> { typedef _Float16 T; };
template <> struct Elem<ATG_TENSOR_F32> { typedef float T; };
template <> struct Elem<ATG_TENSOR_F64> { typedef double T; };
template <> struct Elem<ATG_TENSOR_I32> { typedef int32_t T; };

// sample -> element.  The scale is a power of two and a sample of at most 24
// bits is exact in float32, so the float32 is the double's nearest-even
// rounding (for any int32 as well: one rounding in the conversion, an exact
// scale) and the float16 is one nearest-even step from it, subnormals kept.
template <int DT> __device__ __forceinline__ typename Elem<DT>::T to_elem(int32_t s, uint32_t bps)
{
    if constexpr (DT == ATG_TENSOR_I32) {
        return s;
    } else if constexpr (DT == ATG_TENSOR_F64) {
        return (double)s * __hiloint2double((int)((1023u - (bps - 1)) << 20), 0);
    } else {
        const float x = (float)s * __uint_as_float((127u - (bps - 1)) << 23);
        if constexpr (DT == ATG_TENSOR_F16)
            return (_Float16)x;
        else
            return x;
    }
}

// element -> sample: cvttsd2si of x * 2^(bps-1), clamped to the width
template <int DT> __device__ __forceinline__ int32_t from_elem(typename Elem<DT>::T x, uint32_t bps)
{
    const int32_t smin = -(1 << (bps - 1)), smax = (1 << (bps - 1)) - 1;
    int32_t v;
    if constexpr (DT == ATG_TENSOR_I32) {
        v = x;
    } else if constexpr (DT != ATG_TENSOR_F64) {
        // The same in float32, where it is exact: the scale is a power of two
        // (a product past float32's range is far past int32's on either
        // path), the two bounds fall on the float32 values -2^31 and 2^31,
        // and a float32 inside them has its integer part in int32.
        const float y = (float)x * __uint_as_float((127u + (bps - 1)) << 23);
        v = (y >= -2147483648.0f && y < 2147483648.0f) ? (int32_t)y : INT32_MIN;
    } else {
        const double y = (double)x * __hiloint2double((int)((1023u + (bps - 1)) << 20), 0);
        // false for NaN as well
        v = (y > -2147483649.0 && y < 2147483648.0) ? (int32_t)y : INT32_MIN;
    }
    return v > smax ? smax : (v < smin ? smin : v);
}

// the phase of channel c's run within a group of G elements
template <uint32_t G>
__device__ __forceinline__ uint32_t phase_of(uint32_t e_lo, uint32_t cs_lo, uint32_t c)
{
    return (e_lo + c * cs_lo) & (G - 1);
}

// ------------------------------------------------------------ PCM -> tensor

// The samples of one aligned source unit, unit j of the tile's, into the
// planes.  The tile's first sample is sample `skew` of unit 0; a sample
// before it, or past the tile's n_src frames, belongs to no plane.
template <int FIN, uint32_t G>
__device__ __forceinline__ void scatter(Unit v, uint32_t j, uint32_t skew, uint32_t ch,
                                        uint32_t n_src, uint32_t e_lo, uint32_t cs_lo,
                                        int32_t *lds)
{
    constexpr uint32_t kPer = FIN == ATG_PCM_S32 ? 4 : 8;
    // sample j * kPer - skew of the tile, 8 frames up so that it divides unsigned
    const uint32_t biased = j * kPer + 8 * ch - skew;
    const uint32_t fq = biased / ch;
    uint32_t c = biased - fq * ch;
    int32_t f = (int32_t)fq - 8;
#pragma unroll
    for (uint32_t t = 0; t < kPer; ++t) {
        int32_t s;
        if (FIN == ATG_PCM_S32)
            s = (int32_t)v[t];
        else
            s = (t & 1) ? (int32_t)v[t / 2] >> 16 : (int32_t)(int16_t)(v[t / 2] & 0xFFFFu);
        if ((uint32_t)f < n_src) // f < 0 wraps above it
            lds[c * kPlane + phase_of<G>(e_lo, cs_lo, c) + (uint32_t)f] = s;
        if (++c == ch) {
            c = 0;
            ++f;
        }
    }
}

// The aligned units that cover source frames [fa, fa + n_src) of the row,
// scattered into the planes.
template <int FIN, uint32_t G>
__device__ __forceinline__ void stage(const ToRow &R, uint64_t fa, uint32_t n_src, uint32_t e_lo,
                                      uint32_t cs_lo, int32_t *lds)
{
    constexpr uint32_t kPer = FIN == ATG_PCM_S32 ? 4 : 8;
    const uint32_t ch = R.ch;
    const PcmUnits u = pcm_units(R.src.lo, fa, n_src, ch, kPer);
    pcm_load_units<kTileFrames * kMaxChannels / kPer / kBlock, kBlock>(
        R.src.p, u.u0, u.nu, [=](Unit v, uint32_t j) {
            scatter<FIN, G>(v, j, u.skew, ch, n_src, e_lo, cs_lo, lds);
        });
}

template <int DT>
__global__ __launch_bounds__(kBlock) void k_pcm_to_tensor(const ToRow *__restrict__ rows,
                                                          uint32_t n, void *out)
{
    typedef typename Elem<DT>::T T;
    constexpr uint32_t G = 16 / sizeof(T);
    constexpr uint32_t kGroups = kTileFrames / G + 1; // of a plane, with a phase
    typedef T Vec __attribute__((ext_vector_type(G)));
    typedef int32_t IVec __attribute__((ext_vector_type(G)));
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];

    const uint64_t tile = blockIdx.x;
    const ToRow R = rows[last_le(rows, n, tile, &ToRow::tile0)];
    const uint64_t fa = (tile - R.tile0) * kTileFrames;
    if (fa >= R.pad)
        return;
    const uint32_t nf = R.pad - fa < kTileFrames ? (uint32_t)(R.pad - fa) : kTileFrames;
    const uint32_t n_src =
        fa >= R.frames ? 0 : (R.frames - fa < kTileFrames ? (uint32_t)(R.frames - fa) : kTileFrames);
    const uint32_t ch = R.ch;
    const uint64_t e = R.e0 + fa; // channel 0's frame fa
    const uint32_t e_lo = (uint32_t)e & (G - 1), cs_lo = (uint32_t)R.cstride & (G - 1);
    if (n_src) { // the same for the whole workgroup
        if (R.fmt == ATG_PCM_S32)
            stage<ATG_PCM_S32, G>(R, fa, n_src, e_lo, cs_lo, lds);
        else
            stage<ATG_PCM_S16, G>(R, fa, n_src, e_lo, cs_lo, lds);
    }
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < ch * kGroups; idx += kBlock) {
        const uint32_t c = idx / kGroups, g = idx - c * kGroups;
        const uint32_t ph = phase_of<G>(e_lo, cs_lo, c);
        if (g * G >= ph + nf)
            continue;
        const IVec x = *(const IVec *)(lds + c * kPlane + g * G);
        const int32_t f0 = (int32_t)(g * G) - (int32_t)ph; // the group's first frame in the tile
        Vec y;
#pragma unroll
        for (uint32_t t = 0; t < G; ++t) // past the row's length, or no source at all: zero
            y[t] = to_elem<DT>((uint32_t)(f0 + (int32_t)t) < n_src ? x[t] : 0, R.bps);
        // e + c * cstride - ph is a multiple of G: the group is an aligned unit
        T *dst = (T *)out + (e + c * R.cstride - ph) + g * G;
        if (f0 >= 0 && (uint32_t)f0 + G <= nf) {
            __builtin_nontemporal_store(y, (Vec *)dst);
        } else {
#pragma unroll
            for (uint32_t t = 0; t < G; ++t)
                if ((uint32_t)(f0 + (int32_t)t) < nf)
                    dst[t] = y[t];
        }
    }
}

// ------------------------------------------------------------ tensor -> PCM

template <int DT, int FOUT>
__global__ __launch_bounds__(kBlock) void k_pcm_from_tensor(const FromRow *__restrict__ rows,
                                                            uint32_t n, const void *in, void *out)
{
    typedef typename Elem<DT>::T T;
    constexpr uint32_t G = 16 / sizeof(T);
    constexpr uint32_t kGroups = kTileFrames / G + 1;
    typedef T Vec __attribute__((ext_vector_type(G)));
    typedef int32_t IVec __attribute__((ext_vector_type(G)));
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];

    const uint64_t tile = blockIdx.x;
    const FromRow R = rows[last_le(rows, n, tile, &FromRow::tile0)];
    const uint64_t fa = (tile - R.tile0) * kTileFrames;
    if (fa >= R.frames)
        return;
    const uint32_t nf = R.frames - fa < kTileFrames ? (uint32_t)(R.frames - fa) : kTileFrames;
    const uint32_t ch = R.ch;
    const uint64_t e = R.e0 + fa;
    const uint32_t e_lo = (uint32_t)e & (G - 1), cs_lo = (uint32_t)R.cstride & (G - 1);
    // The runs, converted, into the planes: whole aligned groups, kAhead of
    // a lane's loads in flight before the first is converted (a stereo tile
    // is three groups a lane, so all of its loads are).
    constexpr uint32_t kAhead = 4;
    const uint32_t n_groups = ch * kGroups;
    for (uint32_t first = threadIdx.x; first < n_groups; first += kAhead * kBlock) {
        Vec y[kAhead];
        uint32_t at[kAhead]; // the group's place in the planes, or none
#pragma unroll
        for (uint32_t a = 0; a < kAhead; ++a) {
            const uint32_t idx = first + a * kBlock;
            const uint32_t c = idx / kGroups, g = idx - c * kGroups;
            const uint32_t ph = phase_of<G>(e_lo, cs_lo, c);
            at[a] = UINT32_MAX;
            y[a] = Vec{};
            if (idx >= n_groups || g * G >= ph + nf)
                continue;
            at[a] = c * kPlane + g * G;
            const int32_t f0 = (int32_t)(g * G) - (int32_t)ph;
            const T *src = (const T *)in + (e + c * R.cstride - ph) + g * G;
            if (f0 >= 0 && (uint32_t)f0 + G <= nf) {
                y[a] = *(const Vec *)src;
            } else {
#pragma unroll
                for (uint32_t t = 0; t < G; ++t)
                    if ((uint32_t)(f0 + (int32_t)t) < nf)
                        y[a][t] = src[t];
            }
        }
#pragma unroll
        for (uint32_t a = 0; a < kAhead; ++a) {
            if (at[a] == UINT32_MAX)
                continue;
            IVec x;
#pragma unroll
            for (uint32_t t = 0; t < G; ++t)
                x[t] = from_elem<DT>(y[a][t], R.bps);
            *(IVec *)(lds + at[a]) = x;
        }
    }
    __syncthreads();
    // a lane interleaves the samples of one 16-byte store (pcm_store_group)
    constexpr uint32_t GO = FOUT == ATG_PCM_S16 ? 8 : 4;
    const uint32_t n_out = nf * ch;
    const uint64_t o0 = R.out0 + fa * ch; // a multiple of 8 past the row's start
    for (uint32_t q = threadIdx.x * GO; q < n_out; q += kBlock * GO) {
        uint32_t f = q / ch, c = q - f * ch;
        int32_t x[GO];
#pragma unroll
        for (uint32_t j = 0; j < GO; ++j) {
            x[j] = q + j < n_out ? lds[c * kPlane + phase_of<G>(e_lo, cs_lo, c) + f] : 0;
            if (++c == ch) {
                c = 0;
                ++f;
            }
        }
        pcm_store_group<FOUT>(x, out, o0, q, n_out);
    }
}

// ---------------------------------------------------------------- host side

uint32_t elem_size(int dtype)
{
    switch (dtype) {
    case ATG_TENSOR_F16:
        return 2;
    case ATG_TENSOR_F32:
    case ATG_TENSOR_I32:
        return 4;
    case ATG_TENSOR_F64:
        return 8;
    }
    return 0;
}

// every refusal of atg_pcm_to_tensor_device, before any GPU call
atg_status check_to(const atg_pcm_to_tensor_row *rows, uint32_t n, const void *d_out, int dtype,
                    uint64_t out_cap_elems)
{
    if (n && !rows)
        return g_pt_err.fail(ATG_ERR_INVALID, "rows is NULL");
    const uint32_t size = elem_size(dtype);
    if (!size)
        return g_pt_err.fail(ATG_ERR_INVALID, "unknown dtype");
    if ((uintptr_t)d_out & (size - 1))
        return g_pt_err.fail(ATG_ERR_INVALID, "d_out is not aligned to its element size");
    bool any = false;
    std::vector<std::pair<uint64_t, uint64_t>> ranges; // channel runs [start, end)
    for (uint32_t i = 0; i < n; ++i) {
        const atg_pcm_to_tensor_row &r = rows[i];
        const atg_pcm_view &v = r.src;
        if (r.channels < 1 || r.channels > kMaxChannels)
            return g_pt_err.fail(ATG_ERR_INVALID, at_row(i, "channel count outside 1..8"));
        if (r.bits_per_sample < 1 || r.bits_per_sample > 24)
            return g_pt_err.fail(ATG_ERR_INVALID, at_row(i, "bits per sample outside 1..24"));
        if (const atg_status st = pcm_check_view(g_pt_err, i, v))
            return st;
        if (v.src_frames >= kLimit / kMaxChannels || v.sample_offset >= kLimit ||
            r.pad_frames >= kLimit / kMaxChannels || r.out_offset >= kLimit ||
            r.channel_stride >= kLimit / kMaxChannels)
            return g_pt_err.fail(ATG_ERR_INVALID, at_row(i, "a size or offset is 2^59 or more"));
        if (r.pad_frames < v.src_frames)
            return g_pt_err.fail(ATG_ERR_INVALID, at_row(i, "pad_frames is below src_frames"));
        if (r.channel_stride < r.pad_frames)
            return g_pt_err.fail(ATG_ERR_INVALID, at_row(i, "channel_stride is below pad_frames"));
        if (!r.pad_frames)
            continue;
        any = true;
        if (r.out_offset + (r.channels - 1) * r.channel_stride + r.pad_frames > out_cap_elems)
            return g_pt_err.fail(ATG_ERR_CAPACITY, at_row(i, "a channel run passes out_cap_elems"));
        for (uint32_t c = 0; c < r.channels; ++c) {
            const uint64_t at = r.out_offset + c * r.channel_stride;
            ranges.push_back({at, at + r.pad_frames});
        }
    }
    if (any && !d_out)
        return g_pt_err.fail(ATG_ERR_INVALID, "d_out is NULL");
    if (pcm_ranges_overlap(ranges))
        return g_pt_err.fail(ATG_ERR_INVALID, "channel runs overlap");
    return ATG_OK;
}

atg_status check_from(const atg_pcm_from_tensor_row *rows, uint32_t n, const void *d_in,
                      int dtype, uint64_t in_cap_elems, const void *d_out, int out_format,
                      uint64_t out_cap_samples)
{
    if (n && !rows)
        return g_pt_err.fail(ATG_ERR_INVALID, "rows is NULL");
    const uint32_t size = elem_size(dtype);
    if (!size)
        return g_pt_err.fail(ATG_ERR_INVALID, "unknown dtype");
    if (out_format != ATG_PCM_S16 && out_format != ATG_PCM_S32)
        return g_pt_err.fail(ATG_ERR_INVALID, "unknown output format");
    if ((uintptr_t)d_in & (size - 1))
        return g_pt_err.fail(ATG_ERR_INVALID, "d_in is not aligned to its element size");
    if ((uintptr_t)d_out & 15)
        return g_pt_err.fail(ATG_ERR_INVALID, "d_out is not 16-byte aligned");
    const uint32_t out_size = out_format == ATG_PCM_S32 ? 4 : 2;
    bool any = false;
    std::vector<std::pair<uint64_t, uint64_t>> ranges; // output [start, end)
    for (uint32_t i = 0; i < n; ++i) {
        const atg_pcm_from_tensor_row &r = rows[i];
        if (r.channels < 1 || r.channels > kMaxChannels)
            return g_pt_err.fail(ATG_ERR_INVALID, at_row(i, "channel count outside 1..8"));
        if (r.bits_per_sample < 1 || r.bits_per_sample > 24)
            return g_pt_err.fail(ATG_ERR_INVALID, at_row(i, "bits per sample outside 1..24"));
        if (out_format == ATG_PCM_S16 && r.bits_per_sample > 16)
            return g_pt_err.fail(ATG_ERR_INVALID,
                                 at_row(i, "S16 output with more than 16 bits per sample"));
        if (r.frames >= kLimit / kMaxChannels || r.in_offset >= kLimit ||
            r.out_offset >= kLimit || r.channel_stride >= kLimit / kMaxChannels)
            return g_pt_err.fail(ATG_ERR_INVALID, at_row(i, "a size or offset is 2^59 or more"));
        if (r.channel_stride < r.frames)
            return g_pt_err.fail(ATG_ERR_INVALID, at_row(i, "channel_stride is below frames"));
        if (r.out_offset * out_size % 16)
            return g_pt_err.fail(ATG_ERR_INVALID,
                                 at_row(i, "out_offset is not on a 16-byte boundary"));
        if (!r.frames)
            continue;
        any = true;
        if (r.in_offset + (r.channels - 1) * r.channel_stride + r.frames > in_cap_elems)
            return g_pt_err.fail(ATG_ERR_CAPACITY, at_row(i, "a channel run passes in_cap_elems"));
        const uint64_t n_out = r.frames * r.channels;
        if (r.out_offset + n_out > out_cap_samples)
            return g_pt_err.fail(ATG_ERR_CAPACITY, at_row(i, "output range passes out_cap_samples"));
        ranges.push_back({r.out_offset, r.out_offset + n_out});
    }
    if (any && !d_in)
        return g_pt_err.fail(ATG_ERR_INVALID, "d_in is NULL");
    if (any && !d_out)
        return g_pt_err.fail(ATG_ERR_INVALID, "d_out is NULL");
    if (pcm_ranges_overlap(ranges))
        return g_pt_err.fail(ATG_ERR_INVALID, "output rows overlap");
    return ATG_OK;
}

// the table's one timed launch, on the device that holds the tensor, d_where
template <class Row, class Launch>
atg_status run(const void *d_where, const PcmRowTable<Row> &tab, hipStream_t s, int which,
               Launch launch)
{
    if (tab.rows.empty())
        return ATG_OK;
    DeviceContexts<TableCtx>::Held held;
    atg_status st = tab.check(g_pt_err);
    if (st != ATG_OK || (st = g_ctxs.hold(d_where, g_pt_err, held)) != ATG_OK)
        return st;
    float ms = 0.f;
    st = timed_launch(held->table, held->ev, tab.rows, s, g_pt_err, &ms, launch);
    if (st == ATG_OK) {
        g_pt_times = {{ms}, ms >= 0.f};
        g_pt_which = which;
    }
    return st;
}

} // namespace

extern "C" {

const char *atg_pcm_tensor_last_error(void) { return g_pt_err.msg.c_str(); }

uint32_t atg_pcm_tensor_tile_frames(void) { return kTileFrames; }

atg_status atg_pcm_to_tensor_device(const atg_pcm_to_tensor_row *rows, uint32_t n_rows,
                                    void *d_out, atg_tensor_dtype dtype, uint64_t out_cap_elems,
                                    void *stream)
{
    atg_status st = check_to(rows, n_rows, d_out, (int)dtype, out_cap_elems);
    if (st != ATG_OK)
        return st;
    // the output is addressed in elements from its pointer rounded down to 16 bytes
    const uint32_t size = elem_size((int)dtype);
    const uintptr_t base = (uintptr_t)d_out & ~(uintptr_t)15;
    const uint64_t extra = ((uintptr_t)d_out & 15u) / size;
    PcmRowTable<ToRow> tab;
    uint32_t max_ch = 0;
    for (uint32_t i = 0; i < n_rows; ++i) {
        const atg_pcm_to_tensor_row &r = rows[i];
        if (!r.pad_frames)
            continue;
        ToRow t = {};
        t.src = pcm_split(r.src);
        t.frames = r.src.src_frames;
        t.pad = r.pad_frames;
        t.e0 = extra + r.out_offset;
        t.cstride = r.channel_stride;
        t.ch = (uint8_t)r.channels;
        t.bps = (uint8_t)r.bits_per_sample;
        t.fmt = (uint8_t)r.src.format;
        max_ch = std::max(max_ch, r.channels);
        tab.add(t, (t.pad + kTileFrames - 1) / kTileFrames);
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((uint32_t)tab.tiles), block(kBlock);
    const size_t lds = sizeof(int32_t) * kPlane * max_ch;
    const uint32_t n = (uint32_t)tab.rows.size();
    void *out = (void *)base;
    return run(d_out, tab, s, 0, [&](const ToRow *d_rows) {
        switch ((int)dtype) {
        case ATG_TENSOR_F16:
            hipLaunchKernelGGL(k_pcm_to_tensor<ATG_TENSOR_F16>, grid, block, lds, s, d_rows, n, out);
            break;
        case ATG_TENSOR_F32:
            hipLaunchKernelGGL(k_pcm_to_tensor<ATG_TENSOR_F32>, grid, block, lds, s, d_rows, n, out);
            break;
        case ATG_TENSOR_F64:
            hipLaunchKernelGGL(k_pcm_to_tensor<ATG_TENSOR_F64>, grid, block, lds, s, d_rows, n, out);
            break;
        default:
            hipLaunchKernelGGL(k_pcm_to_tensor<ATG_TENSOR_I32>, grid, block, lds, s, d_rows, n, out);
        }
    });
}

atg_status atg_pcm_from_tensor_device(const atg_pcm_from_tensor_row *rows, uint32_t n_rows,
                                      const void *d_in, atg_tensor_dtype dtype,
                                      uint64_t in_cap_elems, void *d_out,
                                      atg_pcm_format out_format, uint64_t out_cap_samples,
                                      void *stream)
{
    atg_status st = check_from(rows, n_rows, d_in, (int)dtype, in_cap_elems, d_out,
                               (int)out_format, out_cap_samples);
    if (st != ATG_OK)
        return st;
    const uint32_t size = elem_size((int)dtype);
    const uintptr_t base = (uintptr_t)d_in & ~(uintptr_t)15;
    const uint64_t extra = ((uintptr_t)d_in & 15u) / size;
    PcmRowTable<FromRow> tab;
    uint32_t max_ch = 0;
    for (uint32_t i = 0; i < n_rows; ++i) {
        const atg_pcm_from_tensor_row &r = rows[i];
        if (!r.frames)
            continue;
        FromRow t = {};
        t.e0 = extra + r.in_offset;
        t.cstride = r.channel_stride;
        t.frames = r.frames;
        t.out0 = r.out_offset;
        t.ch = (uint8_t)r.channels;
        t.bps = (uint8_t)r.bits_per_sample;
        max_ch = std::max(max_ch, r.channels);
        tab.add(t, (t.frames + kTileFrames - 1) / kTileFrames);
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((uint32_t)tab.tiles), block(kBlock);
    const size_t lds = sizeof(int32_t) * kPlane * max_ch;
    const uint32_t n = (uint32_t)tab.rows.size();
    const void *in = (const void *)base;
#define ATG_FROM(DT)                                                                          \
    if (out_format == ATG_PCM_S16)                                                            \
        hipLaunchKernelGGL((k_pcm_from_tensor<DT, ATG_PCM_S16>), grid, block, lds, s, d_rows, \
                           n, in, d_out);                                                     \
    else                                                                                      \
        hipLaunchKernelGGL((k_pcm_from_tensor<DT, ATG_PCM_S32>), grid, block, lds, s, d_rows, \
                           n, in, d_out)
    return run(d_in, tab, s, 1, [&](const FromRow *d_rows) {
        switch ((int)dtype) {
        case ATG_TENSOR_F16:
            ATG_FROM(ATG_TENSOR_F16);
            break;
        case ATG_TENSOR_F32:
            ATG_FROM(ATG_TENSOR_F32);
            break;
        case ATG_TENSOR_F64:
            ATG_FROM(ATG_TENSOR_F64);
            break;
        default:
            ATG_FROM(ATG_TENSOR_I32);
        }
    });
#undef ATG_FROM
}

int atg_pcm_tensor_kernel_times(const char **names, float *ms, int cap)
{
    return copy_times(kStageNames + g_pt_which, g_pt_times.ms, g_pt_times.n, names, ms, cap);
}

} // extern "C"
