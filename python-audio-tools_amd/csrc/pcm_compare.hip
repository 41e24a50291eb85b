// pcm_compare.hip — are two PCM streams the same audio, and at what offset?
// The device side of trackcmp: the first differing PCM frame of every pair of
// a batch, and the frame shift in [-K, K] at which a pair matches.
//
// Views.  A view is an infinite sequence of frames over a finite source:
// view frame i is source frame window_offset + i, and source frames outside
// [0, src_frames) are silence (PCMReaderWindow's padding at both ends).  A
// pair compares `frames` frames of view A with view B; each side is int16 or
// int32 on its own and an int16 sample counts by its sign-extended value.
//
// Compare pass (k_pcm_compare).  Everything is done in samples.  A pair of
// frames * channels samples is cut into tiles of kTile frames, the batch's
// tiles form one list, and workgroups walk it grid-stride, so one long pair
// spreads over the machine as 1024 short ones do.  The list holds every
// pair's first tile first, then the other tiles pair by pair; the pair of one
// of those is a binary search over the pairs' first numbers among them (as
// accuraterip.hip finds a tile's track).
//
// Alignment.  Both buffers are addressed in samples from their pointer
// rounded down to 16 bytes (pcm_rows.h).  A lane takes 8 consecutive samples whose A index
// is a multiple of 8, so A is one (int16) or two (int32) aligned 16-byte
// loads.  The same 8 samples of B start at any index: the lane loads the two
// (int16) or three (int32) aligned units that cover them.  B's phase within
// a unit is the same for every chunk of a pair, and every (format, format,
// phase) has code of its own, so which registers are compared is fixed at
// compile time (an odd int16 phase is a 16-bit funnel per word); a phase
// used as a run-time index sends the loaded units through scratch.  A unit
// is loaded only if it holds a sample of the source; samples outside the
// source are zeroed and samples outside the tile are masked from the
// comparison.  A lane has the loads of kDeep chunks in flight at once.
//
// Minimum.  A lane keeps its first differing sample, as a frame.  The usual
// tile has none and ends at one barrier (__syncthreads_or); otherwise the
// wave reduces by shuffles, the workgroup through LDS, and one atomicMin
// lands in the pair's slot.  A tile that starts at or after the slot's
// present value skips its loads: everything it could report is no smaller,
// and the slot only ever holds frames that differ, so it ends as the exact
// minimum for every schedule.  With the first tiles first, a mismatch near a
// pair's start is on record before most of its other tiles begin.
//
// Offset search.  S = { k in [-K, K] : A(i) == B(i + k) for all i }, the
// answer the k of smallest |k|, +k before -k.  One compare launch gives the
// first non-silent frame of A (A against an empty source) and the mismatch
// at shift 0.  A probe of up to kProbe frames of A from that frame is tested
// against B at all 2K + 1 shifts (k_pcm_probe, one lane per shift): a shift in
// S passes, because the probe is part of the range.  The survivors are
// verified by the compare kernel in order of |k|, a bounded number per
// launch, until one passes.  A wholly silent A has every shift as candidate.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/atgpu.h"
#include "host_common.h"
#include "pcm_rows.h"
#include "table_search.h"
#include "wave.h"

namespace {

thread_local ErrSlot g_pc_err;
#define CHIP(expr) ATG_HIP_TRY(g_pc_err, expr, #expr)

constexpr uint32_t kTile = 4096; // PCM frames per tile
constexpr uint32_t kBlock = 256;
constexpr uint32_t kMaxBlocks = 2048;
constexpr uint32_t kMaxOffset = 65535;
constexpr uint32_t kMaxChannels = 8;
constexpr uint32_t kProbe = 1024;       // frames of the search's probe
constexpr uint32_t kVerifyPairs = 8192; // compare pairs per verification launch
constexpr uint32_t kVerifyChunk = 256;  // of them, at most this many per pair
constexpr uint64_t kNone = ATG_PCM_NO_MISMATCH;
constexpr uint64_t kLimit = 1ull << 62;

const char *const kStageNames[2] = {"compare", "probe"};
thread_local StageTimes<2> g_pc_times; // summed over a call's compare launches, its probe launch

// a view as the kernels see it: sample indices count from `p`, the caller's
// pointer rounded down to 16 bytes
struct CmpView {
    const void *p;
    long long base;   // index of view sample 0
    long long lo, hi; // the source's samples; lo == hi == 0 when it has none
};

struct CmpPair {
    CmpView a, b;
    uint64_t n;     // samples to compare: frames * channels
    uint64_t rest0; // among the batch's tiles that are no pair's first, the pair's first
    uint32_t channels;
    uint32_t fmt;   // bit 0: A is int32, bit 1: B is int32
    uint32_t slot;  // where the minimum goes
    uint32_t phase; // (b.base - a.base) modulo 8
};

struct ProbeJob {
    CmpView a, b;
    uint64_t first;  // view sample of the probe's first sample
    uint32_t n;      // samples of the probe
    uint32_t channels;
    uint32_t fmt;
    uint32_t pad;
};

struct CmpCtx {
    DevBuf pairs, first, jobs, bits;
    hipEvent_t ev[2] = {nullptr, nullptr};
};
DeviceContexts<CmpCtx> g_ctxs;

// The 8 samples at indices idx .. idx + 7 of a view's buffer, as the aligned
// 16-byte units that cover them.  PH is idx modulo the samples of a unit (4
// for int32, 8 for int16): the same for every chunk of a pair, so each phase
// has code of its own and every register index is fixed.
template <int FMT, int PH> struct Chunk {
    static constexpr int kPer = FMT == ATG_PCM_S32 ? 4 : 8;
    static constexpr int kUnits = (PH + 8 + kPer - 1) / kPer;
    Unit u[kUnits];

    // GUARD: load a unit only if it holds a sample of the source.  Without
    // it the caller knows that idx .. idx + 7 all lie in the source, and then
    // every unit does.
    template <bool GUARD> __device__ __forceinline__ void fetch(const CmpView &v, long long idx)
    {
        const long long u0 = (idx - PH) >> (FMT == ATG_PCM_S32 ? 2 : 3);
#pragma unroll
        for (int k = 0; k < kUnits; ++k) {
            const long long f = (u0 + k) * kPer;
            if (!GUARD || (f < v.hi && f + kPer > v.lo))
                u[k] = ((Units)v.p)[u0 + k];
            else
                u[k] = Unit{0, 0, 0, 0};
        }
    }

    __device__ __forceinline__ void samples(int (&out)[8]) const
    {
        uint32_t w[4 * kUnits];
#pragma unroll
        for (int k = 0; k < kUnits; ++k) {
            w[4 * k] = u[k].x;
            w[4 * k + 1] = u[k].y;
            w[4 * k + 2] = u[k].z;
            w[4 * k + 3] = u[k].w;
        }
        if (FMT == ATG_PCM_S32) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                out[j] = (int)w[PH + j];
        } else {
            // an odd phase starts in the high half of a word
            constexpr int q = PH >> 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t x = (PH & 1) ? (w[q + j] >> 16) | (w[(q + j + 1) % (4 * kUnits)] << 16)
                                            : w[q + j];
                out[2 * j] = (int)(x << 16) >> 16;
                out[2 * j + 1] = (int)x >> 16;
            }
        }
    }
};

// silence where idx + j is outside the source
__device__ __forceinline__ void silence_outside(const CmpView &v, long long idx, int (&out)[8])
{
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (idx + j < v.lo || idx + j >= v.hi)
            out[j] = 0;
}

// one sample, for the probe
__device__ __forceinline__ int sample_at(const CmpView &v, bool s32, long long idx)
{
    if (idx < v.lo || idx >= v.hi)
        return 0;
    return s32 ? ((const int32_t *)v.p)[idx] : (int)((const int16_t *)v.p)[idx];
}

// This lane's first differing view sample among [s0, s1) of a pair, or kNone.
// A lane takes kDeep chunks a round, all their loads issued before the first
// comparison.  PH is the phase of B's index at a chunk's start.
constexpr int kDeep = 4;

template <int FA, int FB, int PH>
__device__ __forceinline__ uint64_t tile_first(const CmpView &A, const CmpView &B, uint64_t s0,
                                               uint64_t s1)
{
    constexpr long long kStep = (long long)kBlock * 8;
    const long long end = (long long)s1 + A.base;
    const long long delta = B.base - A.base;
    uint64_t best = kNone;
    for (long long c = (((long long)s0 + A.base) & ~7ll) + (long long)threadIdx.x * 8; c < end;
         c += kStep * kDeep) {
        Chunk<FA, 0> ra[kDeep];
        Chunk<FB, PH> rb[kDeep];
        const long long last = c + kStep * (kDeep - 1);
        // the usual case: all of this round's chunks inside both sources
        const bool inside = last < end && c >= A.lo && last + 8 <= A.hi && c + delta >= B.lo &&
                            last + delta + 8 <= B.hi;
        if (inside) {
#pragma unroll
            for (int d = 0; d < kDeep; ++d) {
                ra[d].template fetch<false>(A, c + kStep * d);
                rb[d].template fetch<false>(B, c + kStep * d + delta);
            }
        } else {
#pragma unroll
            for (int d = 0; d < kDeep; ++d) {
                // a chunk past the tile's end loads nothing
                const long long cd = c + kStep * d < end ? c + kStep * d : A.hi + 8;
                ra[d].template fetch<true>(A, cd);
                rb[d].template fetch<true>(B, c + kStep * d < end ? cd + delta : B.hi + 8 + PH);
            }
        }
#pragma unroll
        for (int d = 0; d < kDeep; ++d) {
            const long long cd = c + kStep * d;
            int a[8], b[8];
            ra[d].samples(a);
            rb[d].samples(b);
            if (!inside) {
                silence_outside(A, cd, a);
                silence_outside(B, cd + delta, b);
            }
            uint32_t m = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                m |= (uint32_t)(a[j] != b[j]) << j;
            if (m && cd < end) {
                const long long s = cd - A.base; // view sample of a[0]
                if (s < (long long)s0)
                    m &= ~((1u << (uint32_t)((long long)s0 - s)) - 1u);
                if (s + 8 > (long long)s1)
                    m &= (1u << (uint32_t)((long long)s1 - s)) - 1u;
                if (m) {
                    const uint64_t at = (uint64_t)(s + (__ffs(m) - 1));
                    best = at < best ? at : best;
                }
            }
        }
        if (best != kNone)
            break; // this lane's later chunks are later samples
    }
    return best;
}

// the phase is the pair's: pick its code
template <int FA, int FB, int PH = 0> struct ByPhase {
    static __device__ __forceinline__ uint64_t run(uint32_t ph, const CmpView &A, const CmpView &B,
                                                   uint64_t s0, uint64_t s1)
    {
        if (ph == PH)
            return tile_first<FA, FB, PH>(A, B, s0, s1);
        if constexpr (PH + 1 < (FB == ATG_PCM_S32 ? 4 : 8))
            return ByPhase<FA, FB, PH + 1>::run(ph, A, B, s0, s1);
        else
            return kNone;
    }
};

// Batch tile `tile` -> its pair and its number within the pair.  The first
// tiles of all pairs come first in the list, so that a mismatch near a
// pair's start is on record before most of its other tiles are begun; the
// other tiles follow pair by pair, found by a binary search over the pairs'
// first numbers among them.
__device__ __forceinline__ uint32_t pair_of_tile(const CmpPair *pr, uint32_t n, uint64_t tile,
                                                 uint64_t *within)
{
    if (tile < n) {
        *within = 0;
        return (uint32_t)tile;
    }
    const uint64_t rest = tile - n;
    // the last i with pr[i].rest0 <= rest: it has such tiles
    const uint32_t l = last_le(pr, n, rest, &CmpPair::rest0);
    *within = 1 + (rest - pr[l].rest0);
    return l;
}

__global__ __launch_bounds__(kBlock) void k_pcm_compare(const CmpPair *__restrict__ pr, uint32_t n,
                                                        uint64_t n_tiles,
                                                        unsigned long long *first)
{
    __shared__ uint64_t red[kBlock / 64];
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint64_t within;
        const uint32_t i = pair_of_tile(pr, n, tile, &within);
        const CmpView A = pr[i].a, B = pr[i].b;
        const uint64_t total = pr[i].n;
        const uint32_t channels = pr[i].channels, fmt = pr[i].fmt, ph = pr[i].phase;
        unsigned long long *slot = first + pr[i].slot;
        const uint64_t f0 = within * kTile; // the tile's first frame
        // a tile at or after a mismatch on record has nothing smaller to add
        const uint64_t seen = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint64_t best = kNone;
        if (f0 < seen) {
            const uint64_t s0 = f0 * channels;
            const uint64_t t1 = s0 + (uint64_t)kTile * channels, s1 = t1 < total ? t1 : total;
            switch (fmt) {
            case 0:
                best = ByPhase<ATG_PCM_S16, ATG_PCM_S16>::run(ph & 7u, A, B, s0, s1);
                break;
            case 1:
                best = ByPhase<ATG_PCM_S32, ATG_PCM_S16>::run(ph & 7u, A, B, s0, s1);
                break;
            case 2:
                best = ByPhase<ATG_PCM_S16, ATG_PCM_S32>::run(ph & 3u, A, B, s0, s1);
                break;
            default:
                best = ByPhase<ATG_PCM_S32, ATG_PCM_S32>::run(ph & 3u, A, B, s0, s1);
                break;
            }
            if (best != kNone)
                best /= channels;
        }
        // the usual tile has no mismatch and ends at this one barrier
        if (__syncthreads_or(best != kNone)) {
            best = wave_min_u64(best);
            if ((threadIdx.x & 63) == 0)
                red[threadIdx.x >> 6] = best;
            __syncthreads();
            if (threadIdx.x == 0) {
                for (uint32_t w = 1; w < kBlock / 64; ++w)
                    best = red[w] < best ? red[w] : best;
                atomicMin(slot, (unsigned long long)best);
            }
        }
    }
}

// one lane per shift: bit j of a job's row says whether the probe equals B
// at shift j - K
__global__ __launch_bounds__(kBlock) void k_pcm_probe(const ProbeJob *__restrict__ jobs,
                                                      uint32_t K, uint32_t words,
                                                      unsigned long long *__restrict__ bits)
{
    const ProbeJob &J = jobs[blockIdx.y];
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    bool ok = j <= 2 * K;
    if (ok) {
        const long long k = (long long)j - (long long)K;
        const bool a32 = J.fmt & 1u, b32 = J.fmt & 2u;
        const long long ia = J.a.base + (long long)J.first;
        const long long ib = J.b.base + (long long)J.first + k * (long long)J.channels;
        for (uint32_t i = 0; i < J.n; ++i)
            if (sample_at(J.a, a32, ia + i) != sample_at(J.b, b32, ib + i)) {
                ok = false;
                break;
            }
    }
    const unsigned long long mask = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && (j >> 6) < words)
        bits[(uint64_t)blockIdx.y * words + (j >> 6)] = mask;
}

// ---------------------------------------------------------------- host side

atg_status check_view(const atg_pcm_view &v, uint32_t channels)
{
    if (!pcm_known_format(v.format))
        return g_pc_err.fail(ATG_ERR_INVALID, "unknown PCM format");
    if (v.src_frames && !v.d_pcm)
        return g_pc_err.fail(ATG_ERR_INVALID, "d_pcm is NULL with src_frames > 0");
    if (pcm_misaligned(v))
        return g_pc_err.fail(ATG_ERR_INVALID, "d_pcm is not aligned to its sample size");
    if (v.src_frames > (kLimit - 1) / channels)
        return g_pc_err.fail(ATG_ERR_INVALID, "src_frames * channels is 2^62 or more");
    if (v.src_frames && (v.sample_offset >= kLimit ||
                         v.sample_offset + v.src_frames * channels >= kLimit))
        return g_pc_err.fail(ATG_ERR_INVALID, "the source ends at sample 2^62 or beyond");
    if (v.window_offset >= (long long)kLimit || v.window_offset <= -(long long)kLimit)
        return g_pc_err.fail(ATG_ERR_INVALID, "window_offset is 2^62 or more in size");
    return ATG_OK;
}

atg_status check_args(const atg_pcm_pair *pairs, uint32_t n, uint32_t max_offset,
                      const atg_pcm_cmp_result *results)
{
    if (n && (!pairs || !results))
        return g_pc_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (max_offset > kMaxOffset)
        return g_pc_err.fail(ATG_ERR_UNSUPPORTED, "max_offset above 65535");
    for (uint32_t i = 0; i < n; ++i) {
        const atg_pcm_pair &p = pairs[i];
        if (!p.channels)
            return g_pc_err.fail(ATG_ERR_INVALID, "channels must be > 0");
        if (p.channels > kMaxChannels)
            return g_pc_err.fail(ATG_ERR_UNSUPPORTED, "more than 8 channels");
        if (p.frames > (kLimit - 1) / p.channels)
            return g_pc_err.fail(ATG_ERR_INVALID, "frames * channels is 2^62 or more");
        atg_status st = check_view(p.a, p.channels);
        if (st == ATG_OK)
            st = check_view(p.b, p.channels);
        if (st != ATG_OK)
            return st;
    }
    return ATG_OK;
}

// The view shifted by `shift` frames, for `frames` frames.  A view that never
// meets its source becomes an empty one, so that every index stays small.
CmpView plan_view(const atg_pcm_view &v, long long shift, uint64_t frames, uint32_t channels)
{
    CmpView o = {nullptr, 0, 0, 0};
    const long long wo = v.window_offset + shift;
    if (!v.src_frames || wo >= (long long)v.src_frames || wo + (long long)frames <= 0)
        return o;
    const PcmSplit src = pcm_split(v);
    o.p = src.p;
    o.lo = (long long)src.lo;
    o.hi = o.lo + (long long)(v.src_frames * channels);
    o.base = o.lo + wo * (long long)channels;
    return o;
}

uint32_t pair_fmt(const atg_pcm_pair &p)
{
    return (p.a.format == ATG_PCM_S32 ? 1u : 0u) | (p.b.format == ATG_PCM_S32 ? 2u : 0u);
}

CmpPair plan_pair(const atg_pcm_pair &p, long long shift_b, uint32_t slot)
{
    CmpPair c = {};
    c.a = plan_view(p.a, 0, p.frames, p.channels);
    c.b = plan_view(p.b, shift_b, p.frames, p.channels);
    c.n = p.frames * p.channels;
    c.channels = p.channels;
    c.fmt = pair_fmt(p);
    c.slot = slot;
    c.phase = (uint32_t)(c.b.base - c.a.base) & 7u;
    return c;
}

// the batch's first PCM pointer: its device is where the batch runs
const void *first_pcm(const atg_pcm_pair *pairs, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i) {
        if (pairs[i].a.src_frames)
            return pairs[i].a.d_pcm;
        if (pairs[i].b.src_frames)
            return pairs[i].b.d_pcm;
    }
    return nullptr;
}

// One compare launch: tab's pairs (each with frames > 0) into n_slots minima.
atg_status run_compare(CmpCtx &c, std::vector<CmpPair> &tab, uint32_t n_slots,
                       std::vector<uint64_t> &out, hipStream_t s)
{
    out.assign(n_slots, kNone);
    if (tab.empty())
        return ATG_OK;
    uint64_t n_tiles = tab.size(); // every pair's first tile, then the others
    for (CmpPair &p : tab) {
        p.rest0 = n_tiles - tab.size();
        n_tiles += (p.n / p.channels + kTile - 1) / kTile - 1;
    }
    CHIP(c.first.ensure(sizeof(uint64_t) * n_slots));
    CHIP(hipMemsetAsync(c.first.p, 0xFF, sizeof(uint64_t) * n_slots, s));
    const dim3 grid((uint32_t)std::min<uint64_t>(n_tiles, kMaxBlocks));
    const auto launch = [&](const CmpPair *d_pairs) {
        hipLaunchKernelGGL(k_pcm_compare, grid, dim3(kBlock), 0, s, d_pairs, (uint32_t)tab.size(),
                           n_tiles, (unsigned long long *)c.first.p);
    };
    const auto fetch = [&] {
        return hipMemcpyAsync(out.data(), c.first.p, sizeof(uint64_t) * n_slots,
                              hipMemcpyDeviceToHost, s);
    };
    float ms = 0.f;
    const atg_status st = timed_launch(c.pairs, c.ev, tab, s, g_pc_err, &ms, launch, fetch);
    if (st == ATG_OK && ms >= 0.f)
        g_pc_times.ms[0] += ms;
    return st;
}

// the r-th shift in order of |k|, +k before -k: 0, 1, -1, 2, -2, ...
long long shift_of_rank(uint32_t r) { return r & 1u ? (long long)((r + 1) / 2) : -(long long)(r / 2); }

atg_status search(const atg_pcm_pair *pairs, uint32_t n, uint32_t K, atg_pcm_cmp_result *results,
                  CmpCtx &c, hipStream_t s)
{
    // launch 1: A against nothing (its first non-silent frame), A against B
    std::vector<uint32_t> live; // pairs with frames > 0
    std::vector<CmpPair> tab;
    for (uint32_t i = 0; i < n; ++i) {
        if (!pairs[i].frames)
            continue;
        const uint32_t j = (uint32_t)live.size();
        atg_pcm_pair alone = pairs[i];
        alone.b.src_frames = 0;
        tab.push_back(plan_pair(alone, 0, 2 * j));
        tab.push_back(plan_pair(pairs[i], 0, 2 * j + 1));
        live.push_back(i);
    }
    std::vector<uint64_t> out;
    atg_status st = run_compare(c, tab, 2 * (uint32_t)live.size(), out, s);
    if (st != ATG_OK)
        return st;
    struct Open {
        uint32_t pair;
        uint64_t loud; // first non-silent frame of A, or kNone
        uint32_t rank; // next shift to look at, in order of |k|
    };
    std::vector<Open> open;
    for (uint32_t j = 0; j < live.size(); ++j) {
        atg_pcm_cmp_result &r = results[live[j]];
        r.first_mismatch = out[2 * j + 1];
        r.offset_found = r.first_mismatch == kNone;
        if (!r.offset_found && K)
            open.push_back({live[j], out[2 * j], 1});
    }
    if (open.empty())
        return ATG_OK;

    // the probe: which shifts are candidates, a row of bits per open pair
    const uint32_t width = 2 * K + 1, words = (width + 63) / 64;
    std::vector<uint64_t> bits((size_t)open.size() * words, ~0ull);
    std::vector<ProbeJob> jobs;
    std::vector<uint32_t> job_of(open.size(), UINT32_MAX);
    for (uint32_t o = 0; o < open.size(); ++o) {
        if (open[o].loud == kNone)
            continue; // wholly silent: every shift stays a candidate
        const atg_pcm_pair &p = pairs[open[o].pair];
        // B's window over every shift of the probe
        atg_pcm_view wide = p.b;
        wide.window_offset -= (long long)K;
        ProbeJob J = {};
        J.a = plan_view(p.a, 0, p.frames, p.channels);
        J.b = plan_view(wide, 0, p.frames + 2ull * K, p.channels);
        if (J.b.p)
            J.b.base += (long long)K * p.channels; // back to shift 0
        J.first = open[o].loud * p.channels;
        J.n = (uint32_t)(std::min<uint64_t>(kProbe, p.frames - open[o].loud) * p.channels);
        J.channels = p.channels;
        J.fmt = pair_fmt(p);
        job_of[o] = (uint32_t)jobs.size();
        jobs.push_back(J);
    }
    if (!jobs.empty()) {
        std::vector<uint64_t> got((size_t)jobs.size() * words);
        CHIP(c.bits.ensure(sizeof(uint64_t) * got.size()));
        const auto launch = [&](const ProbeJob *d_jobs) {
            for (size_t j0 = 0; j0 < jobs.size(); j0 += 65535) {
                const uint32_t nj = (uint32_t)std::min<size_t>(65535, jobs.size() - j0);
                hipLaunchKernelGGL(k_pcm_probe, dim3((width + kBlock - 1) / kBlock, nj),
                                   dim3(kBlock), 0, s, d_jobs + j0, K, words,
                                   (unsigned long long *)c.bits.p + j0 * words);
            }
        };
        const auto fetch = [&] {
            return hipMemcpyAsync(got.data(), c.bits.p, sizeof(uint64_t) * got.size(),
                                  hipMemcpyDeviceToHost, s);
        };
        float ms = 0.f;
        if ((st = timed_launch(c.jobs, c.ev, jobs, s, g_pc_err, &ms, launch, fetch)) != ATG_OK)
            return st;
        if (ms >= 0.f)
            g_pc_times.ms[1] += ms;
        for (uint32_t o = 0; o < open.size(); ++o)
            if (job_of[o] != UINT32_MAX)
                std::copy(got.begin() + (size_t)job_of[o] * words,
                          got.begin() + (size_t)(job_of[o] + 1) * words,
                          bits.begin() + (size_t)o * words);
    }

    // verification, in order of |k|; every launch moves each open pair on by
    // at least one shift, so there are at most 2K launches
    struct Try {
        uint32_t open;
        int32_t shift;
    };
    for (uint32_t round = 0; round < width && !open.empty(); ++round) {
        const uint32_t chunk = std::max<uint32_t>(
            1, std::min<uint32_t>(kVerifyChunk, kVerifyPairs / (uint32_t)open.size()));
        std::vector<Try> tries;
        tab.clear();
        for (uint32_t o = 0; o < open.size(); ++o) {
            uint32_t taken = 0;
            while (taken < chunk && open[o].rank < width) {
                const long long k = shift_of_rank(open[o].rank++);
                const uint32_t bit = (uint32_t)(k + (long long)K);
                if (!(bits[(size_t)o * words + (bit >> 6)] >> (bit & 63) & 1u))
                    continue;
                tab.push_back(plan_pair(pairs[open[o].pair], k, (uint32_t)tries.size()));
                tries.push_back({o, (int32_t)k});
                ++taken;
            }
        }
        st = run_compare(c, tab, (uint32_t)tries.size(), out, s);
        if (st != ATG_OK)
            return st;
        std::vector<bool> done(open.size(), false);
        for (uint32_t t = 0; t < tries.size(); ++t) {
            const uint32_t o = tries[t].open;
            if (done[o] || out[t] != kNone)
                continue;
            done[o] = true; // the first in order that passes
            results[open[o].pair].offset = tries[t].shift;
            results[open[o].pair].offset_found = 1;
        }
        // what stays open: not found yet and shifts left; the rows of bits follow
        uint32_t keep = 0;
        for (uint32_t o = 0; o < open.size(); ++o) {
            if (done[o] || open[o].rank >= width)
                continue;
            if (keep != o) {
                open[keep] = open[o];
                std::copy(bits.begin() + (size_t)o * words,
                          bits.begin() + (size_t)(o + 1) * words,
                          bits.begin() + (size_t)keep * words);
            }
            ++keep;
        }
        open.resize(keep);
    }
    return ATG_OK;
}

atg_status run(const atg_pcm_pair *pairs, uint32_t n, uint32_t max_offset, bool want_offset,
               atg_pcm_cmp_result *results, void *stream)
{
    atg_status st = check_args(pairs, n, max_offset, results);
    if (st != ATG_OK)
        return st;
    bool any = false;
    for (uint32_t i = 0; i < n; ++i) {
        results[i].first_mismatch = kNone;
        results[i].offset = 0;
        results[i].offset_found = want_offset ? 1u : 0u;
        any = any || pairs[i].frames;
    }
    if (!any)
        return ATG_OK;
    hipStream_t s = (hipStream_t)stream;
    DeviceContexts<CmpCtx>::Held held;
    if ((st = g_ctxs.hold(first_pcm(pairs, n), g_pc_err, held)) != ATG_OK)
        return st;
    CmpCtx &c = *held;
    g_pc_times = {{0.f, 0.f}, 2};
    if (want_offset)
        return search(pairs, n, max_offset, results, c, s);
    std::vector<CmpPair> tab;
    for (uint32_t i = 0; i < n; ++i)
        if (pairs[i].frames)
            tab.push_back(plan_pair(pairs[i], 0, i));
    std::vector<uint64_t> out;
    st = run_compare(c, tab, n, out, s);
    if (st != ATG_OK)
        return st;
    for (uint32_t i = 0; i < n; ++i)
        results[i].first_mismatch = out[i];
    return ATG_OK;
}

} // namespace

extern "C" {

const char *atg_pcm_compare_last_error(void) { return g_pc_err.msg.c_str(); }

atg_status atg_pcm_compare_device(const atg_pcm_pair *pairs, uint32_t n_pairs,
                                  atg_pcm_cmp_result *results, void *stream)
{
    return run(pairs, n_pairs, 0, false, results, stream);
}

atg_status atg_pcm_offset_search_device(const atg_pcm_pair *pairs, uint32_t n_pairs,
                                        uint32_t max_offset, atg_pcm_cmp_result *results,
                                        void *stream)
{
    return run(pairs, n_pairs, max_offset, true, results, stream);
}

uint32_t atg_pcm_compare_tile_frames(void) { return kTile; }

int atg_pcm_compare_kernel_times(const char **names, float *ms, int cap)
{
    return copy_times(kStageNames, g_pc_times.ms, g_pc_times.n, names, ms, cap);
}

} // extern "C"
