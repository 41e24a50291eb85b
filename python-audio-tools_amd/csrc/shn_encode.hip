// shn_encode.hip — Shorten (.shn) encoder for a batch of tracks.
//
// Replaces the body of the reference's audiotools.encoders.encode_shn
// (src/encoders/shn.c: encode_audio :178-294, calculate_best_diff :334-445).
// A .shn file is one MSB-first bit stream; the host writes each track's
// prefix (magic, header, the header VERBATIM) and trailer (footer VERBATIM,
// QUIT, padding), the device the audio commands between them.
//
// One unit is one (block, channel).  Nothing chains from unit to unit: the
// three samples a block's deltas reach back to are recomputed from the block
// before it (shifted by that block's own wasted bits), and the only state the
// reference carries across units, the shift of the last non-zero unit, is a
// segmented look-back done by a scan.
//
//   k_shn_size   one wave per unit: unsigned adjust, the all-zero test and
//                the wasted bits (one OR over the block), the three delta
//                sums, the DIFF choice, the energy and the code lengths.
//   k_shn_scan   one workgroup per track: "shift of the last non-zero unit
//                before me" (a BITSHIFT command where it differs) and the
//                exclusive sum of the units' bit lengths.
//   (host)       the tracks' byte extents; capacity is checked here and
//                ATG_ERR_CAPACITY reports the size needed.
//   k_shn_pack   one wave per unit: the commands and the residual codes
//                OR-ed into the zeroed output at the unit's bit offset (a
//                code's zero run needs no write at all).
//   k_shn_edges  the host's prefix and trailer bytes OR-ed in; they share
//                their last and first byte with the device's codes.
#include "handle_lock.h"
#include "host_common.h"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/atgpu.h"
#include "shn_common.h"
#include "table_search.h"
#include "wave.h"

namespace {

struct ETrack {
    uint64_t pcm_offset, pcm_frames;
    uint64_t unit0;    // first unit of the track in the batch
    uint64_t ends;     // index of the track's block ends in `ends`, or ~0
    uint64_t out_bit0; // bit of the output at which the audio commands start
    uint32_t n_blocks, pad;
};

struct Geom {
    uint64_t start;
    uint32_t n;
};

__device__ __forceinline__ Geom block_geom(const ETrack &T, const uint64_t *__restrict__ ends,
                                           uint32_t bs, uint64_t b)
{
    Geom g;
    if (T.ends != ~0ull) {
        const uint64_t *e = ends + T.ends;
        g.start = b ? e[b - 1] : 0;
        g.n = (uint32_t)(e[b] - g.start);
    } else {
        g.start = b * bs;
        g.n = (uint32_t)min((uint64_t)bs, T.pcm_frames - g.start);
    }
    return g;
}

// the track of unit u: the last t with unit0[t] <= u
__device__ __forceinline__ uint32_t find_track(const ETrack *__restrict__ tr, uint32_t n,
                                               uint64_t u)
{
    return last_le(tr, n, u, &ETrack::unit0);
}

// info word of a unit
constexpr uint32_t kZero = 1u;           // a ZERO command
constexpr uint32_t kShiftAt = 1;         // 5 bits
constexpr uint32_t kDiffAt = 6;          // 2 bits
constexpr uint32_t kEnergyAt = 8;        // 6 bits
constexpr uint32_t kBitshift = 1u << 14; // a BITSHIFT command goes in front
constexpr uint32_t kBlocksize = 1u << 15; // a BLOCKSIZE command goes in front

template <typename T> struct Chan {
    const T *src; // the track's first sample of this channel
    uint32_t C;
    int32_t adjust;
    __device__ int32_t at(uint64_t frame) const { return (int32_t)src[frame * C] + adjust; }
};

template <typename T>
__device__ __forceinline__ uint32_t block_or(const Chan<T> &ch, Geom g, uint32_t lane)
{
    uint32_t acc = 0;
    for (uint32_t i = lane; i < g.n; i += 64u)
        acc |= (uint32_t)ch.at(g.start + i);
    return wave_or_u32(acc);
}

// What both kernels need of a unit: its shift and the three samples before
// it as the reference's wrapped history holds them.
template <typename T>
__device__ __forceinline__ void unit_history(const Chan<T> &ch, const ETrack &Tk,
                                             const uint64_t *__restrict__ ends, uint32_t bs,
                                             uint64_t b, uint32_t lane, int32_t h[3])
{
    h[0] = h[1] = h[2] = 0;
    uint32_t got = 0;
    for (uint64_t j = b; got < 3u && j-- > 0;) {
        const Geom gj = block_geom(Tk, ends, bs, j);
        const uint32_t orv = block_or(ch, gj, lane);
        const uint32_t sh = orv ? (uint32_t)__ffs((int)orv) - 1u : 0u;
        const uint32_t take = min(3u - got, gj.n);
        for (uint32_t k = 0; k < take; ++k)
            h[got + k] = ch.at(gj.start + gj.n - 1u - k) >> sh;
        got += take;
    }
}

template <typename T>
__device__ __forceinline__ int32_t sample_at(const Chan<T> &ch, Geom g, uint32_t sh,
                                             const int32_t h[3], int64_t i)
{
    if (i < 0)
        return h[-i - 1];
    return ch.at(g.start + (uint64_t)i) >> sh;
}

__device__ __forceinline__ uint32_t fold(int32_t r)
{
    return r >= 0 ? (uint32_t)r << 1 : ((0u - (uint32_t)r - 1u) << 1) + 1u;
}

template <typename T>
__global__ __launch_bounds__(256) void k_shn_size(const T *__restrict__ pcm,
                                                  const ETrack *__restrict__ tracks,
                                                  uint32_t n_tracks,
                                                  const uint64_t *__restrict__ ends,
                                                  uint64_t n_units, uint32_t C, uint32_t bs,
                                                  int32_t adjust, uint32_t *__restrict__ uinfo,
                                                  uint32_t *__restrict__ ubits)
{
    const uint64_t u = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (u >= n_units)
        return;
    const ETrack Tk = tracks[find_track(tracks, n_tracks, u)];
    const uint64_t b = (u - Tk.unit0) / C;
    const uint32_t c = (uint32_t)((u - Tk.unit0) % C);
    const Chan<T> ch{pcm + Tk.pcm_offset * C + c, C, adjust};
    const Geom g = block_geom(Tk, ends, bs, b);
    uint32_t info = 0, bits = 0;
    if (c == 0) {
        const uint32_t before = b ? block_geom(Tk, ends, bs, b - 1).n : bs;
        if (before != g.n) {
            info |= kBlocksize;
            bits += 4u + shn::long_bits(g.n);
        }
    }
    const uint32_t orv = block_or(ch, g, lane);
    if (!orv) {
        info |= kZero;
        bits += 5u; // unsigned(2) of 8
    } else {
        const uint32_t sh = (uint32_t)__ffs((int)orv) - 1u;
        int32_t h[3];
        unit_history(ch, Tk, ends, bs, b, lane, h);
        uint32_t s1 = 0, s2 = 0, s3 = 0;
        for (uint32_t i = lane; i < g.n; i += 64u) {
            const uint32_t x0 = (uint32_t)sample_at(ch, g, sh, h, (int64_t)i);
            const uint32_t x1 = (uint32_t)sample_at(ch, g, sh, h, (int64_t)i - 1);
            const uint32_t x2 = (uint32_t)sample_at(ch, g, sh, h, (int64_t)i - 2);
            const uint32_t x3 = (uint32_t)sample_at(ch, g, sh, h, (int64_t)i - 3);
            const int32_t d1 = (int32_t)(x0 - x1);
            const int32_t d2 = (int32_t)(x0 - 2u * x1 + x2);
            const int32_t d3 = (int32_t)(x0 - 3u * x1 + 3u * x2 - x3);
            s1 += (uint32_t)abs(d1);
            s2 += (uint32_t)abs(d2);
            s3 += (uint32_t)abs(d3);
        }
        s1 = wave_sum_u32(s1);
        s2 = wave_sum_u32(s2);
        s3 = wave_sum_u32(s3);
        uint32_t diff, sum;
        if (s1 < min(s2, s3)) {
            diff = 1;
            sum = s1;
        } else if (s2 < s3) {
            diff = 2;
            sum = s2;
        } else {
            diff = 3;
            sum = s3;
        }
        uint32_t energy = 0;
        // in range input ends this well below 31 (|delta3| < 2^19, n <= 4096)
        while (energy < 31u && (g.n << energy) < sum)
            ++energy;
        const uint32_t w = energy + 1u;
        uint32_t len = 0;
        for (uint32_t i = lane; i < g.n; i += 64u) {
            const uint32_t x0 = (uint32_t)sample_at(ch, g, sh, h, (int64_t)i);
            const uint32_t x1 = (uint32_t)sample_at(ch, g, sh, h, (int64_t)i - 1);
            uint32_t r = x0 - x1;
            if (diff >= 2u) {
                const uint32_t x2 = (uint32_t)sample_at(ch, g, sh, h, (int64_t)i - 2);
                r = x0 - 2u * x1 + x2;
                if (diff == 3u)
                    r = x0 - 3u * x1 + 3u * x2 - (uint32_t)sample_at(ch, g, sh, h, (int64_t)i - 3);
            }
            len += (fold((int32_t)r) >> w) + 1u + w;
        }
        len = wave_sum_u32(len);
        info |= (sh << kShiftAt) | ((diff & 3u) << kDiffAt) | (energy << kEnergyAt);
        bits += 3u + shn::unsigned_bits(shn::kEnergySize, energy) + len;
    }
    if (lane == 0) {
        uinfo[u] = info;
        ubits[u] = bits;
    }
}

// ------------------------------------------------------------------- scan
constexpr uint32_t kScanThreads = 256;

__global__ __launch_bounds__(256) void k_shn_scan(const ETrack *__restrict__ tracks, uint32_t C,
                                                  uint32_t *__restrict__ uinfo,
                                                  const uint32_t *__restrict__ ubits,
                                                  uint64_t *__restrict__ uoff,
                                                  uint64_t *__restrict__ track_bits)
{
    __shared__ uint32_t sh_s[kScanThreads];
    __shared__ uint64_t sh_b[kScanThreads];
    const ETrack Tk = tracks[blockIdx.x];
    const uint64_t nu = (uint64_t)Tk.n_blocks * C;
    const uint32_t tid = threadIdx.x;
    uint32_t carry_shift = 0; // the reference starts with left_shift = 0
    uint64_t carry_bits = 0;
    for (uint64_t base = 0; base < nu; base += kScanThreads) {
        const uint64_t u = base + tid;
        const bool valid = u < nu;
        const uint32_t info = valid ? uinfo[Tk.unit0 + u] : kZero;
        const uint32_t shift = (info >> kShiftAt) & 31u;
        // inclusive "last non-zero unit's shift, marked": ZERO units pass the
        // value on the left through
        sh_s[tid] = (info & kZero) ? 0u : (shift | 0x80u);
        __syncthreads();
        for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
            const uint32_t mine = sh_s[tid];
            const uint32_t left = tid >= d ? sh_s[tid - d] : 0u;
            __syncthreads();
            sh_s[tid] = mine ? mine : left;
            __syncthreads();
        }
        const uint32_t before = tid ? sh_s[tid - 1] : 0u;
        const uint32_t prev_shift = before ? (before & 31u) : carry_shift;
        const uint32_t last = sh_s[kScanThreads - 1];
        uint64_t bits = valid ? ubits[Tk.unit0 + u] : 0u;
        const bool cmd = valid && !(info & kZero) && shift != prev_shift;
        if (cmd)
            bits += 4u + shn::unsigned_bits(shn::kShiftSize, shift);
        sh_b[tid] = bits;
        __syncthreads();
        for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
            const uint64_t mine = sh_b[tid];
            const uint64_t left = tid >= d ? sh_b[tid - d] : 0u;
            __syncthreads();
            sh_b[tid] = mine + left;
            __syncthreads();
        }
        if (valid) {
            uoff[Tk.unit0 + u] = carry_bits + sh_b[tid] - bits;
            if (cmd)
                uinfo[Tk.unit0 + u] = info | kBitshift;
        }
        const uint64_t total = sh_b[kScanThreads - 1];
        __syncthreads();
        carry_bits += total;
        if (last)
            carry_shift = last & 31u;
    }
    if (tid == 0)
        track_bits[blockIdx.x] = carry_bits;
}

// ------------------------------------------------------------------- pack
template <typename T>
__global__ __launch_bounds__(256) void k_shn_pack(const T *__restrict__ pcm,
                                                  const ETrack *__restrict__ tracks,
                                                  uint32_t n_tracks,
                                                  const uint64_t *__restrict__ ends,
                                                  uint64_t n_units, uint32_t C, uint32_t bs,
                                                  int32_t adjust,
                                                  const uint32_t *__restrict__ uinfo,
                                                  const uint64_t *__restrict__ uoff,
                                                  uint32_t *__restrict__ out)
{
    const uint64_t u = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (u >= n_units)
        return;
    const ETrack Tk = tracks[find_track(tracks, n_tracks, u)];
    const uint64_t b = (u - Tk.unit0) / C;
    const uint32_t c = (uint32_t)((u - Tk.unit0) % C);
    const Chan<T> ch{pcm + Tk.pcm_offset * C + c, C, adjust};
    const Geom g = block_geom(Tk, ends, bs, b);
    const uint32_t info = uinfo[u];
    uint64_t pos = Tk.out_bit0 + uoff[u];
    // the commands: every lane keeps the position, lane 0 writes
    const bool w0 = lane == 0;
    if (info & kBlocksize) {
        if (w0) {
            (void)shn::put_unsigned(out, pos, shn::kCommandSize, shn::FN_BLOCKSIZE);
            (void)shn::put_long(out, pos + 4u, g.n);
        }
        pos += 4u + shn::long_bits(g.n);
    }
    if (info & kZero) {
        if (w0)
            (void)shn::put_unsigned(out, pos, shn::kCommandSize, shn::FN_ZERO);
        return;
    }
    const uint32_t sh = (info >> kShiftAt) & 31u;
    const uint32_t diff = (info >> kDiffAt) & 3u;
    const uint32_t energy = (info >> kEnergyAt) & 63u;
    if (info & kBitshift) {
        if (w0) {
            (void)shn::put_unsigned(out, pos, shn::kCommandSize, shn::FN_BITSHIFT);
            (void)shn::put_unsigned(out, pos + 4u, shn::kShiftSize, sh);
        }
        pos += 4u + shn::unsigned_bits(shn::kShiftSize, sh);
    }
    if (w0) {
        (void)shn::put_unsigned(out, pos, shn::kCommandSize, diff);
        (void)shn::put_unsigned(out, pos + 3u, shn::kEnergySize, energy);
    }
    pos += 3u + shn::unsigned_bits(shn::kEnergySize, energy);
    int32_t h[3];
    unit_history(ch, Tk, ends, bs, b, lane, h);
    const uint32_t w = energy + 1u;
    for (uint32_t i0 = 0; i0 < g.n; i0 += 64u) {
        const uint32_t i = i0 + lane;
        uint32_t len = 0, f = 0;
        if (i < g.n) {
            const uint32_t x0 = (uint32_t)sample_at(ch, g, sh, h, (int64_t)i);
            const uint32_t x1 = (uint32_t)sample_at(ch, g, sh, h, (int64_t)i - 1);
            uint32_t r = x0 - x1;
            if (diff >= 2u) {
                const uint32_t x2 = (uint32_t)sample_at(ch, g, sh, h, (int64_t)i - 2);
                r = x0 - 2u * x1 + x2;
                if (diff == 3u)
                    r = x0 - 3u * x1 + 3u * x2 - (uint32_t)sample_at(ch, g, sh, h, (int64_t)i - 3);
            }
            f = fold((int32_t)r);
            len = (f >> w) + 1u + w;
        }
        // inclusive sum of the code lengths over the wave
        const uint32_t inc = wave_incl_scan_u32(len, (int)lane);
        if (i < g.n) {
            const uint64_t at = pos + (inc - len) + (f >> w); // past the zero run
            if (w < 32u) {
                shn::put_bits(out, at, (1u << w) | (f & ((1u << w) - 1u)), w + 1u);
            } else {
                shn::put_bits(out, at, 1u, 1u);
                shn::put_bits(out, at + 1u, f, 32u);
            }
        }
        pos += (uint32_t)__shfl((int)inc, 63, 64);
    }
}

// ------------------------------------------------------------------ edges
struct Frag {
    uint64_t dst; // byte of the output
    uint32_t src, len;
};

__global__ __launch_bounds__(64) void k_shn_edges(const Frag *__restrict__ frags,
                                                  const uint8_t *__restrict__ blob,
                                                  uint32_t *__restrict__ out)
{
    const Frag f = frags[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < f.len; i += 64u) {
        const uint32_t v = blob[f.src + i];
        const uint64_t d = f.dst + i;
        if (v)
            atomicOr(out + (d >> 2), v << (8u * ((uint32_t)d & 3u)));
    }
}

// ------------------------------------------------------------------- host
thread_local ErrSlot g_shn_err;
#define SHIP(expr) ATG_HIP_TRY(g_shn_err, expr, #expr)

// "shn_layout" is the host between the scan and the pack: the copy of the
// tracks' bit totals, the byte extents, the second upload of the track table,
// the prefix and trailer bytes and the clearing of the output
const int kSTimed = 6;
const char *kSNames[kSTimed] = {"shn_size",  "shn_scan", "shn_layout",
                                "shn_pack",  "shn_edges", "shn_total"};

} // namespace

struct atg_shn_encoder : StageHandle<kSTimed> {
    DevBuf tracks, ends, uinfo, ubits, uoff, track_bits, frags, blob, h_pcm, h_out;
};

namespace {

struct SPlan {
    std::vector<ETrack> tracks;
    std::vector<uint64_t> ends;
    std::vector<shn::HostBits> prefix;
    uint64_t units = 0;
};

atg_status shn_plan(const atg_track *tracks, const atg_shn_track_data *extra, uint32_t n,
                    uint32_t channels, uint32_t bps, const atg_shn_options &o, SPlan &P)
{
    if (bps != 8 && bps != 16)
        return g_shn_err.fail(ATG_ERR_INVALID, "unsupported bits per sample");
    if (channels < 1 || channels > ATG_SHN_MAX_CHANNELS)
        return g_shn_err.fail(ATG_ERR_INVALID, "channels out of range");
    if (o.block_size < 1)
        return g_shn_err.fail(ATG_ERR_INVALID, "block_size must be at least 1");
    if (o.block_size > ATG_SHN_MAX_ENCODE_BLOCK)
        return g_shn_err.fail(ATG_ERR_UNSUPPORTED, "block_size above ATG_SHN_MAX_ENCODE_BLOCK");
    uint32_t ftype;
    if (bps == 8)
        ftype = o.signed_samples ? 1 : 2;
    else if (o.signed_samples)
        ftype = o.is_big_endian ? 3 : 5;
    else
        ftype = o.is_big_endian ? 4 : 6;
    P.tracks.resize(n);
    P.prefix.resize(n);
    for (uint32_t t = 0; t < n; ++t) {
        const atg_track &T = tracks[t];
        ETrack &E = P.tracks[t];
        std::memset(&E, 0, sizeof(E));
        E.pcm_offset = T.pcm_offset;
        E.pcm_frames = T.pcm_frames;
        E.unit0 = P.units;
        E.ends = ~0ull;
        uint64_t nb;
        if (T.frame_sizes) {
            E.ends = P.ends.size();
            uint64_t pos = 0;
            for (uint64_t k = 0; k < T.n_frame_sizes; ++k) {
                const uint32_t len = T.frame_sizes[k];
                if (len < 1)
                    return g_shn_err.fail(ATG_ERR_INVALID, "frame sizes must be at least 1");
                if (len > ATG_SHN_MAX_ENCODE_BLOCK)
                    return g_shn_err.fail(ATG_ERR_UNSUPPORTED,
                                          "frame size above ATG_SHN_MAX_ENCODE_BLOCK");
                pos += len;
                P.ends.push_back(pos);
            }
            if (pos != T.pcm_frames)
                return g_shn_err.fail(ATG_ERR_INVALID, "frame sizes must sum to pcm_frames");
            nb = T.n_frame_sizes;
        } else {
            nb = (T.pcm_frames + o.block_size - 1) / o.block_size;
        }
        if (nb > 0x7FFFFFFFull / channels)
            return g_shn_err.fail(ATG_ERR_UNSUPPORTED, "too many Shorten blocks in one track");
        E.n_blocks = (uint32_t)nb;
        P.units += nb * channels;
        const atg_shn_track_data *X = extra ? &extra[t] : nullptr;
        if (X && ((X->header_bytes && !X->header) || (X->footer_bytes && !X->footer)))
            return g_shn_err.fail(ATG_ERR_INVALID, "NULL header or footer data");
        if (X && (X->header_bytes > 0x7FFFFFFFull || X->footer_bytes > 0x7FFFFFFFull))
            return g_shn_err.fail(ATG_ERR_UNSUPPORTED, "header or footer data too large");
        shn::HostBits &w = P.prefix[t];
        w.write(8, 'a');
        w.write(8, 'j');
        w.write(8, 'k');
        w.write(8, 'g');
        w.write(8, 2);
        w.lng(ftype);
        w.lng(channels);
        w.lng(o.block_size);
        w.lng(0); // maximum LPC
        w.lng(0); // mean count
        w.lng(0); // bytes to skip
        w.verbatim(X ? X->header : nullptr, X ? (uint32_t)X->header_bytes : 0u);
    }
    if (P.units > 0x7FFFFFFFull * 4u)
        return g_shn_err.fail(ATG_ERR_UNSUPPORTED, "too many Shorten blocks in one batch");
    return ATG_OK;
}

template <typename T>
atg_status shn_run(atg_shn_encoder *enc, SPlan &P, const atg_shn_track_data *extra,
                   const T *d_pcm, uint8_t *d_out, DevBuf *stage, uint64_t out_cap, uint32_t n,
                   uint32_t channels, uint32_t bps, const atg_shn_options &o,
                   atg_shn_track_result *res, uint64_t *needed, uint64_t *out_bytes)
{
    hipStream_t s = enc->s;
    const uint64_t nu = P.units;
    const int32_t adjust = o.signed_samples ? 0 : (int32_t)(1u << (bps - 1));
    SHIP(enc->tracks.ensure(sizeof(ETrack) * std::max<uint64_t>(n, 1)));
    SHIP(enc->ends.ensure(sizeof(uint64_t) * std::max<uint64_t>(P.ends.size(), 1)));
    SHIP(enc->uinfo.ensure(sizeof(uint32_t) * std::max<uint64_t>(nu, 1)));
    SHIP(enc->ubits.ensure(sizeof(uint32_t) * std::max<uint64_t>(nu, 1)));
    SHIP(enc->uoff.ensure(sizeof(uint64_t) * std::max<uint64_t>(nu, 1)));
    SHIP(enc->track_bits.ensure(sizeof(uint64_t) * std::max<uint64_t>(n, 1)));
    if (n)
        SHIP(hipMemcpyAsync(enc->tracks.p, P.tracks.data(), sizeof(ETrack) * n,
                            hipMemcpyHostToDevice, s));
    if (!P.ends.empty())
        SHIP(hipMemcpyAsync(enc->ends.p, P.ends.data(), sizeof(uint64_t) * P.ends.size(),
                            hipMemcpyHostToDevice, s));
    const unsigned ublocks = (unsigned)((nu + 3) / 4);
    SHIP(hipEventRecord(enc->ev[0], s));
    if (nu)
        hipLaunchKernelGGL(k_shn_size<T>, dim3(ublocks), dim3(256), 0, s, d_pcm,
                           (const ETrack *)enc->tracks.p, n, (const uint64_t *)enc->ends.p, nu,
                           channels, o.block_size, adjust, (uint32_t *)enc->uinfo.p,
                           (uint32_t *)enc->ubits.p);
    SHIP(hipGetLastError());
    SHIP(hipEventRecord(enc->ev[1], s));
    if (n)
        hipLaunchKernelGGL(k_shn_scan, dim3(n), dim3(kScanThreads), 0, s,
                           (const ETrack *)enc->tracks.p, channels, (uint32_t *)enc->uinfo.p,
                           (const uint32_t *)enc->ubits.p, (uint64_t *)enc->uoff.p,
                           (uint64_t *)enc->track_bits.p);
    SHIP(hipGetLastError());
    SHIP(hipEventRecord(enc->ev[2], s));
    std::vector<uint64_t> h_bits(n, 0);
    if (n)
        SHIP(hipMemcpyAsync(h_bits.data(), enc->track_bits.p, sizeof(uint64_t) * n,
                            hipMemcpyDeviceToHost, s));
    SHIP(hipStreamSynchronize(s));
    // the extents: whole images, each at a 4-byte aligned offset
    std::vector<Frag> frags;
    std::vector<uint8_t> blob;
    uint64_t pos = 0;
    for (uint32_t t = 0; t < n; ++t) {
        atg_shn_track_result &r = res[t];
        const shn::HostBits &pre = P.prefix[t];
        pos = (pos + 3) & ~3ull;
        const uint64_t end_bit = pre.nbits + h_bits[t];
        // the trailer starts in the byte the audio commands end in
        shn::HostBits tail;
        tail.zeros(end_bit & 7u);
        const atg_shn_track_data *X = extra ? &extra[t] : nullptr;
        if (X && X->footer_bytes)
            tail.verbatim(X->footer, (uint32_t)X->footer_bytes);
        tail.uns(shn::kCommandSize, shn::FN_QUIT);
        uint64_t bytes = (end_bit >> 3) + tail.bytes.size();
        while ((bytes - 5u) % 4u) {
            tail.bytes.push_back(0);
            ++bytes;
        }
        r.out_offset = pos;
        r.bytes = bytes;
        r.pcm_frames = P.tracks[t].pcm_frames;
        r.n_blocks = P.tracks[t].n_blocks;
        r.reserved = 0;
        P.tracks[t].out_bit0 = pos * 8u + pre.nbits;
        if (blob.size() + pre.bytes.size() + tail.bytes.size() > 0xFFFFFFFFull)
            return g_shn_err.fail(ATG_ERR_UNSUPPORTED, "header and footer data too large");
        frags.push_back(Frag{pos, (uint32_t)blob.size(), (uint32_t)pre.bytes.size()});
        blob.insert(blob.end(), pre.bytes.begin(), pre.bytes.end());
        frags.push_back(Frag{pos + (end_bit >> 3), (uint32_t)blob.size(),
                             (uint32_t)tail.bytes.size()});
        blob.insert(blob.end(), tail.bytes.begin(), tail.bytes.end());
        pos += bytes;
    }
    // the kernels write whole 32-bit words
    const uint64_t total = (pos + 3) & ~3ull;
    if (needed)
        *needed = total;
    if (out_bytes)
        *out_bytes = total;
    if (total > out_cap)
        return g_shn_err.fail(ATG_ERR_CAPACITY, "output buffer smaller than the encoded batch");
    if (stage) {
        SHIP(stage->ensure(std::max<uint64_t>(total, 4)));
        d_out = (uint8_t *)stage->p;
    }
    SHIP(enc->frags.ensure(sizeof(Frag) * std::max<uint64_t>(frags.size(), 1)));
    SHIP(enc->blob.ensure(std::max<uint64_t>(blob.size(), 1)));
    if (n) {
        SHIP(hipMemcpyAsync(enc->tracks.p, P.tracks.data(), sizeof(ETrack) * n,
                            hipMemcpyHostToDevice, s));
        SHIP(hipMemcpyAsync(enc->frags.p, frags.data(), sizeof(Frag) * frags.size(),
                            hipMemcpyHostToDevice, s));
        SHIP(hipMemcpyAsync(enc->blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
    }
    if (total)
        SHIP(hipMemsetAsync(d_out, 0, total, s));
    SHIP(hipEventRecord(enc->ev[3], s));
    if (nu)
        hipLaunchKernelGGL(k_shn_pack<T>, dim3(ublocks), dim3(256), 0, s, d_pcm,
                           (const ETrack *)enc->tracks.p, n, (const uint64_t *)enc->ends.p, nu,
                           channels, o.block_size, adjust, (const uint32_t *)enc->uinfo.p,
                           (const uint64_t *)enc->uoff.p, (uint32_t *)d_out);
    SHIP(hipGetLastError());
    SHIP(hipEventRecord(enc->ev[4], s));
    if (!frags.empty())
        hipLaunchKernelGGL(k_shn_edges, dim3((unsigned)frags.size()), dim3(64), 0, s,
                           (const Frag *)enc->frags.p, (const uint8_t *)enc->blob.p,
                           (uint32_t *)d_out);
    SHIP(hipGetLastError());
    SHIP(hipEventRecord(enc->ev[5], s));
    SHIP(hipStreamSynchronize(s));
    enc->finish_times();
    return ATG_OK;
}

atg_status shn_check(atg_shn_encoder *e, const atg_track *tracks, uint32_t n,
                     atg_shn_track_result *results, const atg_shn_options *o, atg_pcm_format fmt)
{
    if (!e || !o || (!tracks && n) || (!results && n))
        return g_shn_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (fmt != ATG_PCM_S16 && fmt != ATG_PCM_S32)
        return g_shn_err.fail(ATG_ERR_INVALID, "unknown PCM format");
    return ATG_OK;
}

} // namespace

extern "C" {

const char *atg_shn_encoder_last_error(void) { return g_shn_err.msg.c_str(); }

atg_status atg_shn_encoder_create(int device, atg_shn_encoder **out)
{
    return open_handle(device, out, g_shn_err, "encoder create");
}

void atg_shn_encoder_destroy(atg_shn_encoder *e)
{
    if (!e)
        return;
    e->close({&e->tracks, &e->ends, &e->uinfo, &e->ubits, &e->uoff, &e->track_bits, &e->frags,
              &e->blob, &e->h_pcm, &e->h_out});
    delete e;
}

atg_status atg_shn_encode_device(atg_shn_encoder *e, const void *d_pcm, atg_pcm_format fmt,
                                 const atg_track *tracks, const atg_shn_track_data *extra,
                                 uint32_t n, uint32_t channels, uint32_t bps,
                                 const atg_shn_options *options, void *d_out, uint64_t out_cap,
                                 atg_shn_track_result *results, uint64_t *needed)
{
    ATG_HANDLE_LOCK(e);
    atg_status st = shn_check(e, tracks, n, results, options, fmt);
    if (st != ATG_OK)
        return st;
    if (((uintptr_t)d_out) & 3)
        return g_shn_err.fail(ATG_ERR_INVALID, "d_out must be 4-byte aligned");
    SHIP(hipSetDevice(e->device));
    SPlan P;
    st = shn_plan(tracks, extra, n, channels, bps, *options, P);
    if (st != ATG_OK)
        return st;
    if (fmt == ATG_PCM_S16)
        return shn_run(e, P, extra, (const int16_t *)d_pcm, (uint8_t *)d_out, nullptr, out_cap, n,
                       channels, bps, *options, results, needed, nullptr);
    return shn_run(e, P, extra, (const int32_t *)d_pcm, (uint8_t *)d_out, nullptr, out_cap, n,
                   channels, bps, *options, results, needed, nullptr);
}

atg_status atg_shn_encode_host(atg_shn_encoder *e, const void *pcm, atg_pcm_format fmt,
                               const atg_track *tracks, const atg_shn_track_data *extra,
                               uint32_t n, uint32_t channels, uint32_t bps,
                               const atg_shn_options *options, uint8_t *out, uint64_t out_cap,
                               atg_shn_track_result *results, uint64_t *needed)
{
    ATG_HANDLE_LOCK(e);
    atg_status st = shn_check(e, tracks, n, results, options, fmt);
    if (st != ATG_OK)
        return st;
    SHIP(hipSetDevice(e->device));
    SPlan P;
    st = shn_plan(tracks, extra, n, channels, bps, *options, P);
    if (st != ATG_OK)
        return st;
    uint64_t frames = 0;
    for (uint32_t t = 0; t < n; ++t)
        frames = std::max<uint64_t>(frames, tracks[t].pcm_offset + tracks[t].pcm_frames);
    if ((!pcm && frames) || (!out && n))
        return g_shn_err.fail(ATG_ERR_INVALID, "NULL argument");
    const size_t es = fmt == ATG_PCM_S16 ? 2 : 4;
    const uint64_t in_bytes = frames * channels * es;
    SHIP(e->h_pcm.ensure(std::max<uint64_t>(in_bytes, 4)));
    if (in_bytes)
        SHIP(hipMemcpyAsync(e->h_pcm.p, pcm, in_bytes, hipMemcpyHostToDevice, e->s));
    uint64_t total = 0;
    st = fmt == ATG_PCM_S16
             ? shn_run(e, P, extra, (const int16_t *)e->h_pcm.p, nullptr, &e->h_out, out_cap, n,
                       channels, bps, *options, results, needed, &total)
             : shn_run(e, P, extra, (const int32_t *)e->h_pcm.p, nullptr, &e->h_out, out_cap, n,
                       channels, bps, *options, results, needed, &total);
    if (st != ATG_OK)
        return st;
    if (total)
        SHIP(hipMemcpyAsync(out, e->h_out.p, total, hipMemcpyDeviceToHost, e->s));
    SHIP(hipStreamSynchronize(e->s));
    return ATG_OK;
}

int atg_shn_encoder_kernel_times(atg_shn_encoder *e, const char **names, float *ms, int cap)
{
    ATG_HANDLE_LOCK(e);
    return e ? e->report(kSNames, names, ms, cap) : 0;
}

} // extern "C"
