// tta_encode.hip — True Audio (TTA1) frame encoder for a batch of tracks.
//
// Replaces the body of the reference's audiotools.encoders.encode_tta
// (src/encoders/tta.c: encode_frame :144-259, correlate_channels :261-287,
// fixed_prediction :289-305, hybrid_filter :307-383): every read of
// block_size = sample_rate 256 / 245 PCM frames becomes one TTA frame, the
// Rice payload byte-aligned and followed by its CRC-32.  The output holds
// frames only; header and seektable are host work (audiotools/tta.py).
//
// Every TTA frame resets the filter and the Rice state, so frames are
// independent; inside a frame each channel is a serial chain.
//
//   k_tta_chain   one lane per (frame, channel): correlate + fixed
//                 prediction fused into the load, the hybrid filter and the
//                 Rice state walk, all state in registers.  Per sample it
//                 stores the channel's running code length (bits) and the
//                 code's binary tail with a marker bit above it; the unary
//                 run is the difference of two running lengths minus the
//                 tail, so a run of any length is representable.
//   (host)        frame sizes = sum of the channels' totals: the tracks'
//                 byte extents are known before a single output byte is
//                 written.  A frame has no useful a-priori bound (a
//                 full-scale sample after a quiet passage costs a unary run
//                 as long as its value), so capacity is checked here and
//                 ATG_ERR_CAPACITY reports the size needed.
//   k_tta_pack    one lane per sample in interleaved order: its bit offset
//                 is the sum of the channels' running lengths up to it;
//                 the code is OR-ed into the zeroed output (whole words of
//                 a long run are plain stores).
//   k_tta_crc     one workgroup per frame: CRC-32 over the payload in 256
//                 pieces combined by polynomial arithmetic (tta_common.h).
#include "handle_lock.h"
#include "host_common.h"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/atgpu.h"
#include "tta_common.h"

namespace {

using tta::Frame;

// ------------------------------------------------------------------ chain
// channel c of the correlated signal at PCM frame i (tta.c:261-287)
template <typename T>
__device__ __forceinline__ int32_t tta_correlated(const T *__restrict__ src, uint64_t i,
                                                  uint32_t C, uint32_t c)
{
    if (C == 1)
        return (int32_t)src[i];
    const T *f = src + i * C;
    if (c + 1 < C)
        return (int32_t)((uint32_t)(int32_t)f[c + 1] - (uint32_t)(int32_t)f[c]);
    const int32_t prev = (int32_t)((uint32_t)(int32_t)f[C - 1] - (uint32_t)(int32_t)f[C - 2]);
    return (int32_t)((uint32_t)(int32_t)f[C - 1] - (uint32_t)(prev / 2)); // truncating
}

constexpr uint32_t kLoadAhead = 8;

template <typename T>
__global__ __launch_bounds__(64) void k_tta_chain(const T *__restrict__ pcm,
                                                  const Frame *__restrict__ frames,
                                                  const uint32_t *__restrict__ chain_frame,
                                                  uint64_t n_chains, uint32_t *__restrict__ pre,
                                                  uint32_t *__restrict__ tail,
                                                  uint64_t *__restrict__ chain_bits)
{
    const uint64_t g = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (g >= n_chains)
        return;
    const Frame fr = frames[chain_frame[g]];
    const uint32_t C = fr.channels;
    const uint32_t c = (uint32_t)(g - fr.chain0);
    const T *src = pcm + fr.pcm_start * C;
    uint32_t *mypre = pre + fr.sbase + (uint64_t)c * fr.n;
    uint32_t *mytail = tail + fr.sbase + (uint64_t)c * fr.n;
    tta::Hybrid h;
    h.reset();
    tta::Rice rs;
    uint64_t bits = 0;
    int32_t xprev = 0, rprev = 0;
    // kLoadAhead samples are loaded before the recurrence needs them: the
    // loads of a group are independent of the chain and overlap each other,
    // where a load per step puts a memory round trip into every step
    for (uint32_t i0 = 0; i0 < fr.n; i0 += kLoadAhead) {
        int32_t xs[kLoadAhead];
#pragma unroll
        for (uint32_t j = 0; j < kLoadAhead; ++j)
            xs[j] = i0 + j < fr.n ? tta_correlated(src, i0 + j, C, c) : 0;
#pragma unroll
        for (uint32_t j = 0; j < kLoadAhead; ++j) {
            const uint32_t i = i0 + j;
            if (i >= fr.n)
                break;
            const int32_t x = xs[j];
            int32_t p, r;
            if (i == 0) {
                p = x;
                r = p;
            } else {
                p = (int32_t)((uint32_t)x - (uint32_t)tta::fixed_term(xprev, fr.pshift));
                h.adapt(rprev);
                r = (int32_t)((uint32_t)p - (uint32_t)h.predict(fr.hshift));
            }
            h.push(p);
            xprev = x;
            rprev = r;
            const uint32_t u = r > 0 ? ((uint32_t)r * 2u) - 1u : (0u - (uint32_t)r) * 2u;
            uint32_t k, val, run;
            if (u < (1u << (rs.k0 & 31))) {
                k = rs.k0;
                val = u;
                run = 0;
            } else {
                const uint32_t shifted = u - (1u << (rs.k0 & 31));
                k = rs.k1;
                run = 1u + (shifted >> (k & 31));
                val = shifted & ((1u << (k & 31)) - 1u);
                tta::rice_adapt(rs.k1, rs.sum1, shifted);
            }
            tta::rice_adapt(rs.k0, rs.sum0, u);
            bits += (uint64_t)run + 1u + k;
            mypre[i] = (uint32_t)bits;
            mytail[i] = val | (1u << (k & 31));
        }
    }
    chain_bits[g] = bits;
}

// ------------------------------------------------------------------- pack
__device__ __forceinline__ void or_bits(uint32_t *__restrict__ out, uint64_t pos, uint32_t v,
                                        uint32_t nb)
{
    // nb <= 32 bits of v at absolute bit position pos (LSB first)
    const uint64_t w = pos >> 5;
    const uint32_t sh = (uint32_t)pos & 31u;
    const uint32_t lo = v << sh;
    if (lo)
        atomicOr(out + w, lo);
    if (sh && sh + nb > 32u) {
        const uint32_t hi = v >> (32u - sh);
        if (hi)
            atomicOr(out + w + 1, hi);
    }
}

constexpr uint32_t kPackThreads = 256;

__global__ __launch_bounds__(256) void k_tta_pack(const Frame *__restrict__ frames,
                                                  uint32_t chunks_per_frame,
                                                  const uint32_t *__restrict__ pre,
                                                  const uint32_t *__restrict__ tail,
                                                  uint32_t *__restrict__ out)
{
    const uint32_t fidx = blockIdx.x / chunks_per_frame;
    const uint32_t chunk = blockIdx.x % chunks_per_frame;
    const Frame fr = frames[fidx];
    const uint32_t C = fr.channels;
    const uint64_t j = (uint64_t)chunk * kPackThreads + threadIdx.x;
    if (j >= (uint64_t)fr.n * C)
        return;
    const uint32_t i = (uint32_t)(j / C), c = (uint32_t)(j % C);
    // bits before sample (i, c): channels before c up to and including i,
    // channels from c on up to i - 1
    uint64_t off = 0;
    uint32_t mine_prev = 0, mine = 0;
    for (uint32_t cc = 0; cc < C; ++cc) {
        const uint32_t *P = pre + fr.sbase + (uint64_t)cc * fr.n;
        if (cc < c) {
            off += P[i];
        } else {
            const uint32_t v = i ? P[i - 1] : 0u;
            off += v;
            if (cc == c) {
                mine_prev = v;
                mine = P[i];
            }
        }
    }
    const uint32_t t = tail[fr.sbase + (uint64_t)c * fr.n + i];
    const uint32_t k = 31u - (uint32_t)__clz(t);
    const uint32_t val = t ^ (1u << k);
    uint32_t run = mine - mine_prev - 1u - k;
    uint64_t pos = fr.byte_off * 8u + off;
    // the unary run of ones
    if (run) {
        const uint32_t head = (32u - ((uint32_t)pos & 31u)) & 31u; // bits to a word edge
        if (run <= head || (head == 0 && run < 32u)) {
            or_bits(out, pos, (1u << run) - 1u, run);
            pos += run;
        } else {
            if (head) {
                or_bits(out, pos, (1u << head) - 1u, head);
                pos += head;
                run -= head;
            }
            uint64_t w = pos >> 5;
            for (; run >= 32u; run -= 32u, pos += 32u)
                out[w++] = 0xFFFFFFFFu; // whole words belong to this run alone
            if (run) {
                or_bits(out, pos, (1u << run) - 1u, run);
                pos += run;
            }
        }
    }
    // the stop bit and the k-bit tail
    or_bits(out, pos, val << 1, k + 1u);
}

// -------------------------------------------------------------------- crc
__global__ __launch_bounds__(256) void k_tta_crc(const Frame *__restrict__ frames,
                                                 uint8_t *__restrict__ out)
{
    __shared__ uint32_t tab[256];
    __shared__ uint32_t red[tta::kCrcThreads];
    const Frame fr = frames[blockIdx.x];
    const uint32_t crc = tta::crc32_block(out + fr.byte_off, fr.payload, tab, red);
    if (threadIdx.x < 4)
        out[fr.byte_off + fr.payload + threadIdx.x] = (uint8_t)(crc >> (8u * threadIdx.x));
}

// ------------------------------------------------------------------- host
thread_local ErrSlot g_tta_err;
#define THIP(expr) ATG_HIP_TRY(g_tta_err, expr, #expr)

// "tta_size" is everything between the chain and the pack: the copy of the
// chains' totals, the host's extents, the frame table's second upload and the
// clearing of the output the pack ORs into
const int kTTimed = 5;
const char *kTNames[kTTimed] = {"tta_chain", "tta_size", "tta_pack", "tta_crc", "tta_total"};

} // namespace

struct atg_tta_encoder : StageHandle<kTTimed> {
    DevBuf frames, chain_frame, pre, tail, chain_bits, h_pcm, h_out;
};

namespace {

struct TPlan {
    std::vector<Frame> frames;
    std::vector<uint32_t> chain_frame;
    std::vector<uint32_t> first, count; // per track
    uint64_t samples = 0;
    uint32_t max_n = 0;
};

atg_status tta_plan(const atg_track *tracks, uint32_t n, uint32_t channels, uint32_t bps,
                    uint32_t sample_rate, TPlan &P)
{
    if (bps != 8 && bps != 16 && bps != 24)
        return g_tta_err.fail(ATG_ERR_INVALID, "bits per sample must be 8, 16 or 24");
    if (channels < 1 || channels > 65535)
        return g_tta_err.fail(ATG_ERR_INVALID, "channels must be 1..65535");
    const uint64_t block = ((uint64_t)sample_rate * 256u) / 245u;
    if (block < 1 || block > 0xFFFFFFFFull)
        return g_tta_err.fail(ATG_ERR_INVALID, "sample rate gives no usable TTA block size");
    P.first.assign(n, 0);
    P.count.assign(n, 0);
    for (uint32_t t = 0; t < n; ++t) {
        const atg_track &T = tracks[t];
        P.first[t] = (uint32_t)P.frames.size();
        auto add = [&](uint64_t start, uint32_t len) {
            Frame f;
            std::memset(&f, 0, sizeof(f));
            f.pcm_start = T.pcm_offset + start;
            f.sbase = P.samples;
            f.chain0 = P.chain_frame.size();
            f.n = len;
            f.channels = (uint16_t)channels;
            f.hshift = bps == 16 ? 9 : 10;
            f.pshift = bps == 8 ? 4 : 5;
            P.samples += (uint64_t)len * channels;
            P.max_n = std::max(P.max_n, len);
            for (uint32_t c = 0; c < channels; ++c)
                P.chain_frame.push_back((uint32_t)P.frames.size());
            P.frames.push_back(f);
        };
        if (T.frame_sizes) {
            uint64_t pos = 0;
            for (uint64_t k = 0; k < T.n_frame_sizes; ++k) {
                const uint32_t len = T.frame_sizes[k];
                if (len < 1)
                    return g_tta_err.fail(ATG_ERR_INVALID, "frame sizes must be at least 1");
                add(pos, len);
                pos += len;
            }
            if (pos != T.pcm_frames)
                return g_tta_err.fail(ATG_ERR_INVALID, "frame sizes must sum to pcm_frames");
        } else {
            for (uint64_t pos = 0; pos < T.pcm_frames; pos += block)
                add(pos, (uint32_t)std::min<uint64_t>(block, T.pcm_frames - pos));
        }
        if (P.frames.size() > 0x7FFFFFFFull)
            return g_tta_err.fail(ATG_ERR_UNSUPPORTED, "too many TTA frames in one batch");
        P.count[t] = (uint32_t)P.frames.size() - P.first[t];
    }
    return ATG_OK;
}

template <typename T>
atg_status tta_run(atg_tta_encoder *enc, TPlan &P, const T *d_pcm, uint8_t *d_out, DevBuf *stage,
                   uint64_t out_cap, uint32_t n, atg_tta_track_result *res,
                   uint32_t *frame_bytes, uint64_t *needed, uint64_t *out_bytes)
{
    hipStream_t s = enc->s;
    const uint64_t nfr = P.frames.size(), nch = P.chain_frame.size();
    THIP(enc->frames.ensure(sizeof(Frame) * std::max<uint64_t>(nfr, 1)));
    THIP(enc->chain_frame.ensure(sizeof(uint32_t) * std::max<uint64_t>(nch, 1)));
    THIP(enc->pre.ensure(sizeof(uint32_t) * std::max<uint64_t>(P.samples, 1)));
    THIP(enc->tail.ensure(sizeof(uint32_t) * std::max<uint64_t>(P.samples, 1)));
    THIP(enc->chain_bits.ensure(sizeof(uint64_t) * std::max<uint64_t>(nch, 1)));
    if (nfr) {
        THIP(hipMemcpyAsync(enc->frames.p, P.frames.data(), sizeof(Frame) * nfr,
                            hipMemcpyHostToDevice, s));
        THIP(hipMemcpyAsync(enc->chain_frame.p, P.chain_frame.data(), sizeof(uint32_t) * nch,
                            hipMemcpyHostToDevice, s));
    }
    THIP(hipEventRecord(enc->ev[0], s));
    if (nch)
        hipLaunchKernelGGL(k_tta_chain<T>, dim3((unsigned)((nch + 63) / 64)), dim3(64), 0, s,
                           d_pcm, (const Frame *)enc->frames.p,
                           (const uint32_t *)enc->chain_frame.p, nch, (uint32_t *)enc->pre.p,
                           (uint32_t *)enc->tail.p, (uint64_t *)enc->chain_bits.p);
    THIP(hipGetLastError());
    THIP(hipEventRecord(enc->ev[1], s));
    std::vector<uint64_t> h_bits(nch, 0);
    if (nch)
        THIP(hipMemcpyAsync(h_bits.data(), enc->chain_bits.p, sizeof(uint64_t) * nch,
                            hipMemcpyDeviceToHost, s));
    THIP(hipStreamSynchronize(s));
    // the extents: every track's frames back to back, tracks 16-byte aligned
    uint64_t pos = 0;
    uint64_t chain = 0;
    for (uint32_t t = 0; t < n; ++t) {
        atg_tta_track_result &r = res[t];
        pos = (pos + 15) & ~15ull;
        r.out_offset = pos;
        r.first_frame = P.first[t];
        r.n_frames = P.count[t];
        r.pcm_frames = 0;
        r.status = 0;
        r.reserved = 0;
        for (uint32_t k = 0; k < P.count[t]; ++k) {
            Frame &f = P.frames[P.first[t] + k];
            uint64_t bits = 0;
            for (uint32_t c = 0; c < f.channels; ++c)
                bits += h_bits[chain++];
            const uint64_t payload = (bits + 7) / 8;
            // the running lengths are 32-bit, and the seektable entry too
            if (bits > 0xFFFFFFFFull || payload + 4 > 0xFFFFFFFFull)
                return g_tta_err.fail(ATG_ERR_UNSUPPORTED, "a TTA frame longer than 2^32 bits");
            f.byte_off = pos;
            f.payload = (uint32_t)payload;
            if (frame_bytes)
                frame_bytes[P.first[t] + k] = (uint32_t)payload + 4u;
            pos += payload + 4;
            r.pcm_frames += f.n;
        }
        r.bytes = pos - r.out_offset;
    }
    if (needed)
        *needed = pos;
    if (out_bytes)
        *out_bytes = pos;
    if (pos > out_cap)
        return g_tta_err.fail(ATG_ERR_CAPACITY, "output buffer smaller than the encoded batch");
    if (stage) { // host call: the device image is sized from the length pass
        THIP(stage->ensure(std::max<uint64_t>(pos, 4)));
        d_out = (uint8_t *)stage->p;
    }
    if (nfr)
        THIP(hipMemcpyAsync(enc->frames.p, P.frames.data(), sizeof(Frame) * nfr,
                            hipMemcpyHostToDevice, s));
    // the codes are OR-ed into place
    if (pos)
        THIP(hipMemsetAsync(d_out, 0, pos, s));
    THIP(hipEventRecord(enc->ev[2], s));
    if (nfr) {
        const uint64_t per = ((uint64_t)P.max_n * P.frames[0].channels + kPackThreads - 1) /
                             kPackThreads;
        const uint64_t blocks = per * nfr;
        if (per > 0xFFFFFFFFull || blocks > 0x7FFFFFFFull)
            return g_tta_err.fail(ATG_ERR_UNSUPPORTED, "batch too large for one pack launch");
        hipLaunchKernelGGL(k_tta_pack, dim3((unsigned)blocks), dim3(kPackThreads), 0, s,
                           (const Frame *)enc->frames.p, (uint32_t)per,
                           (const uint32_t *)enc->pre.p, (const uint32_t *)enc->tail.p,
                           (uint32_t *)d_out);
    }
    THIP(hipGetLastError());
    THIP(hipEventRecord(enc->ev[3], s));
    if (nfr)
        hipLaunchKernelGGL(k_tta_crc, dim3((unsigned)nfr), dim3(tta::kCrcThreads), 0, s,
                           (const Frame *)enc->frames.p, d_out);
    THIP(hipGetLastError());
    THIP(hipEventRecord(enc->ev[4], s));
    THIP(hipStreamSynchronize(s));
    enc->finish_times();
    return ATG_OK;
}

atg_status tta_check(atg_tta_encoder *e, const atg_track *tracks, uint32_t n,
                     atg_tta_track_result *results, atg_pcm_format fmt, uint32_t bps)
{
    if (!e || (!tracks && n) || (!results && n))
        return g_tta_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (fmt != ATG_PCM_S16 && fmt != ATG_PCM_S32)
        return g_tta_err.fail(ATG_ERR_INVALID, "unknown PCM format");
    if (fmt == ATG_PCM_S16 && bps > 16)
        return g_tta_err.fail(ATG_ERR_INVALID, "S16 PCM holds at most 16-bit samples");
    return ATG_OK;
}

} // namespace

extern "C" {

const char *atg_tta_last_error(void) { return g_tta_err.msg.c_str(); }

atg_status atg_tta_encoder_create(int device, atg_tta_encoder **out)
{
    return open_handle(device, out, g_tta_err, "encoder create");
}

void atg_tta_encoder_destroy(atg_tta_encoder *e)
{
    if (!e)
        return;
    e->close({&e->frames, &e->chain_frame, &e->pre, &e->tail, &e->chain_bits, &e->h_pcm,
              &e->h_out});
    delete e;
}

atg_status atg_tta_encode_device(atg_tta_encoder *e, const void *d_pcm, atg_pcm_format fmt,
                                 const atg_track *tracks, uint32_t n, uint32_t channels,
                                 uint32_t bps, uint32_t sample_rate, void *d_out,
                                 uint64_t out_cap, atg_tta_track_result *results,
                                 uint32_t *frame_bytes, uint64_t frame_bytes_cap,
                                 uint64_t *needed)
{
    ATG_HANDLE_LOCK(e);
    atg_status st = tta_check(e, tracks, n, results, fmt, bps);
    if (st != ATG_OK)
        return st;
    if (((uintptr_t)d_out) & 3)
        return g_tta_err.fail(ATG_ERR_INVALID, "d_out must be 4-byte aligned");
    THIP(hipSetDevice(e->device));
    TPlan P;
    st = tta_plan(tracks, n, channels, bps, sample_rate, P);
    if (st != ATG_OK)
        return st;
    if (frame_bytes && frame_bytes_cap < P.frames.size())
        return g_tta_err.fail(ATG_ERR_INVALID,
                              "frame_bytes holds fewer entries than the batch has frames");
    if (fmt == ATG_PCM_S16)
        return tta_run(e, P, (const int16_t *)d_pcm, (uint8_t *)d_out, nullptr, out_cap, n, results,
                       frame_bytes, needed, nullptr);
    return tta_run(e, P, (const int32_t *)d_pcm, (uint8_t *)d_out, nullptr, out_cap, n, results,
                   frame_bytes, needed, nullptr);
}

atg_status atg_tta_encode_host(atg_tta_encoder *e, const void *pcm, atg_pcm_format fmt,
                               const atg_track *tracks, uint32_t n, uint32_t channels,
                               uint32_t bps, uint32_t sample_rate, uint8_t *out,
                               uint64_t out_cap, atg_tta_track_result *results,
                               uint32_t *frame_bytes, uint64_t frame_bytes_cap,
                               uint64_t *needed)
{
    ATG_HANDLE_LOCK(e);
    atg_status st = tta_check(e, tracks, n, results, fmt, bps);
    if (st != ATG_OK)
        return st;
    if (!pcm && n)
        return g_tta_err.fail(ATG_ERR_INVALID, "NULL argument");
    THIP(hipSetDevice(e->device));
    TPlan P;
    st = tta_plan(tracks, n, channels, bps, sample_rate, P);
    if (st != ATG_OK)
        return st;
    if (frame_bytes && frame_bytes_cap < P.frames.size())
        return g_tta_err.fail(ATG_ERR_INVALID,
                              "frame_bytes holds fewer entries than the batch has frames");
    uint64_t frames = 0;
    for (uint32_t t = 0; t < n; ++t)
        frames = std::max<uint64_t>(frames, tracks[t].pcm_offset + tracks[t].pcm_frames);
    const size_t es = fmt == ATG_PCM_S16 ? 2 : 4;
    const uint64_t in_bytes = frames * channels * es;
    THIP(e->h_pcm.ensure(std::max<uint64_t>(in_bytes, 4)));
    if (in_bytes)
        THIP(hipMemcpyAsync(e->h_pcm.p, pcm, in_bytes, hipMemcpyHostToDevice, e->s));
    uint64_t total = 0;
    st = fmt == ATG_PCM_S16
             ? tta_run(e, P, (const int16_t *)e->h_pcm.p, nullptr, &e->h_out, out_cap, n,
                       results, frame_bytes, needed, &total)
             : tta_run(e, P, (const int32_t *)e->h_pcm.p, nullptr, &e->h_out, out_cap, n,
                       results, frame_bytes, needed, &total);
    if (st != ATG_OK)
        return st;
    if (total)
        THIP(hipMemcpyAsync(out, e->h_out.p, total, hipMemcpyDeviceToHost, e->s));
    THIP(hipStreamSynchronize(e->s));
    return ATG_OK;
}

int atg_tta_encoder_kernel_times(atg_tta_encoder *e, const char **names, float *ms, int cap)
{
    ATG_HANDLE_LOCK(e);
    return e ? e->report(kTNames, names, ms, cap) : 0;
}

} // extern "C"
