// wavpack_encode.hip — WavPack (.wv) encoder for a batch of tracks.
//
// Replaces the body of the reference's audiotools.encoders.encode_wavpack
// (src/encoders/wavpack.c): every read of block_size PCM frames becomes one
// block per channel group (init_context :262-290), and a track's output is
// the complete file: the blocks, the RIFF header sub-block in the first of
// them, the footer block with the MD5 of the PCM, total_samples in every
// header.
//
// A block carries its decoder state, but the encoder carries its own from
// block to block: weights, history samples and medians are round-tripped
// through their stored forms at every boundary (or reset where false stereo
// toggles).  The serial unit is therefore the stream, a track's blocks of
// one channel group; everything else is parallel over blocks.
//
//   k_wve_prep    one workgroup per block: magnitude, wasted bits and
//                 false-stereo equality by reduction, the CRC of the shifted
//                 samples as a linear recurrence in 256 pieces, then shift
//                 and joint stereo into the block's work slot.
//   k_wve_chain_wave  one wave per stream, block after block: lane 0 does the
//                 round trip or reset and the sub-blocks that hold the state
//                 at the block's start; then the passes run as a pipeline
//                 over the lanes (lane l: the l-th pass applied, on sample
//                 t - l at step t) and one more lane walks write_bitstream's
//                 state machine, only counting bits.  Leaves the residuals,
//                 the medians at each block's start and each bitstream's
//                 length.  No wave waits for another.
//   k_wve_md5in   the PCM in its hashed byte form (little endian at the
//                 sample width, 8-bit unsigned), hashed by md5.hip.
//   (host)        block sizes from the lengths, extents by prefix sum; a
//                 block has no useful a-priori bound (a unary run is as long
//                 as its value), so capacity is checked here.
//   k_wve_pack    one lane per block: header, sub-blocks, and the same walk
//                 writing the bits.
//   k_wve_finish  one lane per track: the footer block, the RIFF header over
//                 the dummy at byte 32 (over the footer's MD5 sub-block when
//                 the track is empty, as the reference does).
#include "handle_lock.h"
#include "host_common.h"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/atgpu.h"
#include "launch.h"
#include "wavpack_enc_core.h"

namespace {

using wve::EBlock;
using wve::EMeta;
using wve::EOpts;
using wve::EState;
using wve::EStream;
using wve::ETables;

struct ETrack {
    uint64_t pcm_start, frames; // PCM frames
    uint64_t out_off;           // the image in the output
    uint64_t footer_off;        // the footer block, from out_off
    uint64_t md5_off;           // its hashed bytes in the md5 staging buffer (64-aligned)
    uint32_t total, has_blocks;
};

constexpr uint32_t kPrepThreads = 256;

// ------------------------------------------------------------------- prep
template <typename T>
__global__ __launch_bounds__(256) void k_wve_prep(const T *__restrict__ pcm, EOpts o,
                                                  EBlock *__restrict__ blocks,
                                                  int32_t *__restrict__ work)
{
    __shared__ uint32_t red[4][kPrepThreads];
    __shared__ uint32_t crcs[kPrepThreads];
    const uint32_t t = threadIdx.x;
    EBlock b = blocks[blockIdx.x];
    wve::Scan s{0, 0, 0, 0};
    wve::scan_range(pcm, o.channels, b, t, kPrepThreads, s);
    red[0][t] = s.or0, red[1][t] = s.or1, red[2][t] = s.amax, red[3][t] = s.neq;
    __syncthreads();
    for (uint32_t d = kPrepThreads / 2; d; d >>= 1) {
        if (t < d) {
            red[0][t] |= red[0][t + d];
            red[1][t] |= red[1][t + d];
            red[2][t] = max(red[2][t], red[2][t + d]);
            red[3][t] |= red[3][t + d];
        }
        __syncthreads();
    }
    s = wve::Scan{red[0][0], red[1][0], red[2][0], red[3][0]};
    wve::decide(b, s, o);
    wve::transform_range(pcm, o.channels, b, o, work, t, kPrepThreads);
    const uint64_t m = (uint64_t)b.n * b.eff;
    const uint64_t per = (m + kPrepThreads - 1) / kPrepThreads;
    const uint64_t j0 = min(per * t, m), j1 = min(per * (t + 1), m);
    crcs[t] = wve::crc_piece(pcm, o.channels, b, j0, j1);
    __syncthreads();
    for (uint32_t d = kPrepThreads / 2; d; d >>= 1) {
        if (t < d)
            crcs[t] += crcs[t + d];
        __syncthreads();
    }
    if (t == 0) {
        b.crc = crcs[0] + 0xFFFFFFFFu * wve::pow3(m);
        blocks[blockIdx.x] = b;
    }
}

// ------------------------------------------------------------------ chain
// One wave per stream: lane l < nt is a pass, lane nt the walk (PipeLane in
// wavpack_enc_core.h).  Lane 0 takes sample t at step t, lane l what lane
// l - 1 made of sample t - l the step before.  The block's samples come in 64
// at a time, one per lane, a batch ahead of their use; the last pass stores
// the residuals for k_wve_pack.  Nothing is shared with another wave.
__global__ __launch_bounds__(64) void k_wve_chain_wave(const EStream *__restrict__ streams,
                                                       EBlock *blocks, EMeta *meta,
                                                       EState *state, int32_t *work, ETables tb,
                                                       uint32_t passes)
{
    const uint32_t lane = threadIdx.x;
    const EStream S = streams[blockIdx.x];
    EState &st = state[blockIdx.x];
    if (lane == 0)
        st.eff = S.nch;
    for (uint32_t k = 0; k < S.n_blocks; ++k) {
        EBlock &b = blocks[S.first_block + (uint64_t)k * S.step];
        EMeta &m = meta[S.first_block + (uint64_t)k * S.step];
        if (lane == 0)
            wve::begin_block(b, m, st, tb, passes);
        __threadfence(); // lane 0's state and terms, read by the other lanes
        const uint32_t eff = b.eff, n = b.n;
        const uint32_t nt = (uint32_t)wve::table_len(eff, passes);
        const int32_t p = (int32_t)nt - 1 - (int32_t)lane;
        const int32_t term = lane < nt ? m.term[p] : 0;
        wve::PipeLane L;
        if (lane < nt)
            L.load(term, st, p);
        wve::CountSink cs;
        wve::Walker<wve::CountSink> wk{cs, wve::Medians{st.ent[0][0], st.ent[0][1], st.ent[0][2]},
                                       wve::Medians{st.ent[1][0], st.ent[1][1], st.ent[1][2]}};
        int32_t *x0 = work + b.slot, *x1 = x0 + b.stride;
        int32_t out0 = 0, out1 = 0;
        int32_t nx0 = lane < n ? x0[lane] : 0;
        int32_t nx1 = (eff == 2 && lane < n) ? x1[lane] : 0;
        const uint64_t steps = (uint64_t)n + nt;
        for (uint64_t t0 = 0; t0 < steps; t0 += 64) {
            const int32_t c0 = nx0, c1 = nx1;
            const uint64_t idx = t0 + 64u + lane;
            nx0 = idx < n ? x0[idx] : 0;
            nx1 = (eff == 2 && idx < n) ? x1[idx] : 0;
            const uint32_t tend = (uint32_t)(steps - t0 < 64u ? steps - t0 : 64u);
            for (uint32_t tt = 0; tt < tend; ++tt) {
                const int32_t f0 = __shfl(c0, (int)tt), f1 = __shfl(c1, (int)tt);
                const int32_t u0 = __shfl_up(out0, 1), u1 = __shfl_up(out1, 1);
                const int32_t in0 = lane == 0 ? f0 : u0, in1 = lane == 0 ? f1 : u1;
                const int64_t i = (int64_t)(t0 + tt) - lane;
                const bool live = i >= 0 && i < (int64_t)n;
                if (lane < nt) {
                    if (live) {
                        L.step(in0, in1, out0, out1);
                        if (lane + 1 == nt) {
                            x0[i] = out0;
                            if (eff == 2)
                                x1[i] = out1;
                        }
                    }
                } else if (lane == nt && live) {
                    wk.step(in0, wk.e0);
                    if (eff == 2)
                        wk.step(in1, wk.e1);
                }
            }
        }
        if (lane < nt)
            L.store(term, st, p);
        if (lane == nt) {
            wk.end();
            st.ent[0][0] = wk.e0.a, st.ent[0][1] = wk.e0.b, st.ent[0][2] = wk.e0.c;
            st.ent[1][0] = wk.e1.a, st.ent[1][1] = wk.e1.b, st.ent[1][2] = wk.e1.c;
            b.bits = cs.bits;
        }
        __threadfence(); // the state, read by lane 0 at the next block's start
    }
}

// ------------------------------------------------------------------- pack
__global__ __launch_bounds__(64) void k_wve_pack(const EBlock *__restrict__ blocks, uint32_t n,
                                                 const EMeta *__restrict__ meta, EOpts o,
                                                 const int32_t *__restrict__ work,
                                                 const uint32_t *__restrict__ sub_bytes,
                                                 uint8_t *__restrict__ out)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n)
        return;
    wve::pack_block(blocks[g], meta[g], o, work, sub_bytes[g], out);
}

// the fmt chunk is the classic one for up to two channels of up to 16 bits
__device__ void put_wave_header(wve::Out &w, const EOpts &o, uint64_t frames)
{
    const uint32_t bb = o.bps / 8u;
    const uint32_t data = (uint32_t)(frames * o.channels * bb);
    const bool classic = o.channels <= 2 && o.bps <= 16;
    const uint32_t fmt = classic ? 16u : 40u;
    const uint32_t total = 12u + 8u + fmt + 8u + data;
    w.u8('R'), w.u8('I'), w.u8('F'), w.u8('F');
    w.u32(total - 8u);
    w.u8('W'), w.u8('A'), w.u8('V'), w.u8('E');
    w.u8('f'), w.u8('m'), w.u8('t'), w.u8(' ');
    w.u32(fmt);
    w.u16(classic ? 1u : 0xFFFEu);
    w.u16(o.channels);
    w.u32(o.rate);
    w.u32(o.rate * o.channels * bb);
    w.u16(o.channels * bb);
    w.u16(o.bps);
    if (!classic) {
        w.u16(22);
        w.u16(o.bps);
        w.u32(o.mask);
        const uint8_t sub[16] = {0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x10, 0x00,
                                 0x80, 0x00, 0x00, 0xaa, 0x00, 0x38, 0x9b, 0x71};
        for (uint32_t k = 0; k < 16; ++k)
            w.u8(sub[k]);
    }
    w.u8('d'), w.u8('a'), w.u8('t'), w.u8('a');
    w.u32(data);
}

__global__ __launch_bounds__(64) void k_wve_finish(const ETrack *__restrict__ tracks, uint32_t n,
                                                   EOpts o, const uint8_t *__restrict__ md5,
                                                   uint8_t *__restrict__ out)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n)
        return;
    const ETrack T = tracks[t];
    wve::Out f{out + T.out_off + T.footer_off};
    wve::put_header(f, 18u, T.total, 0xFFFFFFFFu, 0u,
                    wve::header_flags(o, 1u, 0u, 0u, 0u, 1u, 1u, 0u, 0u), 0xFFFFFFFFu);
    f.sub_head(6, 1, 16);
    for (uint32_t k = 0; k < 16; ++k)
        f.u8(md5[16u * t + k]);
    // data sizes of 2^32 and more keep the dummy
    if (T.frames * o.channels * (o.bps / 8u) < (1ull << 32)) {
        wve::Out h{out + T.out_off + 32u};
        h.sub_head(1, 1, o.wave_bytes);
        put_wave_header(h, o, T.frames);
    }
}

// --------------------------------------------------------------- md5 input
// a lane per four samples of a track: 4 bb bytes in whole dwords
template <typename S>
__global__ __launch_bounds__(256) void k_wve_md5in(const S *__restrict__ pcm,
                                                   const ETrack *__restrict__ tracks, uint32_t n,
                                                   uint32_t C, uint32_t bb,
                                                   uint8_t *__restrict__ dst)
{
    for (uint32_t t = blockIdx.y; t < n; t += gridDim.y) {
        const ETrack T = tracks[t];
        const uint64_t ns = T.frames * C;
        const uint64_t i = 4u * ((uint64_t)blockIdx.x * 256u + threadIdx.x);
        if (i >= ns)
            continue;
        const S *src = pcm + T.pcm_start * C;
        uint8_t *d = dst + T.md5_off;
        const uint32_t flip = bb == 1u ? 0x80u : 0u; // 8-bit samples are hashed unsigned
        if (i + 4u <= ns) {
            const uint32_t v0 = (uint32_t)(int32_t)src[i] ^ flip, v1 = (uint32_t)(int32_t)src[i + 1] ^ flip;
            const uint32_t v2 = (uint32_t)(int32_t)src[i + 2] ^ flip,
                           v3 = (uint32_t)(int32_t)src[i + 3] ^ flip;
            uint32_t *q = (uint32_t *)(d + i * bb);
            if (bb == 1u) {
                q[0] = (v0 & 0xFFu) | ((v1 & 0xFFu) << 8) | ((v2 & 0xFFu) << 16) | (v3 << 24);
            } else if (bb == 2u) {
                q[0] = (v0 & 0xFFFFu) | (v1 << 16);
                q[1] = (v2 & 0xFFFFu) | (v3 << 16);
            } else {
                q[0] = (v0 & 0xFFFFFFu) | (v1 << 24);
                q[1] = ((v1 >> 8) & 0xFFFFu) | (v2 << 16);
                q[2] = ((v2 >> 16) & 0xFFu) | (v3 << 8);
            }
        } else {
            for (uint64_t k = i; k < ns; ++k) {
                const uint32_t v = (uint32_t)(int32_t)src[k] ^ flip;
                for (uint32_t q = 0; q < bb; ++q)
                    d[k * bb + q] = (uint8_t)(v >> (8u * q));
            }
        }
    }
}

// ------------------------------------------------------------------- host
thread_local ErrSlot g_wve_err;
#define EHIP(expr) ATG_HIP_TRY(g_wve_err, expr, #expr)

// "wv_size" is everything between the chain and the pack: the block table
// copied to the host, the extents, the table's second upload
const int kETimed = 6;
const char *kENames[kETimed] = {"wv_prep", "wv_chain", "wv_md5", "wv_size", "wv_pack", "wv_total"};

uint32_t rate_code(uint32_t rate)
{
    static const uint32_t rates[15] = {6000,  8000,  9600,  11025, 12000, 16000, 22050, 24000,
                                       32000, 44100, 48000, 64000, 88200, 96000, 192000};
    for (uint32_t k = 0; k < 15; ++k)
        if (rates[k] == rate)
            return k;
    return 15;
}

// lanes per workgroup for kernels whose lanes are long serial walks: few
// lanes to a wave while the batch leaves SIMDs idle
uint32_t walk_lanes(uint64_t n)
{
    uint32_t l = 1;
    while (l < 64 && n / l > 2048)
        l *= 2;
    return l;
}

} // namespace

struct atg_wv_encoder : StageHandle<kETimed> {
    DevBuf blocks, streams, meta, state, work, tracks, sub_bytes, tables, md5in, md5meta, md5,
        h_pcm, h_out;
};

namespace {

struct EPlan {
    EOpts o;
    std::vector<EBlock> blocks;
    std::vector<EStream> streams;
    std::vector<ETrack> tracks;
    std::vector<uint32_t> first, count; // blocks per track
    uint64_t work = 0, md5_bytes = 0, max_samples = 0;
};

atg_status wve_plan(const atg_track *tracks, uint32_t n, uint32_t channels, uint32_t mask,
                    uint32_t bps, uint32_t rate, const atg_wv_enc_options *opt, EPlan &P)
{
    if (bps != 8 && bps != 16 && bps != 24)
        return g_wve_err.fail(ATG_ERR_INVALID, "bits per sample must be 8, 16 or 24");
    if (channels < 1)
        return g_wve_err.fail(ATG_ERR_INVALID, "channels must be at least 1");
    if (channels > 255)
        return g_wve_err.fail(ATG_ERR_UNSUPPORTED,
                              "the channel-info sub-block holds at most 255 channels");
    const uint32_t passes = opt->correlation_passes;
    if (passes != 0 && passes != 1 && passes != 2 && passes != 5 && passes != 10 && passes != 16)
        return g_wve_err.fail(ATG_ERR_INVALID, "correlation passes must be 0, 1, 2, 5, 10 or 16");
    if (opt->block_size < 1)
        return g_wve_err.fail(ATG_ERR_INVALID, "block size must be at least 1");
    uint8_t split[256];
    const uint32_t S = wv::stream_split(channels, mask, split, 256);
    if (passes)
        for (uint32_t k = 0; k < S; ++k)
            if (opt->block_size < wv::term_depth(split[k], passes))
                return g_wve_err.fail(ATG_ERR_INVALID,
                             "block size below the history depth of the pass table");
    EOpts &o = P.o;
    o.channels = channels, o.mask = mask, o.bps = bps, o.rate = rate;
    o.rate_code = rate_code(rate);
    o.passes = passes;
    o.joint = opt->joint_stereo ? 1 : 0;
    o.false_stereo = opt->false_stereo ? 1 : 0;
    o.wasted = opt->wasted_bits ? 1 : 0;
    o.wave_bytes = 20u + ((channels <= 2 && bps <= 16) ? 16u : 40u) + 8u;
    const uint64_t B = opt->block_size;
    P.first.assign(n, 0);
    P.count.assign(n, 0);
    P.tracks.resize(n);
    for (uint32_t t = 0; t < n; ++t) {
        const atg_track &T = tracks[t];
        if (T.frame_sizes)
            return g_wve_err.fail(ATG_ERR_UNSUPPORTED,
                                  "explicit frame sizes: WavPack is fed whole blocks");
        if (T.pcm_frames >= 0xFFFFFFFFull)
            return g_wve_err.fail(ATG_ERR_INVALID,
                                  "a WavPack file holds fewer than 2^32 - 1 frames");
        const uint64_t sets = (T.pcm_frames + B - 1) / B;
        if (P.blocks.size() + sets * S > 0x7FFFFFFFull)
            return g_wve_err.fail(ATG_ERR_UNSUPPORTED, "too many WavPack blocks in one batch");
        P.first[t] = (uint32_t)P.blocks.size();
        ETrack &D = P.tracks[t];
        std::memset(&D, 0, sizeof(D));
        D.pcm_start = T.pcm_offset;
        D.frames = T.pcm_frames;
        D.total = (uint32_t)T.pcm_frames;
        D.has_blocks = sets ? 1 : 0;
        D.md5_off = P.md5_bytes;
        P.md5_bytes += (T.pcm_frames * channels * (bps / 8u) + 63u) & ~63ull;
        P.max_samples = std::max<uint64_t>(P.max_samples, T.pcm_frames * channels);
        if (sets)
            for (uint32_t k = 0; k < S; ++k)
                P.streams.push_back(EStream{P.first[t] + k, (uint32_t)sets, S, split[k]});
        for (uint64_t q = 0; q < sets; ++q) {
            const uint32_t len = (uint32_t)std::min<uint64_t>(B, T.pcm_frames - q * B);
            uint32_t ch = 0;
            for (uint32_t k = 0; k < S; ++k) {
                EBlock b;
                std::memset(&b, 0, sizeof(b));
                b.pcm_start = T.pcm_offset + q * B;
                b.slot = P.work;
                b.n = len;
                b.stride = (len + wve::kGroup - 1) / wve::kGroup * wve::kGroup;
                b.block_index = (uint32_t)(q * B);
                b.total = D.total;
                b.track = t;
                b.first_ch = (uint8_t)ch;
                b.nch = split[k];
                b.first = k == 0;
                b.last = k + 1 == S;
                b.first_of_file = q == 0 && k == 0;
                P.work += (uint64_t)b.stride * b.nch;
                ch += split[k];
                P.blocks.push_back(b);
            }
        }
        P.count[t] = (uint32_t)P.blocks.size() - P.first[t];
    }
    return ATG_OK;
}

template <typename T>
atg_status wve_run(atg_wv_encoder *enc, EPlan &P, const T *d_pcm, uint8_t *d_out, DevBuf *stage,
                   uint64_t out_cap, uint32_t n, atg_wv_track_result *res, uint32_t *block_bytes,
                   uint64_t *needed, uint64_t *out_bytes)
{
    hipStream_t s = enc->s;
    const EOpts &o = P.o;
    const uint64_t nb = P.blocks.size(), ns = P.streams.size();
    EHIP(enc->blocks.ensure(sizeof(EBlock) * std::max<uint64_t>(nb, 1)));
    EHIP(enc->meta.ensure(sizeof(EMeta) * std::max<uint64_t>(nb, 1)));
    EHIP(enc->sub_bytes.ensure(sizeof(uint32_t) * std::max<uint64_t>(nb, 1)));
    EHIP(enc->streams.ensure(sizeof(EStream) * std::max<uint64_t>(ns, 1)));
    EHIP(enc->state.ensure(sizeof(EState) * std::max<uint64_t>(ns, 1)));
    EHIP(enc->work.ensure(sizeof(int32_t) * std::max<uint64_t>(P.work, 1)));
    EHIP(enc->tracks.ensure(sizeof(ETrack) * std::max<uint32_t>(n, 1)));
    EHIP(enc->md5in.ensure(std::max<uint64_t>(P.md5_bytes, 64)));
    EHIP(enc->md5meta.ensure(sizeof(uint64_t) * 2 * std::max<uint32_t>(n, 1)));
    EHIP(enc->md5.ensure(16ull * std::max<uint32_t>(n, 1)));
    const ETables tb{(const uint8_t *)enc->tables.p,
                     (const uint16_t *)((const uint8_t *)enc->tables.p + 256)};
    if (nb) {
        EHIP(hipMemcpyAsync(enc->blocks.p, P.blocks.data(), sizeof(EBlock) * nb,
                            hipMemcpyHostToDevice, s));
        EHIP(hipMemcpyAsync(enc->streams.p, P.streams.data(), sizeof(EStream) * ns,
                            hipMemcpyHostToDevice, s));
        EHIP(hipMemsetAsync(enc->state.p, 0, sizeof(EState) * ns, s));
    }
    std::vector<uint64_t> md5meta(2 * (size_t)std::max<uint32_t>(n, 1));
    for (uint32_t t = 0; t < n; ++t) {
        md5meta[t] = P.tracks[t].md5_off;
        md5meta[n + t] = P.tracks[t].frames * o.channels * (o.bps / 8u);
    }
    if (n) {
        EHIP(hipMemcpyAsync(enc->tracks.p, P.tracks.data(), sizeof(ETrack) * n,
                            hipMemcpyHostToDevice, s));
        EHIP(hipMemcpyAsync(enc->md5meta.p, md5meta.data(), sizeof(uint64_t) * 2 * n,
                            hipMemcpyHostToDevice, s));
    }
    EHIP(hipEventRecord(enc->ev[0], s));
    if (nb)
        hipLaunchKernelGGL(k_wve_prep<T>, dim3((unsigned)nb), dim3(kPrepThreads), 0, s, d_pcm, o,
                           (EBlock *)enc->blocks.p, (int32_t *)enc->work.p);
    EHIP(hipGetLastError());
    EHIP(hipEventRecord(enc->ev[1], s));
    if (ns)
        hipLaunchKernelGGL(k_wve_chain_wave, dim3((unsigned)ns), dim3(64), 0, s,
                           (const EStream *)enc->streams.p, (EBlock *)enc->blocks.p,
                           (EMeta *)enc->meta.p, (EState *)enc->state.p, (int32_t *)enc->work.p,
                           tb, o.passes);
    EHIP(hipGetLastError());
    EHIP(hipEventRecord(enc->ev[2], s));
    if (n) {
        if (P.max_samples) {
            const uint64_t gx = (P.max_samples + 1023u) / 1024u;
            if (gx > 0x7FFFFFFFull)
                return g_wve_err.fail(ATG_ERR_UNSUPPORTED,
                                      "track too long for one MD5 staging launch");
            hipLaunchKernelGGL(k_wve_md5in<T>, dim3((unsigned)gx, std::min<uint32_t>(n, 65535u)),
                               dim3(256), 0, s, d_pcm, (const ETrack *)enc->tracks.p, n,
                               o.channels, o.bps / 8u, (uint8_t *)enc->md5in.p);
            EHIP(hipGetLastError());
        }
        EHIP(launch_bytes_md5((const uint8_t *)enc->md5in.p, (const uint64_t *)enc->md5meta.p,
                              (const uint64_t *)enc->md5meta.p + n, n, (uint8_t *)enc->md5.p, s));
    }
    EHIP(hipEventRecord(enc->ev[3], s));
    if (nb)
        EHIP(hipMemcpyAsync(P.blocks.data(), enc->blocks.p, sizeof(EBlock) * nb,
                            hipMemcpyDeviceToHost, s));
    std::vector<uint8_t> md5(16 * (size_t)std::max<uint32_t>(n, 1));
    if (n)
        EHIP(hipMemcpyAsync(md5.data(), enc->md5.p, 16ull * n, hipMemcpyDeviceToHost, s));
    EHIP(hipStreamSynchronize(s));
    // the extents: every track's blocks back to back, tracks 16-byte aligned
    std::vector<uint32_t> subs(std::max<uint64_t>(nb, 1));
    uint64_t pos = 0;
    for (uint32_t t = 0; t < n; ++t) {
        atg_wv_track_result &r = res[t];
        ETrack &D = P.tracks[t];
        pos = (pos + 15) & ~15ull;
        r.out_offset = D.out_off = pos;
        r.first_block = P.first[t];
        r.n_blocks = P.count[t];
        r.pcm_frames = D.frames;
        r.status = 0;
        r.reserved = 0;
        std::memcpy(r.md5, md5.data() + 16 * (size_t)t, 16);
        for (uint32_t k = 0; k < P.count[t]; ++k) {
            EBlock &b = P.blocks[P.first[t] + k];
            const uint64_t sub = wve::block_sub_bytes(b, o);
            if (sub + 24u > 0xFFFFFFFFull)
                return g_wve_err.fail(ATG_ERR_UNSUPPORTED,
                                      "a WavPack block longer than 2^32 bytes");
            subs[P.first[t] + k] = (uint32_t)sub;
            b.byte_off = pos;
            if (block_bytes)
                block_bytes[P.first[t] + k] = (uint32_t)sub + 32u;
            pos += sub + 32u;
        }
        D.footer_off = pos - D.out_off;
        // an empty track's RIFF header goes over the footer's MD5 sub-block
        pos += P.count[t] ? 50u : 32u + 2u + o.wave_bytes;
        r.bytes = pos - r.out_offset;
    }
    if (needed)
        *needed = pos;
    if (out_bytes)
        *out_bytes = pos;
    if (pos > out_cap)
        return g_wve_err.fail(ATG_ERR_CAPACITY, "output buffer smaller than the encoded batch");
    if (stage) { // host call: the device image is sized from the length pass
        EHIP(stage->ensure(std::max<uint64_t>(pos, 4)));
        d_out = (uint8_t *)stage->p;
    }
    if (nb) {
        EHIP(hipMemcpyAsync(enc->blocks.p, P.blocks.data(), sizeof(EBlock) * nb,
                            hipMemcpyHostToDevice, s));
        EHIP(hipMemcpyAsync(enc->sub_bytes.p, subs.data(), sizeof(uint32_t) * nb,
                            hipMemcpyHostToDevice, s));
    }
    if (n)
        EHIP(hipMemcpyAsync(enc->tracks.p, P.tracks.data(), sizeof(ETrack) * n,
                            hipMemcpyHostToDevice, s));
    if (pos) // the gaps between the tracks
        EHIP(hipMemsetAsync(d_out, 0, pos, s));
    EHIP(hipEventRecord(enc->ev[4], s));
    if (nb) {
        const uint32_t lanes = walk_lanes(nb);
        hipLaunchKernelGGL(k_wve_pack, dim3((unsigned)((nb + lanes - 1) / lanes)), dim3(lanes), 0,
                           s, (const EBlock *)enc->blocks.p, (uint32_t)nb,
                           (const EMeta *)enc->meta.p, o, (const int32_t *)enc->work.p,
                           (const uint32_t *)enc->sub_bytes.p, d_out);
    }
    EHIP(hipGetLastError());
    if (n)
        hipLaunchKernelGGL(k_wve_finish, dim3((n + 63u) / 64u), dim3(64), 0, s,
                           (const ETrack *)enc->tracks.p, n, o, (const uint8_t *)enc->md5.p,
                           d_out);
    EHIP(hipGetLastError());
    EHIP(hipEventRecord(enc->ev[5], s));
    EHIP(hipStreamSynchronize(s));
    enc->finish_times();
    return ATG_OK;
}

atg_status wve_check(atg_wv_encoder *e, const atg_track *tracks, uint32_t n,
                     atg_wv_track_result *results, atg_pcm_format fmt, uint32_t bps,
                     const atg_wv_enc_options *opt)
{
    if (!e || !opt || (!tracks && n) || (!results && n))
        return g_wve_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (fmt != ATG_PCM_S16 && fmt != ATG_PCM_S32)
        return g_wve_err.fail(ATG_ERR_INVALID, "unknown PCM format");
    if (fmt == ATG_PCM_S16 && bps > 16)
        return g_wve_err.fail(ATG_ERR_INVALID, "S16 PCM holds at most 16-bit samples");
    return ATG_OK;
}

} // namespace

extern "C" {

const char *atg_wv_encoder_last_error(void) { return g_wve_err.msg.c_str(); }

atg_status atg_wv_encoder_create(int device, atg_wv_encoder **out)
{
    atg_status st = open_handle(device, out, g_wve_err, "encoder create");
    if (st != ATG_OK)
        return st;
    atg_wv_encoder *e = *out;
    hipError_t err = e->tables.ensure(256 + sizeof(uint16_t) * 256);
    if (err == hipSuccess) {
        // the tables of the 16-bit log form: floor(256 log2(1 + i/256) + 0.5)
        // and floor(256 2^(i/256) + 0.5)
        uint8_t tab[256 + 512];
        uint16_t ex[256];
        for (int i = 0; i < 256; ++i) {
            tab[i] = (uint8_t)std::floor(256.0 * std::log2(1.0 + i / 256.0) + 0.5);
            ex[i] = (uint16_t)std::floor(256.0 * std::exp2(i / 256.0) + 0.5);
        }
        std::memcpy(tab + 256, ex, sizeof(ex));
        err = hipMemcpy(e->tables.p, tab, sizeof(tab), hipMemcpyHostToDevice);
    }
    if (err != hipSuccess) {
        *out = nullptr;
        atg_wv_encoder_destroy(e);
        return g_wve_err.fail(ATG_ERR_DEVICE,
                              std::string("encoder create: ") + hipGetErrorString(err));
    }
    return ATG_OK;
}

void atg_wv_encoder_destroy(atg_wv_encoder *e)
{
    if (!e)
        return;
    e->close({&e->blocks, &e->streams, &e->meta, &e->state, &e->work, &e->tracks, &e->sub_bytes,
              &e->tables, &e->md5in, &e->md5meta, &e->md5, &e->h_pcm, &e->h_out});
    delete e;
}

atg_status atg_wv_encode_device(atg_wv_encoder *e, const void *d_pcm, atg_pcm_format fmt,
                                const atg_track *tracks, uint32_t n, uint32_t channels,
                                uint32_t channel_mask, uint32_t bps, uint32_t sample_rate,
                                const atg_wv_enc_options *options, void *d_out, uint64_t out_cap,
                                atg_wv_track_result *results, uint32_t *block_bytes,
                                uint64_t block_bytes_cap, uint64_t *needed)
{
    ATG_HANDLE_LOCK(e);
    atg_status st = wve_check(e, tracks, n, results, fmt, bps, options);
    if (st != ATG_OK)
        return st;
    EHIP(hipSetDevice(e->device));
    EPlan P;
    st = wve_plan(tracks, n, channels, channel_mask, bps, sample_rate, options, P);
    if (st != ATG_OK)
        return st;
    if (block_bytes && block_bytes_cap < P.blocks.size())
        return g_wve_err.fail(ATG_ERR_INVALID,
                              "block_bytes holds fewer entries than the batch has blocks");
    if (fmt == ATG_PCM_S16)
        return wve_run(e, P, (const int16_t *)d_pcm, (uint8_t *)d_out, nullptr, out_cap, n, results,
                       block_bytes, needed, nullptr);
    return wve_run(e, P, (const int32_t *)d_pcm, (uint8_t *)d_out, nullptr, out_cap, n, results,
                   block_bytes, needed, nullptr);
}

atg_status atg_wv_encode_host(atg_wv_encoder *e, const void *pcm, atg_pcm_format fmt,
                              const atg_track *tracks, uint32_t n, uint32_t channels,
                              uint32_t channel_mask, uint32_t bps, uint32_t sample_rate,
                              const atg_wv_enc_options *options, uint8_t *out, uint64_t out_cap,
                              atg_wv_track_result *results, uint32_t *block_bytes,
                              uint64_t block_bytes_cap, uint64_t *needed)
{
    ATG_HANDLE_LOCK(e);
    atg_status st = wve_check(e, tracks, n, results, fmt, bps, options);
    if (st != ATG_OK)
        return st;
    EHIP(hipSetDevice(e->device));
    EPlan P;
    st = wve_plan(tracks, n, channels, channel_mask, bps, sample_rate, options, P);
    if (st != ATG_OK)
        return st;
    if (block_bytes && block_bytes_cap < P.blocks.size())
        return g_wve_err.fail(ATG_ERR_INVALID,
                              "block_bytes holds fewer entries than the batch has blocks");
    uint64_t frames = 0;
    for (uint32_t t = 0; t < n; ++t)
        frames = std::max<uint64_t>(frames, tracks[t].pcm_offset + tracks[t].pcm_frames);
    if (!pcm && frames)
        return g_wve_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (!out && out_cap)
        return g_wve_err.fail(ATG_ERR_INVALID, "NULL argument");
    const size_t es = fmt == ATG_PCM_S16 ? 2 : 4;
    const uint64_t in_bytes = frames * channels * es;
    EHIP(e->h_pcm.ensure(std::max<uint64_t>(in_bytes, 4)));
    if (in_bytes)
        EHIP(hipMemcpyAsync(e->h_pcm.p, pcm, in_bytes, hipMemcpyHostToDevice, e->s));
    uint64_t total = 0;
    st = fmt == ATG_PCM_S16
             ? wve_run(e, P, (const int16_t *)e->h_pcm.p, nullptr, &e->h_out, out_cap, n, results,
                       block_bytes, needed, &total)
             : wve_run(e, P, (const int32_t *)e->h_pcm.p, nullptr, &e->h_out, out_cap, n, results,
                       block_bytes, needed, &total);
    if (st != ATG_OK)
        return st;
    if (total)
        EHIP(hipMemcpyAsync(out, e->h_out.p, total, hipMemcpyDeviceToHost, e->s));
    EHIP(hipStreamSynchronize(e->s));
    return ATG_OK;
}

int atg_wv_encoder_kernel_times(atg_wv_encoder *e, const char **names, float *ms, int cap)
{
    ATG_HANDLE_LOCK(e);
    return e ? e->report(kENames, names, ms, cap) : 0;
}

} // extern "C"
