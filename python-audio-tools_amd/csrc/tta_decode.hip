// tta_decode.hip — True Audio (TTA1) decoder for a batch of images.
//
// Replaces the reference's audiotools.decoders.TTADecoder
// (src/decoders/tta.c: read_header :357-404, read_seektable :406-436,
// TTADecoder_read :194-262, read_frame :438-544, hybrid_filter :546-619,
// fixed_prediction :621-637, decorrelate_channels :639-681).
//
// The host parses header and seektable (atg_tta_read_info) and lays the
// frames out from the seektable; a frame whose bytes are not all in the
// image is the track's "I/O error reading frame" and nothing of it is
// touched.  On the device, per frame:
//
//   k_ttad_crc     one workgroup per frame: CRC-32 of the payload against
//                  the trailing word, before anything is decoded
//                  (TTADecoder_read :230-245).
//   k_ttad_parse   one lane per frame: the interleaved Rice stream to
//                  channel-major residuals.  The adaptive k makes the walk
//                  serial.  Every read is bounded by the frame's payload: a
//                  code that would run past it ends the frame with
//                  ATG_TD_FRAME_READ, and only the frame's own slot is
//                  written.  A unary run may span millions of bits; it is
//                  consumed a word at a time.
//   k_ttad_chain   one lane per (frame, channel): the inverse hybrid filter
//                  and the inverse fixed prediction, in place.
//   k_ttad_out     one lane per PCM frame: decorrelate and interleave.
//
// A track's PCM ends before its first bad frame.
#include "handle_lock.h"
#include "host_common.h"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/atgpu.h"
#include "bits_lsb.h"
#include "tta_common.h"

namespace {

using tta::Frame;

__global__ __launch_bounds__(256) void k_ttad_crc(const Frame *__restrict__ frames,
                                                  const uint8_t *__restrict__ data,
                                                  int32_t *__restrict__ status)
{
    __shared__ uint32_t tab[256];
    __shared__ uint32_t red[tta::kCrcThreads];
    const Frame fr = frames[blockIdx.x];
    const uint8_t *p = data + fr.byte_off;
    const uint32_t crc = tta::crc32_block(p, fr.payload, tab, red);
    if (threadIdx.x == 0) {
        const uint8_t *q = p + fr.payload;
        const uint32_t want = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) |
                              ((uint32_t)q[3] << 24);
        status[blockIdx.x] = crc == want ? ATG_TD_OK : ATG_TD_CRC_MISMATCH;
    }
}

constexpr uint32_t kMaxCh = 8; // Rice states kept in private memory up to here

// CT: the batch's channel count when every track has 1 or 2 channels (the
// Rice states are then registers), 0 for any mix of counts
template <uint32_t CT>
__global__ __launch_bounds__(64) void k_ttad_parse(const Frame *__restrict__ frames,
                                                   uint32_t n_frames,
                                                   const uint8_t *__restrict__ data,
                                                   int32_t *__restrict__ status,
                                                   int32_t *__restrict__ resid,
                                                   tta::Rice *__restrict__ wide_state)
{
    const uint32_t f = blockIdx.x * 64u + threadIdx.x;
    if (f >= n_frames || status[f] != ATG_TD_OK)
        return;
    const Frame fr = frames[f];
    const uint32_t C = CT ? CT : fr.channels;
    // only words that hold at least one byte of the payload are loaded (it
    // is followed by the frame's 4 CRC bytes and starts inside the batch
    // buffer, so such a word lies inside the buffer)
    LsbReader<false> br;
    br.data = data;
    br.pos = fr.byte_off;
    br.end = fr.byte_off + fr.payload;
    tta::Rice reg[CT ? CT : kMaxCh];
    // more channels than registers hold: the states live in the frame's own
    // row of wide_state
    tta::Rice *st = C <= kMaxCh ? reg : wide_state + fr.chain0;
    if (C > kMaxCh)
        for (uint32_t c = 0; c < C; ++c)
            st[c] = tta::Rice();
    int32_t *out = resid + fr.sbase;
    for (uint32_t i = 0; i < fr.n; ++i) {
        for (uint32_t c = 0; c < C; ++c) {
            tta::Rice rs = st[c];
            uint32_t msb, u = 0;
            bool ok = br.unary(msb);
            if (ok && msb == 0) {
                ok = br.bits(rs.k0 & 31u, u);
            } else if (ok) {
                uint32_t lsb = 0;
                ok = br.bits(rs.k1 & 31u, lsb);
                const uint32_t unshifted = ((msb - 1u) << (rs.k1 & 31u)) + lsb;
                u = unshifted + (1u << (rs.k0 & 31u));
                tta::rice_adapt(rs.k1, rs.sum1, unshifted);
            }
            if (!ok) {
                status[f] = ATG_TD_FRAME_READ;
                return;
            }
            tta::rice_adapt(rs.k0, rs.sum0, u);
            st[c] = rs;
            out[(uint64_t)c * fr.n + i] =
                (u & 1u) ? (int32_t)((u + 1u) >> 1) : -(int32_t)(u >> 1);
        }
    }
}

__global__ __launch_bounds__(64) void k_ttad_chain(const Frame *__restrict__ frames,
                                                   const uint32_t *__restrict__ chain_frame,
                                                   uint64_t n_chains,
                                                   const int32_t *__restrict__ status,
                                                   int32_t *__restrict__ resid)
{
    const uint64_t g = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (g >= n_chains)
        return;
    const uint32_t fidx = chain_frame[g];
    if (status[fidx] != ATG_TD_OK)
        return;
    const Frame fr = frames[fidx];
    int32_t *x = resid + fr.sbase + (g - fr.chain0) * fr.n;
    tta::Hybrid h;
    h.reset();
    int32_t rprev = 0, out_prev = 0;
    // the residuals of a group are loaded before the recurrence needs them
    // (tta_encode.hip k_tta_chain)
    constexpr uint32_t kAhead = 8;
    for (uint32_t i0 = 0; i0 < fr.n; i0 += kAhead) {
        int32_t rs[kAhead];
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j)
            rs[j] = i0 + j < fr.n ? x[i0 + j] : 0;
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) {
            const uint32_t i = i0 + j;
            if (i >= fr.n)
                break;
            const int32_t r = rs[j];
            int32_t fv, o;
            if (i == 0) {
                fv = r;
                o = fv;
            } else {
                h.adapt(rprev);
                fv = (int32_t)((uint32_t)r + (uint32_t)h.predict(fr.hshift));
                o = (int32_t)((uint32_t)fv + (uint32_t)tta::fixed_term(out_prev, fr.pshift));
            }
            h.push(fv);
            rprev = r;
            out_prev = o;
            x[i] = o;
        }
    }
}

__global__ __launch_bounds__(256) void k_ttad_out(const Frame *__restrict__ frames,
                                                  uint32_t chunks_per_frame,
                                                  const int32_t *__restrict__ status,
                                                  const int32_t *__restrict__ pred,
                                                  int32_t *__restrict__ pcm)
{
    const uint32_t fidx = blockIdx.x / chunks_per_frame;
    const uint32_t chunk = blockIdx.x % chunks_per_frame;
    const Frame fr = frames[fidx];
    const uint64_t i = (uint64_t)chunk * 256u + threadIdx.x;
    if (i >= fr.n)
        return;
    const uint32_t C = fr.channels;
    const int32_t *p = pred + fr.sbase + i;
    int32_t *o = pcm + fr.pcm_start + i * C; // pcm_start counts samples here
    if (status[fidx] != ATG_TD_OK) { // a bad frame leaves zeros, not stale samples
        for (uint32_t c = 0; c < C; ++c)
            o[c] = 0;
        return;
    }
    if (C == 1) {
        o[0] = p[0];
        return;
    }
    // decorrelate_channels (tta.c:639-681): the last channel first
    const int32_t side = p[(uint64_t)(C - 2) * fr.n];
    uint32_t v = (uint32_t)p[(uint64_t)(C - 1) * fr.n] + (uint32_t)(side / 2);
    o[C - 1] = (int32_t)v;
    for (uint32_t c = C - 1; c-- > 0;) {
        v -= (uint32_t)p[(uint64_t)c * fr.n];
        o[c] = (int32_t)v;
    }
}

// ------------------------------------------------------------------- host
thread_local ErrSlot g_ttad_err;
#define DHIP(expr) ATG_HIP_TRY(g_ttad_err, expr, #expr)

const int kDTimed = 5;
const char *kDNames[kDTimed] = {"ttad_crc", "ttad_parse", "ttad_chain", "ttad_out",
                                "ttad_total"};

uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
uint32_t rd32(const uint8_t *p) { return rd16(p) | (rd16(p + 2) << 16); }

uint32_t host_crc32(const uint8_t *p, uint64_t n)
{
    uint32_t r = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; ++i)
        r = tta::crc_byte_entry((r ^ p[i]) & 0xFFu) ^ (r >> 8);
    return r ^ 0xFFFFFFFFu;
}

} // namespace

struct atg_tta_decoder : StageHandle<kDTimed> {
    DevBuf frames, chain_frame, status, resid, pcm, wide, h_data;
    uint64_t last_samples = 0;
};

namespace {

atg_status ttad_run(atg_tta_decoder *dec, const uint8_t *d_data, uint64_t len,
                    const atg_tta_dec_track *tracks, uint32_t n, atg_tta_dec_result *res,
                    uint64_t *total_samples)
{
    hipStream_t s = dec->s;
    std::vector<Frame> frames;
    std::vector<uint32_t> chain_frame;
    std::vector<uint32_t> first(n), count(n);
    std::vector<int32_t> host_status(n, ATG_TD_OK); // status past the laid-out frames
    uint64_t samples = 0, out_samples = 0;
    uint32_t max_n = 0;
    bool wide = false;
    uint32_t uniform = n ? tracks[0].channels : 0; // 1 or 2 when every track has that many
    for (uint32_t t = 0; t < n; ++t) {
        const atg_tta_dec_track &T = tracks[t];
        if (T.channels < 1 || T.channels > 65535)
            return g_ttad_err.fail(ATG_ERR_INVALID, "channels must be 1..65535");
        if (T.bits_per_sample != 8 && T.bits_per_sample != 16 && T.bits_per_sample != 24)
            return g_ttad_err.fail(ATG_ERR_INVALID, "bits per sample must be 8, 16 or 24");
        if (T.block_size < 1)
            return g_ttad_err.fail(ATG_ERR_INVALID, "block_size must be at least 1");
        if (T.data_offset > len || T.data_bytes > len - T.data_offset)
            return g_ttad_err.fail(ATG_ERR_INVALID, "track data outside the buffer");
        if (T.n_frame_bytes && !T.frame_bytes)
            return g_ttad_err.fail(ATG_ERR_INVALID, "frame_bytes is NULL");
        wide = wide || T.channels > kMaxCh;
        if (T.channels != uniform || T.channels > 2)
            uniform = 0;
        first[t] = (uint32_t)frames.size();
        res[t].sample_offset = out_samples;
        uint64_t pos = T.start, remaining = T.remaining, k = 0;
        while (remaining) {
            const uint32_t nf = (uint32_t)std::min<uint64_t>(remaining, T.block_size);
            // the seektable entry; one missing from the table, or a frame
            // whose bytes are not all in the image, is an I/O error
            if (k >= T.n_frame_bytes || T.frame_bytes[k] < 4 || pos > T.data_bytes ||
                T.frame_bytes[k] > T.data_bytes - pos) {
                host_status[t] = ATG_TD_IO_ERROR;
                break;
            }
            Frame f;
            std::memset(&f, 0, sizeof(f));
            f.pcm_start = out_samples; // in samples: tracks may differ in channels
            f.sbase = samples;
            f.byte_off = T.data_offset + pos;
            f.chain0 = chain_frame.size();
            f.n = nf;
            f.payload = T.frame_bytes[k] - 4;
            f.channels = (uint16_t)T.channels;
            f.hshift = T.bits_per_sample == 16 ? 9 : 10;
            f.pshift = T.bits_per_sample == 8 ? 4 : 5;
            for (uint32_t c = 0; c < T.channels; ++c)
                chain_frame.push_back((uint32_t)frames.size());
            frames.push_back(f);
            if (frames.size() > 0x7FFFFFFFull)
                return g_ttad_err.fail(ATG_ERR_UNSUPPORTED, "too many TTA frames in one batch");
            samples += (uint64_t)nf * T.channels;
            out_samples += (uint64_t)nf * T.channels;
            max_n = std::max(max_n, nf);
            pos += T.frame_bytes[k];
            remaining -= nf;
            ++k;
        }
        count[t] = (uint32_t)frames.size() - first[t];
    }
    const uint64_t nfr = frames.size(), nch = chain_frame.size();
    DHIP(dec->frames.ensure(sizeof(Frame) * std::max<uint64_t>(nfr, 1)));
    DHIP(dec->chain_frame.ensure(sizeof(uint32_t) * std::max<uint64_t>(nch, 1)));
    DHIP(dec->status.ensure(sizeof(int32_t) * std::max<uint64_t>(nfr, 1)));
    DHIP(dec->resid.ensure(sizeof(int32_t) * std::max<uint64_t>(samples, 1)));
    DHIP(dec->pcm.ensure(sizeof(int32_t) * std::max<uint64_t>(out_samples, 1)));
    if (wide)
        DHIP(dec->wide.ensure(sizeof(tta::Rice) * std::max<uint64_t>(nch, 1)));
    if (nfr) {
        DHIP(hipMemcpyAsync(dec->frames.p, frames.data(), sizeof(Frame) * nfr,
                            hipMemcpyHostToDevice, s));
        DHIP(hipMemcpyAsync(dec->chain_frame.p, chain_frame.data(), sizeof(uint32_t) * nch,
                            hipMemcpyHostToDevice, s));
    }
    const Frame *dfr = (const Frame *)dec->frames.p;
    int32_t *dst = (int32_t *)dec->status.p;
    DHIP(hipEventRecord(dec->ev[0], s));
    if (nfr)
        hipLaunchKernelGGL(k_ttad_crc, dim3((unsigned)nfr), dim3(tta::kCrcThreads), 0, s, dfr,
                           d_data, dst);
    DHIP(hipGetLastError());
    DHIP(hipEventRecord(dec->ev[1], s));
    if (nfr) {
        auto kern = uniform == 1 ? k_ttad_parse<1> : uniform == 2 ? k_ttad_parse<2>
                                                                   : k_ttad_parse<0>;
        hipLaunchKernelGGL(kern, dim3((unsigned)((nfr + 63) / 64)), dim3(64), 0, s, dfr,
                           (uint32_t)nfr, d_data, dst, (int32_t *)dec->resid.p,
                           (tta::Rice *)dec->wide.p);
    }
    DHIP(hipGetLastError());
    DHIP(hipEventRecord(dec->ev[2], s));
    if (nch)
        hipLaunchKernelGGL(k_ttad_chain, dim3((unsigned)((nch + 63) / 64)), dim3(64), 0, s, dfr,
                           (const uint32_t *)dec->chain_frame.p, nch, (const int32_t *)dst,
                           (int32_t *)dec->resid.p);
    DHIP(hipGetLastError());
    DHIP(hipEventRecord(dec->ev[3], s));
    if (nfr) {
        const uint64_t per = ((uint64_t)max_n + 255) / 256;
        if (per * nfr > 0x7FFFFFFFull)
            return g_ttad_err.fail(ATG_ERR_UNSUPPORTED, "batch too large for one launch");
        hipLaunchKernelGGL(k_ttad_out, dim3((unsigned)(per * nfr)), dim3(256), 0, s, dfr,
                           (uint32_t)per, (const int32_t *)dst, (const int32_t *)dec->resid.p,
                           (int32_t *)dec->pcm.p);
    }
    DHIP(hipGetLastError());
    DHIP(hipEventRecord(dec->ev[4], s));
    std::vector<int32_t> st(nfr);
    if (nfr)
        DHIP(hipMemcpyAsync(st.data(), dst, sizeof(int32_t) * nfr, hipMemcpyDeviceToHost, s));
    DHIP(hipStreamSynchronize(s));
    dec->finish_times();
    dec->last_samples = out_samples;
    for (uint32_t t = 0; t < n; ++t) {
        atg_tta_dec_result &r = res[t];
        r.first_frame = first[t];
        r.channels = tracks[t].channels;
        r.pcm_frames = 0;
        r.status = ATG_TD_OK;
        uint32_t k = 0;
        for (; k < count[t]; ++k) {
            if (st[first[t] + k] != ATG_TD_OK) {
                r.status = st[first[t] + k];
                break;
            }
            r.pcm_frames += frames[first[t] + k].n;
        }
        if (r.status == ATG_TD_OK)
            r.status = host_status[t];
        r.n_frames = k; // good frames; the bad one is frame n_frames of the track
    }
    if (total_samples)
        *total_samples = out_samples;
    return ATG_OK;
}

} // namespace

extern "C" {

const char *atg_tta_decoder_last_error(void) { return g_ttad_err.msg.c_str(); }

int atg_tta_read_info(const uint8_t *data, uint64_t len, atg_tta_info *info,
                      uint32_t *frame_bytes, uint32_t cap, uint32_t *n_frame_bytes)
{
    if (n_frame_bytes)
        *n_frame_bytes = 0;
    if (!data || !info)
        return ATG_TD_IO_ERROR;
    std::memset(info, 0, sizeof(*info));
    // ID3v2 comments in front of the header: 10-byte header with a
    // sync-safe size, one after another
    uint64_t pos = 0;
    while (len - pos >= 10 && data[pos] == 'I' && data[pos + 1] == 'D' && data[pos + 2] == '3' &&
           data[pos + 3] >= 2 && data[pos + 3] <= 4 &&
           !((data[pos + 6] | data[pos + 7] | data[pos + 8] | data[pos + 9]) & 0x80)) {
        const uint64_t size = ((uint64_t)data[pos + 6] << 21) | ((uint64_t)data[pos + 7] << 14) |
                              ((uint64_t)data[pos + 8] << 7) | data[pos + 9];
        if (10 + size > len - pos) {
            pos = len;
            break;
        }
        pos += 10 + size;
    }
    info->id3_bytes = pos;
    info->stage = 0;
    const uint8_t *h = data + pos;
    const uint64_t left = len - pos;
    // read_header: the fields are parsed before the signature is looked at
    if (left < 18)
        return ATG_TD_IO_ERROR;
    info->channels = rd16(h + 6);
    info->bits_per_sample = rd16(h + 8);
    info->sample_rate = rd32(h + 10);
    info->total_pcm_frames = rd32(h + 14);
    if (std::memcmp(h, "TTA1", 4))
        return ATG_TD_INVALID_SIGNATURE;
    if (rd16(h + 4) != 1)
        return ATG_TD_UNSUPPORTED_FORMAT;
    if (left < 22)
        return ATG_TD_IO_ERROR;
    if (host_crc32(h, 18) != rd32(h + 18))
        return ATG_TD_CRC_MISMATCH;
    info->block_size = (uint32_t)(((uint64_t)info->sample_rate * 256u) / 245u);
    info->stage = 1;
    uint64_t nf = 0;
    if (info->total_pcm_frames) {
        // a zero block size divides by zero in the reference; refuse it
        if (info->block_size == 0)
            return ATG_TD_UNSUPPORTED_FORMAT;
        nf = ((uint64_t)info->total_pcm_frames + info->block_size - 1) / info->block_size;
    }
    info->total_tta_frames = (uint32_t)nf;
    if (left - 22 < 4 * nf + 4)
        return ATG_TD_IO_ERROR;
    const uint8_t *tb = h + 22;
    if (host_crc32(tb, 4 * nf) != rd32(tb + 4 * nf))
        return ATG_TD_CRC_MISMATCH;
    if (frame_bytes)
        for (uint64_t k = 0; k < nf && k < cap; ++k)
            frame_bytes[k] = rd32(tb + 4 * k);
    if (n_frame_bytes)
        *n_frame_bytes = (uint32_t)nf;
    info->frames_offset = pos + 22 + 4 * nf + 4;
    info->stage = 2;
    return ATG_TD_OK;
}

atg_status atg_tta_decoder_create(int device, atg_tta_decoder **out)
{
    return open_handle(device, out, g_ttad_err, "decoder create");
}

void atg_tta_decoder_destroy(atg_tta_decoder *d)
{
    if (!d)
        return;
    d->close({&d->frames, &d->chain_frame, &d->status, &d->resid, &d->pcm, &d->wide, &d->h_data});
    delete d;
}

atg_status atg_tta_decode_device(atg_tta_decoder *d, const void *d_data, uint64_t len,
                                 const atg_tta_dec_track *tracks, uint32_t n,
                                 atg_tta_dec_result *results, const int32_t **d_pcm,
                                 uint64_t *total_samples)
{
    ATG_HANDLE_LOCK(d);
    if (!d || (!tracks && n) || (!results && n) || (!d_data && len))
        return g_ttad_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (((uintptr_t)d_data) & 3)
        return g_ttad_err.fail(ATG_ERR_INVALID, "d_data must be 4-byte aligned");
    DHIP(hipSetDevice(d->device));
    atg_status st = ttad_run(d, (const uint8_t *)d_data, len, tracks, n, results, total_samples);
    if (st == ATG_OK && d_pcm)
        *d_pcm = (const int32_t *)d->pcm.p;
    return st;
}

atg_status atg_tta_decode_host(atg_tta_decoder *d, const uint8_t *data, uint64_t len,
                               const atg_tta_dec_track *tracks, uint32_t n,
                               atg_tta_dec_result *results, uint64_t *total_samples)
{
    ATG_HANDLE_LOCK(d);
    if (!d || (!tracks && n) || (!results && n) || (!data && len))
        return g_ttad_err.fail(ATG_ERR_INVALID, "NULL argument");
    DHIP(hipSetDevice(d->device));
    DHIP(d->h_data.ensure(std::max<uint64_t>(len, 4)));
    if (len)
        DHIP(hipMemcpyAsync(d->h_data.p, data, len, hipMemcpyHostToDevice, d->s));
    return ttad_run(d, (const uint8_t *)d->h_data.p, len, tracks, n, results, total_samples);
}

atg_status atg_tta_decode_fetch(atg_tta_decoder *d, int32_t *pcm, uint64_t pcm_cap)
{
    ATG_HANDLE_LOCK(d);
    if (!d || (!pcm && pcm_cap))
        return g_ttad_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (pcm_cap < d->last_samples)
        return g_ttad_err.fail(ATG_ERR_CAPACITY, "pcm buffer smaller than the decoded batch");
    DHIP(hipSetDevice(d->device));
    if (d->last_samples)
        DHIP(hipMemcpyAsync(pcm, d->pcm.p, sizeof(int32_t) * d->last_samples,
                            hipMemcpyDeviceToHost, d->s));
    DHIP(hipStreamSynchronize(d->s));
    return ATG_OK;
}

int atg_tta_decoder_kernel_times(atg_tta_decoder *d, const char **names, float *ms, int cap)
{
    ATG_HANDLE_LOCK(d);
    return d ? d->report(kDNames, names, ms, cap) : 0;
}

} // extern "C"
