// wavpack_decode.hip — WavPack (.wv) decoder for a batch of images.
//
// Replaces the reference's audiotools.decoders.WavPackDecoder
// (src/decoders/wavpack.c: WavPackDecoder_init :24-187, the read loop
// :261-361, decode_block :599-811, read_bitstream :1137-1212, read_residual
// :1238-1313, decorrelate_*_pass :1392-1578, undo_extended_integers
// :1840-1880).
//
// A WavPack block carries all its state in its sub-blocks, so blocks decode
// independently and a batch is a flat list of blocks.  The host walks the
// block headers (atg_wv_read_info), groups blocks into sets (one set = one
// PCM frame range over all channels) and refuses a set whose headers do not
// fit the stream (ATG_WVD_INCONSISTENT_BLOCK): that is what bounds every
// slot below by the stream's declared size.  On the device, per block:
//
//   k_wvd_parse   one lane per block: the sub-blocks (terms, weights, history
//                 samples, entropy medians, int32 info) in the reference's
//                 order of checks, then the residual bitstream to the
//                 block's channel-major slot.  Every read is bounded by the
//                 sub-block it belongs to; unary counts and Elias-gamma
//                 lengths are bounded before they are used as shift counts.
//   k_wvd_decorr  one lane per block: all decorrelation passes applied per
//                 sample, the histories of the passes in LDS; then joint
//                 stereo and the block CRC.
//   k_wvd_out     one lane per PCM frame of a block: extended integers,
//                 false stereo, interleave into the track's int32 PCM.
//
// A track's PCM ends before its first bad set.  The trailing MD5 sub-block,
// where there is one, is checked on the host (md5_cpu.h) over the PCM in its
// file byte form.
#include "handle_lock.h"
#include "host_common.h"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/atgpu.h"
#include "bits_lsb.h"
#include "md5_cpu.h"
#include "wavpack_common.h"

namespace {

using wv::Block;
using wv::Params;

// words whole below the batch buffer's length are loaded aligned, the rest by bytes
using BitReader = LsbReader<true>;

// read_egc: an Elias-gamma code; a length beyond 32 bits is refused
__device__ __forceinline__ bool read_egc(BitReader &br, uint32_t &value)
{
    uint32_t t;
    if (!br.unary(t))
        return false;
    if (t <= 1u) {
        value = t;
        return true;
    }
    if (t > 32u)
        return false;
    uint32_t p;
    if (!br.bits(t - 1u, p))
        return false;
    value = (1u << (t - 1u)) + p;
    return true;
}

__device__ __forceinline__ int32_t wadd(int32_t a, int32_t b)
{
    return (int32_t)((uint32_t)a + (uint32_t)b);
}

// read_residual (:1238-1313): `last` is the carried unary count (-1 =
// undefined), e the channel's three medians
__device__ __forceinline__ bool read_residual(BitReader &br, int32_t &last, int32_t *e,
                                              int32_t &out)
{
    uint32_t m;
    if (last < 0 || (last & 1)) {
        uint32_t u;
        if (!br.unary(u))
            return false;
        if (u == 16u) {
            uint32_t x;
            if (!read_egc(br, x))
                return false;
            u += x;
        }
        m = u / 2u + (last < 0 ? 0u : 1u);
        last = (int32_t)(u & 0x7FFFFFFFu);
    } else {
        last = -1;
        m = 0;
    }
    uint32_t base;
    int32_t add;
    const int32_t e0 = e[0], e1 = e[1], e2 = e[2];
    if (m == 0) {
        base = 0;
        add = e0 >> 4;
        e[0] = (int32_t)((uint32_t)e0 - (uint32_t)((wadd(e0, 126) >> 7) * 2));
    } else if (m == 1) {
        base = (uint32_t)((e0 >> 4) + 1);
        add = e1 >> 4;
        e[0] = (int32_t)((uint32_t)e0 + (uint32_t)(wadd(e0, 128) >> 7) * 5u);
        e[1] = (int32_t)((uint32_t)e1 - (uint32_t)((wadd(e1, 62) >> 6) * 2));
    } else if (m == 2) {
        base = (uint32_t)((e0 >> 4) + 1) + (uint32_t)((e1 >> 4) + 1);
        add = e2 >> 4;
        e[0] = (int32_t)((uint32_t)e0 + (uint32_t)(wadd(e0, 128) >> 7) * 5u);
        e[1] = (int32_t)((uint32_t)e1 + (uint32_t)(wadd(e1, 64) >> 6) * 5u);
        e[2] = (int32_t)((uint32_t)e2 - (uint32_t)((wadd(e2, 30) >> 5) * 2));
    } else {
        base = (uint32_t)((e0 >> 4) + 1) + (uint32_t)((e1 >> 4) + 1) +
               (uint32_t)((e2 >> 4) + 1) * (m - 2u);
        add = e2 >> 4;
        e[0] = (int32_t)((uint32_t)e0 + (uint32_t)(wadd(e0, 128) >> 7) * 5u);
        e[1] = (int32_t)((uint32_t)e1 + (uint32_t)(wadd(e1, 64) >> 6) * 5u);
        e[2] = (int32_t)((uint32_t)e2 + (uint32_t)(wadd(e2, 32) >> 5) * 5u);
    }
    uint32_t u;
    if (add == 0) {
        u = base;
    } else {
        const uint32_t p = 31u - (uint32_t)__clz((int)add); // add != 0: 0..31
        const uint32_t ee = (uint32_t)(1ull << (p + 1u)) - (uint32_t)add - 1u;
        uint32_t r, b;
        if (!br.bits(p, r))
            return false;
        if (r >= ee) {
            if (!br.bits(1u, b))
                return false;
            u = base + r * 2u - ee + b;
        } else {
            u = base + r;
        }
    }
    uint32_t sign;
    if (!br.bits(1u, sign))
        return false;
    out = (int32_t)(sign ? ~u : u);
    return true;
}

__device__ __forceinline__ int32_t rd_s16(const uint8_t *p)
{
    return (int32_t)(int16_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8));
}

__global__ __launch_bounds__(64) void k_wvd_parse(const Block *__restrict__ blocks,
                                                  uint32_t n_blocks,
                                                  const uint8_t *__restrict__ data, uint64_t limit,
                                                  const uint16_t *__restrict__ exp2_table,
                                                  Params *__restrict__ params,
                                                  int32_t *__restrict__ status,
                                                  int32_t *__restrict__ resid)
{
    const uint32_t bi = blockIdx.x * 64u + threadIdx.x;
    if (bi >= n_blocks)
        return;
    const Block B = blocks[bi];
    Params &P = params[bi];
    const uint32_t coded = wv::coded_channels(B.flags);
    const uint8_t *d = data + B.byte_off;
    int32_t n_terms = -1;
    bool have_weights = false, have_samples = false, have_entropy = false, have_bits = false;
    uint32_t has_ext = 0;
    int32_t ent[2][3] = {{0, 0, 0}, {0, 0, 0}};
    int32_t st = ATG_WVD_OK;
    uint32_t pos = 0;
    // decode_block's loop runs while bytes of the block are left; a
    // sub-block that does not fit them is an I/O error
    while (pos < B.size && st == ATG_WVD_OK) {
        if (B.size - pos < 2u) {
            st = ATG_WVD_IO_ERROR;
            break;
        }
        const uint32_t id = d[pos];
        const uint32_t hdr = (id & 0x80u) ? 4u : 2u;
        if (B.size - pos < hdr) {
            st = ATG_WVD_IO_ERROR;
            break;
        }
        uint32_t words = d[pos + 1];
        if (hdr == 4u)
            words |= ((uint32_t)d[pos + 2] << 8) | ((uint32_t)d[pos + 3] << 16);
        const uint32_t one_less = (id >> 6) & 1u;
        if ((one_less && words == 0) || (uint64_t)B.size - pos - hdr < 2ull * words) {
            st = ATG_WVD_IO_ERROR;
            break;
        }
        const uint8_t *p = d + pos + hdr;
        const uint32_t len = 2u * words - one_less; // payload bytes
        const uint64_t payload_off = B.byte_off + pos + hdr;
        pos += hdr + 2u * words;
        if (id & 0x20u) // non-decoder data
            continue;
        switch (id & 0x1Fu) {
        case 2: // decorrelation terms and deltas
            if (len > (uint32_t)wv::kMaxTerms) {
                st = ATG_WVD_EXCESSIVE_DECORRELATION_PASSES;
                break;
            }
            n_terms = (int32_t)len;
            have_weights = have_samples = false;
            for (uint32_t i = 0; i < len; ++i) {
                const int32_t t = (int32_t)(p[i] & 31u) - 5;
                P.term[i] = (int8_t)t;
                P.delta[i] = (uint8_t)(p[i] >> 5);
                if (!((t >= -3 && t <= -1) || (t >= 1 && t <= 8) || t == 17 || t == 18)) {
                    st = ATG_WVD_INVALID_DECORRELATION_TERM;
                    break;
                }
            }
            break;
        case 3: { // weights
            if (n_terms < 0) {
                st = ATG_WVD_DECORRELATION_TERMS_MISSING;
                break;
            }
            const uint32_t cnt = len / coded;
            if (cnt > (uint32_t)n_terms) {
                st = ATG_WVD_EXCESSIVE_DECORRELATION_WEIGHTS;
                break;
            }
            for (uint32_t i = 0; i < (uint32_t)n_terms; ++i)
                for (uint32_t c = 0; c < 2u; ++c)
                    P.weight[i][c] =
                        (i < cnt && c < coded) ? wv::restore_weight(p[i * coded + c]) : 0;
            have_weights = true;
            break;
        }
        case 4: { // history samples
            if (n_terms < 0) {
                st = ATG_WVD_DECORRELATION_TERMS_MISSING;
                break;
            }
            uint32_t left = len, q = 0;
            for (int32_t i = 0; i < n_terms && st == ATG_WVD_OK; ++i) {
                const int32_t t = P.term[i];
                if (t < 0 && coded == 1u) {
                    st = ATG_WVD_INVALID_DECORRELATION_TERM;
                    break;
                }
                const uint32_t cnt = t > 8 ? 2u : (t > 0 ? (uint32_t)t : 1u);
                const uint32_t need = cnt * 2u * coded;
                const bool sent = left >= need;
                for (uint32_t k = 0; k < cnt; ++k)
                    for (uint32_t c = 0; c < 2u; ++c) {
                        int32_t v = 0;
                        if (sent && c < coded) {
                            // 17/18: a channel's two values together; else
                            // the channels alternate
                            const uint32_t at = t > 8 ? c * 2u + k : k * coded + c;
                            v = wv::exp2_value(exp2_table, rd_s16(p + q + 2u * at));
                        }
                        P.hist[i][c][k] = v;
                    }
                if (sent) {
                    q += need;
                    left -= need;
                } else {
                    left = 0;
                }
            }
            have_samples = st == ATG_WVD_OK;
            break;
        }
        case 5: // entropy medians
            if (one_less || words != 3u * coded) {
                st = ATG_WVD_INVALID_ENTROPY_VARIABLE_COUNT;
                break;
            }
            for (uint32_t c = 0; c < 2u; ++c)
                for (uint32_t k = 0; k < 3u; ++k)
                    ent[c][k] =
                        c < coded ? wv::exp2_value(exp2_table, rd_s16(p + 2u * (c * 3u + k))) : 0;
            have_entropy = true;
            break;
        case 9: // int32 info
            if (len != 4u) {
                st = ATG_WVD_IO_ERROR;
                break;
            }
            for (uint32_t k = 0; k < 4u; ++k)
                P.ext[k] = p[k];
            has_ext = 1;
            break;
        case 10: { // the residual bitstream (read_bitstream :1137-1212)
            if (!have_entropy) {
                st = ATG_WVD_ENTROPY_VARIABLES_MISSING;
                break;
            }
            BitReader br;
            br.data = data;
            br.pos = payload_off;
            br.end = payload_off + len;
            br.limit = limit;
            int32_t *out = resid + B.rbase;
            const uint64_t total = (uint64_t)coded * B.n;
            const uint32_t sh = coded - 1u; // sample i: channel i & sh, frame i >> sh
            int32_t last = -1;
            uint64_t i = 0;
            bool ok = true;
            while (i < total && ok) {
                if (last < 0 && ent[0][0] < 2 && ent[1][0] < 2) {
                    uint32_t zeroes;
                    ok = read_egc(br, zeroes);
                    if (!ok)
                        break;
                    if (zeroes > 0) {
                        uint64_t z = zeroes;
                        if (z > total - i)
                            z = total - i;
                        for (uint64_t j = 0; j < z; ++j, ++i)
                            out[(i & sh) * B.n + (i >> sh)] = 0;
                        for (uint32_t k = 0; k < 3u; ++k)
                            ent[0][k] = ent[1][k] = 0;
                    }
                    if (i >= total)
                        break;
                }
                const uint32_t c = (uint32_t)(i & sh);
                int32_t r;
                ok = read_residual(br, last, ent[c], r);
                if (ok) {
                    out[(uint64_t)c * B.n + (i >> sh)] = r;
                    ++i;
                }
            }
            if (!ok)
                st = ATG_WVD_IO_ERROR;
            have_bits = ok;
            break;
        }
        default:
            break;
        }
    }
    if (st == ATG_WVD_OK) {
        if (n_terms >= 0 && !have_weights)
            st = ATG_WVD_DECORRELATION_WEIGHTS_MISSING;
        else if (n_terms >= 0 && !have_samples)
            st = ATG_WVD_DECORRELATION_SAMPLES_MISSING;
        else if (!have_bits)
            st = ATG_WVD_RESIDUALS_MISSING;
    }
    P.n_terms = n_terms;
    P.has_ext = has_ext;
    status[bi] = st;
}

constexpr uint32_t kDecorrLanes = 32; // blocks per workgroup: 38 KB of LDS (histories 32, weights 4, terms 2)

// All passes of a block applied sample by sample.  Pass p's output at sample
// i needs pass p's own history (up to 8 samples per channel) and the pass
// before it at i, so nothing but the final value goes back to memory.
__global__ __launch_bounds__(kDecorrLanes) void k_wvd_decorr(const Block *__restrict__ blocks,
                                                             uint32_t n_blocks,
                                                             const Params *__restrict__ params,
                                                             int32_t *__restrict__ status,
                                                             int32_t *__restrict__ resid)
{
    __shared__ int32_t hist[wv::kMaxTerms * 2 * 8][kDecorrLanes];
    __shared__ int32_t wgt[wv::kMaxTerms * 2][kDecorrLanes];
    __shared__ int32_t tdl[wv::kMaxTerms][kDecorrLanes]; // term | delta << 8
    const uint32_t lane = threadIdx.x;
    const uint32_t bi = blockIdx.x * kDecorrLanes + lane;
    if (bi >= n_blocks || status[bi] != ATG_WVD_OK)
        return;
    const Block B = blocks[bi];
    const Params &P = params[bi];
    const uint32_t coded = wv::coded_channels(B.flags);
    const int32_t nt = P.n_terms > 0 ? P.n_terms : 0;
    for (int32_t p = 0; p < nt; ++p) {
        const int32_t t = P.term[p];
        // a negative term in a one-channel block never gets here: k_wvd_parse
        // refuses it when it reads the history samples, which a block with
        // terms must carry
        tdl[p][lane] = (t & 0xFF) | ((int32_t)P.delta[p] << 8);
        for (uint32_t c = 0; c < 2u; ++c) {
            wgt[p * 2 + c][lane] = P.weight[p][c];
            if (t >= 1 && t <= 8) {
                // sample k (oldest first) is out[k - t]: ring slot (k - t) & 7
                for (int32_t k = 0; k < t; ++k)
                    hist[(p * 2 + c) * 8 + ((k - t) & 7)][lane] = P.hist[p][c][k];
            } else if (t > 8) {
                hist[(p * 2 + c) * 8 + 0][lane] = P.hist[p][c][0]; // out[i-1]
                hist[(p * 2 + c) * 8 + 1][lane] = P.hist[p][c][1]; // out[i-2]
            } else {
                // cross-channel terms: channel 0 reads channel 1's last
                // output and the reverse; slot 0 holds out_c[i-1]
                hist[(p * 2 + c) * 8 + 0][lane] = P.hist[p][c ^ 1u][0];
            }
        }
    }
    int32_t *x0 = resid + B.rbase;
    int32_t *x1 = x0 + (coded == 2u ? B.n : 0u);
    const bool joint = coded == 2u && (B.flags & wv::kJoint);
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < B.n; ++i) {
        int32_t a = x0[i];
        int32_t b = coded == 2u ? x1[i] : 0;
        for (int32_t p = nt - 1; p >= 0; --p) {
            const int32_t td = tdl[p][lane];
            const int32_t t = (int32_t)(int8_t)(td & 0xFF);
            const int32_t delta = td >> 8;
            int32_t w0 = wgt[p * 2][lane], w1 = wgt[p * 2 + 1][lane];
            int32_t *h0 = &hist[(p * 2) * 8][lane];
            int32_t *h1 = &hist[(p * 2 + 1) * 8][lane];
            if (t > 0) {
                for (uint32_t c = 0; c < coded; ++c) {
                    int32_t *h = c ? h1 : h0;
                    int32_t &w = c ? w1 : w0;
                    const int32_t in = c ? b : a;
                    int64_t src;
                    const uint32_t slot = (i & 7u) * kDecorrLanes;
                    if (t > 8) {
                        const int64_t n1 = h[0], n2 = h[kDecorrLanes];
                        src = t == 17 ? 2 * n1 - n2 : (3 * n1 - n2) >> 1;
                    } else {
                        src = h[((i - (uint32_t)t) & 7u) * kDecorrLanes];
                    }
                    const int32_t o =
                        (int32_t)((uint32_t)wv::apply_weight(w, src) + (uint32_t)in);
                    w = (int32_t)((uint32_t)w + (uint32_t)wv::update_weight(src, in, delta));
                    if (t > 8) {
                        h[kDecorrLanes] = h[0];
                        h[0] = o;
                    } else {
                        h[slot] = o;
                    }
                    if (c)
                        b = o;
                    else
                        a = o;
                }
            } else {
                const int32_t p0 = h0[0], p1 = h1[0]; // out0[i-1], out1[i-1]
                int32_t o0, o1;
                if (t == -1) {
                    o0 = (int32_t)((uint32_t)wv::apply_weight(w0, p1) + (uint32_t)a);
                    o1 = (int32_t)((uint32_t)wv::apply_weight(w1, o0) + (uint32_t)b);
                    w0 = wv::clamp_weight(w0 + wv::update_weight(p1, a, delta));
                    w1 = wv::clamp_weight(w1 + wv::update_weight(o0, b, delta));
                } else if (t == -2) {
                    o1 = (int32_t)((uint32_t)wv::apply_weight(w1, p0) + (uint32_t)b);
                    o0 = (int32_t)((uint32_t)wv::apply_weight(w0, o1) + (uint32_t)a);
                    w1 = wv::clamp_weight(w1 + wv::update_weight(p0, b, delta));
                    w0 = wv::clamp_weight(w0 + wv::update_weight(o1, a, delta));
                } else {
                    o0 = (int32_t)((uint32_t)wv::apply_weight(w0, p1) + (uint32_t)a);
                    o1 = (int32_t)((uint32_t)wv::apply_weight(w1, p0) + (uint32_t)b);
                    w0 = wv::clamp_weight(w0 + wv::update_weight(p1, a, delta));
                    w1 = wv::clamp_weight(w1 + wv::update_weight(p0, b, delta));
                }
                h0[0] = o0;
                h1[0] = o1;
                a = o0;
                b = o1;
            }
            wgt[p * 2][lane] = w0;
            wgt[p * 2 + 1][lane] = w1;
        }
        if (joint) { // undo_joint_stereo: a = mid, b = side
            const int32_t right = (int32_t)((uint32_t)b - (uint32_t)(a >> 1));
            a = (int32_t)((uint32_t)a + (uint32_t)right);
            b = right;
        }
        crc = 3u * crc + (uint32_t)a;
        x0[i] = a;
        if (coded == 2u) {
            crc = 3u * crc + (uint32_t)b;
            x1[i] = b;
        }
    }
    if (crc != B.crc)
        status[bi] = ATG_WVD_BLOCK_DATA_CRC_MISMATCH;
    else if ((B.flags & wv::kExtended) && !P.has_ext)
        status[bi] = ATG_WVD_EXTENDED_INTEGERS_MISSING;
}

__global__ __launch_bounds__(256) void k_wvd_out(const Block *__restrict__ blocks,
                                                 uint32_t chunks_per_block,
                                                 const Params *__restrict__ params,
                                                 const int32_t *__restrict__ status,
                                                 const int32_t *__restrict__ resid,
                                                 int32_t *__restrict__ pcm)
{
    const uint32_t bi = blockIdx.x / chunks_per_block;
    const uint32_t chunk = blockIdx.x % chunks_per_block;
    const Block B = blocks[bi];
    const uint64_t i = (uint64_t)chunk * 256u + threadIdx.x;
    if (i >= B.n || B.scratch)
        return;
    const uint32_t coded = wv::coded_channels(B.flags), outc = wv::out_channels(B.flags);
    int32_t *o = pcm + B.pcm_base + i * B.track_ch + B.first_ch;
    if (status[bi] != ATG_WVD_OK) { // a bad block leaves zeros, not stale samples
        for (uint32_t c = 0; c < outc; ++c)
            o[c] = 0;
        return;
    }
    uint32_t zb = 0, ob = 0, db = 0;
    if (B.flags & wv::kExtended) {
        const Params &P = params[bi];
        zb = P.ext[1];
        ob = zb ? 0u : P.ext[2];
        db = (zb || ob) ? 0u : P.ext[3];
    }
    for (uint32_t c = 0; c < outc; ++c) {
        uint32_t v = (uint32_t)resid[B.rbase + (uint64_t)(c < coded ? c : 0u) * B.n + i];
        if (zb)
            v <<= (zb & 31u);
        else if (ob)
            v = (v << (ob & 31u)) | ((1u << (ob & 31u)) - 1u);
        else if (db)
            v = (v << (db & 31u)) | ((v & 1u) ? (1u << (db & 31u)) - 1u : 0u);
        o[c] = (int32_t)v;
    }
}

// ------------------------------------------------------------------- host
thread_local ErrSlot g_wvd_err;
#define WHIP(expr) ATG_HIP_TRY(g_wvd_err, expr, #expr)

const int kWTimed = 4;
const char *kWNames[kWTimed] = {"wvd_parse", "wvd_decorr", "wvd_out", "wvd_total"};

uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
uint32_t rd32(const uint8_t *p) { return rd16(p) | (rd16(p + 2) << 16); }

const uint32_t kRates[15] = {6000,  8000,  9600,  11025, 12000, 16000, 22050, 24000,
                             32000, 44100, 48000, 64000, 88200, 96000, 192000};

struct Header {
    uint32_t block_size, total_samples, block_index, block_samples, flags, crc;
};

// read_block_header (:547-597)
int read_header(const uint8_t *data, uint64_t len, uint64_t pos, Header &h)
{
    if (pos > len || len - pos < 32)
        return ATG_WVD_IO_ERROR;
    const uint8_t *p = data + pos;
    h.block_size = rd32(p + 4);
    h.total_samples = rd32(p + 12);
    h.block_index = rd32(p + 16);
    h.block_samples = rd32(p + 20);
    h.flags = rd32(p + 24);
    h.crc = rd32(p + 28);
    if (std::memcmp(p, "wvpk", 4))
        return ATG_WVD_INVALID_BLOCK_ID;
    if (h.flags & wv::kReserved)
        return ATG_WVD_INVALID_RESERVED_BIT;
    return ATG_WVD_OK;
}

// find_sub_block (:1727-1765) in the block whose header is at pos
int find_sub_block(const uint8_t *data, uint64_t len, uint64_t pos, const Header &h,
                   uint32_t function, uint32_t nondecoder, const uint8_t **payload,
                   uint32_t *payload_len)
{
    const uint32_t size = h.block_size - 24u; // wraps as the reference's unsigned does
    if (len - (pos + 32) < size)
        return ATG_WVD_IO_ERROR;
    const uint8_t *d = data + pos + 32;
    uint32_t at = 0;
    while (at < size) {
        if (size - at < 2)
            return ATG_WVD_IO_ERROR;
        const uint32_t id = d[at];
        const uint32_t hdr = (id & 0x80u) ? 4u : 2u;
        if (size - at < hdr)
            return ATG_WVD_IO_ERROR;
        uint32_t words = d[at + 1];
        if (hdr == 4)
            words |= ((uint32_t)d[at + 2] << 8) | ((uint32_t)d[at + 3] << 16);
        const uint32_t one_less = (id >> 6) & 1u;
        if ((one_less && words == 0) || (uint64_t)size - at - hdr < 2ull * words)
            return ATG_WVD_IO_ERROR;
        if ((id & 31u) == function && ((id >> 5) & 1u) == nondecoder) {
            *payload = d + at + hdr;
            *payload_len = 2u * words - one_less;
            return ATG_WVD_OK;
        }
        at += hdr + 2u * words;
    }
    return ATG_WVD_SUB_BLOCK_NOT_FOUND;
}

uint32_t rd_le(const uint8_t *p, uint32_t n)
{
    uint32_t v = 0;
    for (uint32_t k = 0; k < n && k < 4; ++k)
        v |= (uint32_t)p[k] << (8 * k);
    return v;
}

} // namespace

struct atg_wv_decoder : StageHandle<kWTimed> {
    DevBuf blocks, params, status, resid, pcm, table, h_data;
    uint64_t last_samples = 0;
};

namespace {

atg_status wvd_run(atg_wv_decoder *dec, const uint8_t *d_data, uint64_t len,
                   const atg_wv_dec_track *tracks, uint32_t n, atg_wv_dec_result *res,
                   uint64_t *total_samples)
{
    hipStream_t s = dec->s;
    std::vector<Block> blocks;
    std::vector<uint32_t> first(n), count(n), set_blocks; // blocks of every set, batch-wide
    std::vector<uint32_t> first_set(n);
    uint64_t slots = 0, out_samples = 0;
    uint32_t max_n = 0;
    for (uint32_t t = 0; t < n; ++t) {
        const atg_wv_dec_track &T = tracks[t];
        if (T.channels < 1 || T.channels > 256)
            return g_wvd_err.fail(ATG_ERR_INVALID, "channels must be 1..256");
        if (T.bits_per_sample != 8 && T.bits_per_sample != 16 && T.bits_per_sample != 24 &&
            T.bits_per_sample != 32)
            return g_wvd_err.fail(ATG_ERR_INVALID, "bits per sample must be 8, 16, 24 or 32");
        if (T.data_offset > len || T.data_bytes > len - T.data_offset || (T.data_offset & 3))
            return g_wvd_err.fail(ATG_ERR_INVALID,
                                  "track data outside the buffer or not 4-byte aligned");
        if (T.n_blocks && !T.blocks)
            return g_wvd_err.fail(ATG_ERR_INVALID, "blocks is NULL");
        if (T.tail_blocks > T.n_blocks)
            return g_wvd_err.fail(ATG_ERR_INVALID, "tail_blocks exceeds n_blocks");
        first[t] = (uint32_t)blocks.size();
        first_set[t] = (uint32_t)set_blocks.size();
        res[t].sample_offset = out_samples;
        // the table is checked again here: a slot is sized by the set's
        // first block and every block of the set must agree with it
        uint32_t k = 0, chans = 0, in_set = 0, set_n = 0;
        uint64_t frames = 0, set_base = out_samples;
        const uint32_t body = T.n_blocks - T.tail_blocks;
        for (; k < T.n_blocks; ++k) {
            const atg_wv_block &S = T.blocks[k];
            const bool tail = k >= body;
            if (S.offset > T.data_bytes || T.data_bytes - S.offset < 32 ||
                T.data_bytes - S.offset - 32 < S.size)
                return g_wvd_err.fail(ATG_ERR_INVALID, "block outside its image");
            if (k == body && in_set)
                return g_wvd_err.fail(ATG_ERR_INVALID, "the last set has no final block");
            if (tail && (S.flags & wv::kFinal))
                return g_wvd_err.fail(ATG_ERR_INVALID,
                                      "a tail block cannot be a set's final block");
            if (in_set == 0) {
                set_n = S.block_samples;
                chans = 0;
                set_base = out_samples;
            } else if (S.block_samples != set_n) {
                return g_wvd_err.fail(ATG_ERR_INVALID, "blocks of a set disagree on block_samples");
            }
            const uint32_t oc = wv::out_channels(S.flags);
            if (chans + oc > T.channels)
                return g_wvd_err.fail(ATG_ERR_INVALID, "a set has more channels than its track");
            frames += in_set == 0 && !tail ? set_n : 0;
            if (frames > 0xFFFFFFFFull || set_n > 0x7FFFFFFFu)
                return g_wvd_err.fail(ATG_ERR_INVALID,
                                      "track longer than a WavPack stream can declare");
            Block b;
            std::memset(&b, 0, sizeof(b));
            b.byte_off = T.data_offset + S.offset + 32;
            b.rbase = slots;
            b.pcm_base = set_base;
            b.size = S.size;
            b.n = set_n;
            b.flags = S.flags;
            b.crc = S.crc;
            b.first_ch = (uint16_t)chans;
            b.track_ch = (uint16_t)T.channels;
            b.scratch = tail ? 1u : 0u;
            blocks.push_back(b);
            if (blocks.size() > 0x7FFFFFFFull)
                return g_wvd_err.fail(ATG_ERR_UNSUPPORTED, "too many WavPack blocks in one batch");
            slots += (uint64_t)set_n * wv::coded_channels(S.flags);
            max_n = std::max(max_n, set_n);
            chans += oc;
            ++in_set;
            if (!tail && (S.flags & wv::kFinal)) {
                if (chans != T.channels)
                    return g_wvd_err.fail(ATG_ERR_INVALID,
                                          "a set does not add up to the channel count");
                set_blocks.push_back(in_set);
                out_samples += (uint64_t)set_n * T.channels;
                in_set = 0;
            }
        }
        if (in_set && T.tail_blocks == 0)
            return g_wvd_err.fail(ATG_ERR_INVALID, "the last set has no final block");
        count[t] = (uint32_t)blocks.size() - first[t];
    }
    const uint64_t nb = blocks.size();
    WHIP(dec->blocks.ensure(sizeof(Block) * std::max<uint64_t>(nb, 1)));
    WHIP(dec->params.ensure(sizeof(Params) * std::max<uint64_t>(nb, 1)));
    WHIP(dec->status.ensure(sizeof(int32_t) * std::max<uint64_t>(nb, 1)));
    WHIP(dec->resid.ensure(sizeof(int32_t) * std::max<uint64_t>(slots, 1)));
    WHIP(dec->pcm.ensure(sizeof(int32_t) * std::max<uint64_t>(out_samples, 1)));
    if (nb)
        WHIP(hipMemcpyAsync(dec->blocks.p, blocks.data(), sizeof(Block) * nb,
                            hipMemcpyHostToDevice, s));
    const Block *dbl = (const Block *)dec->blocks.p;
    int32_t *dst = (int32_t *)dec->status.p;
    WHIP(hipEventRecord(dec->ev[0], s));
    if (nb)
        hipLaunchKernelGGL(k_wvd_parse, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, s, dbl,
                           (uint32_t)nb, d_data, len, (const uint16_t *)dec->table.p,
                           (Params *)dec->params.p, dst, (int32_t *)dec->resid.p);
    WHIP(hipGetLastError());
    WHIP(hipEventRecord(dec->ev[1], s));
    if (nb)
        hipLaunchKernelGGL(k_wvd_decorr, dim3((unsigned)((nb + kDecorrLanes - 1) / kDecorrLanes)),
                           dim3(kDecorrLanes), 0, s, dbl, (uint32_t)nb,
                           (const Params *)dec->params.p, dst, (int32_t *)dec->resid.p);
    WHIP(hipGetLastError());
    WHIP(hipEventRecord(dec->ev[2], s));
    if (nb && max_n) {
        const uint64_t per = ((uint64_t)max_n + 255) / 256;
        if (per * nb > 0x7FFFFFFFull)
            return g_wvd_err.fail(ATG_ERR_UNSUPPORTED, "batch too large for one launch");
        hipLaunchKernelGGL(k_wvd_out, dim3((unsigned)(per * nb)), dim3(256), 0, s, dbl,
                           (uint32_t)per, (const Params *)dec->params.p, (const int32_t *)dst,
                           (const int32_t *)dec->resid.p, (int32_t *)dec->pcm.p);
    }
    WHIP(hipGetLastError());
    WHIP(hipEventRecord(dec->ev[3], s));
    std::vector<int32_t> st(nb);
    if (nb)
        WHIP(hipMemcpyAsync(st.data(), dst, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, s));
    WHIP(hipStreamSynchronize(s));
    dec->finish_times();
    dec->last_samples = out_samples;
    std::vector<int32_t> hashed;
    for (uint32_t t = 0; t < n; ++t) {
        const atg_wv_dec_track &T = tracks[t];
        atg_wv_dec_result &r = res[t];
        r.channels = T.channels;
        r.pcm_frames = 0;
        r.n_sets = 0;
        r.status = ATG_WVD_OK;
        r.reserved = 0;
        uint32_t k = 0;
        // whole sets first: a set is good when every block of it is
        for (uint32_t sidx = first_set[t];
             sidx < (t + 1 < n ? first_set[t + 1] : (uint32_t)set_blocks.size()); ++sidx) {
            for (uint32_t j = 0; j < set_blocks[sidx] && r.status == ATG_WVD_OK; ++j)
                r.status = st[first[t] + k + j];
            if (r.status != ATG_WVD_OK)
                break;
            r.pcm_frames += blocks[first[t] + k].n;
            r.n_sets += 1;
            k += set_blocks[sidx];
        }
        // then the readable blocks of the set the host stopped in, then
        // what stopped it
        if (r.status == ATG_WVD_OK)
            for (k = count[t] - T.tail_blocks; k < count[t] && r.status == ATG_WVD_OK; ++k)
                r.status = st[first[t] + k];
        if (r.status == ATG_WVD_OK)
            r.status = T.end_status;
        if (r.status == ATG_WVD_OK && T.check_md5) {
            // the PCM in its file byte form: clamped to the width as the
            // reference's converter does, little endian
            const uint64_t ns = r.pcm_frames * T.channels;
            hashed.resize(std::max<uint64_t>(ns, 1));
            if (ns)
                WHIP(hipMemcpy(hashed.data(), (const int32_t *)dec->pcm.p + r.sample_offset,
                               sizeof(int32_t) * ns, hipMemcpyDeviceToHost));
            const uint32_t bits = T.bits_per_sample;
            if (bits < 32) {
                const int32_t hi = (int32_t)((1u << (bits - 1)) - 1u), lo = -hi - 1;
                // check_md5 2: 8-bit samples as unsigned bytes
                const int32_t bias = (bits == 8 && T.check_md5 == 2) ? 128 : 0;
                for (uint64_t i = 0; i < ns; ++i)
                    hashed[i] = std::min(std::max(hashed[i], lo), hi) + bias;
            }
            uint8_t sum[16];
            md5cpu::hash_s32(hashed.data(), ns, bits / 8, sum);
            if (std::memcmp(sum, T.md5, 16))
                r.status = ATG_WVD_MD5_MISMATCH;
        }
    }
    if (total_samples)
        *total_samples = out_samples;
    return ATG_OK;
}

} // namespace

extern "C" {

const char *atg_wv_decoder_last_error(void) { return g_wvd_err.msg.c_str(); }

int atg_wv_read_info(const uint8_t *data, uint64_t len, atg_wv_info *info, atg_wv_block *blocks,
                     uint32_t cap, uint32_t *n_blocks)
{
    if (n_blocks)
        *n_blocks = 0;
    if (!data || !info)
        return ATG_WVD_IO_ERROR;
    std::memset(info, 0, sizeof(*info));
    Header h;
    int st = read_header(data, len, 0, h);
    if (st)
        return st;
    const uint8_t *p = nullptr;
    uint32_t plen = 0;
    // WavPackDecoder_init (:108-175): rate, then channels, each from a
    // sub-block of the first block where the header does not say
    const uint32_t rate_code = (h.flags >> 23) & 15u;
    if (rate_code < 15) {
        info->sample_rate = kRates[rate_code];
    } else {
        st = find_sub_block(data, len, 0, h, 7, 1, &p, &plen);
        if (st == ATG_WVD_SUB_BLOCK_NOT_FOUND)
            return ATG_WVD_SAMPLE_RATE_UNDEFINED;
        if (st)
            return st;
        info->sample_rate = rd_le(p, plen);
    }
    static const uint32_t kBits[4] = {8, 16, 24, 32};
    info->bits_per_sample = kBits[h.flags & 3u];
    if (h.flags & wv::kFinal) {
        info->channels = wv::out_channels(h.flags);
        info->channel_mask = info->channels == 2 ? 0x3 : 0x4;
    } else {
        st = find_sub_block(data, len, 0, h, 13, 0, &p, &plen);
        if (st == ATG_WVD_SUB_BLOCK_NOT_FOUND)
            return ATG_WVD_CHANNELS_UNDEFINED;
        if (st)
            return st;
        if (plen < 2)
            return ATG_WVD_IO_ERROR;
        info->channels = p[0];
        if (info->channels == 0) // no set could add up to it: not a stream to open
            return ATG_WVD_CHANNELS_UNDEFINED;
        info->channel_mask = rd_le(p + 1, plen - 1);
    }
    info->total_pcm_frames = h.total_samples;
    // the read loop (:276-311), with the layout checks the reference leaves out
    uint64_t pos = 0;
    uint32_t remaining = h.total_samples, expected = h.block_index, nb = 0, sets = 0;
    int end = ATG_WVD_OK;
    uint32_t tail = 0;
    while (remaining > 0 && end == ATG_WVD_OK) {
        uint64_t at = pos;
        uint32_t chans = 0, in_set = 0, set_n = 0;
        for (;;) {
            st = read_header(data, len, at, h);
            if (st) {
                end = st;
                break;
            }
            if (in_set == 0) {
                if (h.block_index != expected || h.block_samples > remaining ||
                    h.block_samples > 0x7FFFFFFFu) {
                    end = ATG_WVD_INCONSISTENT_BLOCK;
                    break;
                }
                set_n = h.block_samples;
            } else if (h.block_samples != set_n) {
                end = ATG_WVD_INCONSISTENT_BLOCK;
                break;
            }
            const uint32_t oc = wv::out_channels(h.flags);
            if (chans + oc > info->channels) {
                end = ATG_WVD_INCONSISTENT_BLOCK;
                break;
            }
            const uint32_t size = h.block_size - 24u;
            if (len - (at + 32) < size) {
                end = ATG_WVD_BLOCK_DATA_IO;
                break;
            }
            if (blocks && nb + in_set < cap) {
                atg_wv_block &B = blocks[nb + in_set];
                B.offset = at;
                B.size = size;
                B.block_index = h.block_index;
                B.block_samples = h.block_samples;
                B.flags = h.flags;
                B.crc = h.crc;
                B.set = sets;
                B.first_channel = chans;
            }
            chans += oc;
            ++in_set;
            at += 32ull + size;
            if (h.flags & wv::kFinal) {
                if (chans != info->channels)
                    end = ATG_WVD_INCONSISTENT_BLOCK;
                break;
            }
        }
        if (end == ATG_WVD_INCONSISTENT_BLOCK)
            break; // the set is refused whole
        nb += in_set;
        if (end != ATG_WVD_OK) {
            tail = in_set; // readable blocks of the set that a header or a short file ended
            break;
        }
        ++sets;
        pos = at;
        expected += set_n;
        remaining -= std::min(set_n, remaining);
    }
    info->n_sets = sets;
    info->n_blocks = nb;
    info->tail_blocks = tail;
    info->end_status = end;
    info->end_offset = pos;
    if (end == ATG_WVD_OK && read_header(data, len, pos, h) == ATG_WVD_OK &&
        find_sub_block(data, len, pos, h, 6, 1, &p, &plen) == ATG_WVD_OK && plen == 16) {
        info->has_md5 = 1;
        std::memcpy(info->md5, p, 16);
    }
    if (n_blocks)
        *n_blocks = nb;
    return ATG_WVD_OK;
}

atg_status atg_wv_decoder_create(int device, atg_wv_decoder **out)
{
    atg_status st = open_handle(device, out, g_wvd_err, "decoder create");
    if (st != ATG_OK)
        return st;
    atg_wv_decoder *d = *out;
    hipError_t err = d->table.ensure(sizeof(uint16_t) * 256);
    if (err == hipSuccess) {
        // the exponent table of the 16-bit log form: floor(256 * 2^(i/256) + 0.5)
        uint16_t table[256];
        for (int i = 0; i < 256; ++i)
            table[i] = (uint16_t)std::floor(256.0 * std::exp2(i / 256.0) + 0.5);
        err = hipMemcpy(d->table.p, table, sizeof(table), hipMemcpyHostToDevice);
    }
    if (err != hipSuccess) {
        *out = nullptr;
        atg_wv_decoder_destroy(d);
        return g_wvd_err.fail(ATG_ERR_DEVICE,
                              std::string("decoder create: ") + hipGetErrorString(err));
    }
    return ATG_OK;
}

void atg_wv_decoder_destroy(atg_wv_decoder *d)
{
    if (!d)
        return;
    d->close({&d->blocks, &d->params, &d->status, &d->resid, &d->pcm, &d->table, &d->h_data});
    delete d;
}

atg_status atg_wv_decode_device(atg_wv_decoder *d, const void *d_data, uint64_t len,
                                const atg_wv_dec_track *tracks, uint32_t n,
                                atg_wv_dec_result *results, const int32_t **d_pcm,
                                uint64_t *total_samples)
{
    ATG_HANDLE_LOCK(d);
    if (!d || (!tracks && n) || (!results && n) || (!d_data && len))
        return g_wvd_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (((uintptr_t)d_data) & 3)
        return g_wvd_err.fail(ATG_ERR_INVALID, "d_data must be 4-byte aligned");
    WHIP(hipSetDevice(d->device));
    atg_status st = wvd_run(d, (const uint8_t *)d_data, len, tracks, n, results, total_samples);
    if (st == ATG_OK && d_pcm)
        *d_pcm = (const int32_t *)d->pcm.p;
    return st;
}

atg_status atg_wv_decode_host(atg_wv_decoder *d, const uint8_t *data, uint64_t len,
                              const atg_wv_dec_track *tracks, uint32_t n,
                              atg_wv_dec_result *results, uint64_t *total_samples)
{
    ATG_HANDLE_LOCK(d);
    if (!d || (!tracks && n) || (!results && n) || (!data && len))
        return g_wvd_err.fail(ATG_ERR_INVALID, "NULL argument");
    WHIP(hipSetDevice(d->device));
    WHIP(d->h_data.ensure(std::max<uint64_t>(len, 4)));
    if (len)
        WHIP(hipMemcpyAsync(d->h_data.p, data, len, hipMemcpyHostToDevice, d->s));
    return wvd_run(d, (const uint8_t *)d->h_data.p, len, tracks, n, results, total_samples);
}

atg_status atg_wv_decode_fetch(atg_wv_decoder *d, int32_t *pcm, uint64_t pcm_cap)
{
    ATG_HANDLE_LOCK(d);
    if (!d || (!pcm && pcm_cap))
        return g_wvd_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (pcm_cap < d->last_samples)
        return g_wvd_err.fail(ATG_ERR_CAPACITY, "pcm buffer smaller than the decoded batch");
    WHIP(hipSetDevice(d->device));
    if (d->last_samples)
        WHIP(hipMemcpyAsync(pcm, d->pcm.p, sizeof(int32_t) * d->last_samples,
                            hipMemcpyDeviceToHost, d->s));
    WHIP(hipStreamSynchronize(d->s));
    return ATG_OK;
}

int atg_wv_decoder_kernel_times(atg_wv_decoder *d, const char **names, float *ms, int cap)
{
    ATG_HANDLE_LOCK(d);
    return d ? d->report(kWNames, names, ms, cap) : 0;
}

} // extern "C"
