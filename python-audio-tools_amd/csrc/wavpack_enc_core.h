// wavpack_enc_core.h — the WavPack encoder's per-block and per-stream work,
// written once for the kernels of wavpack_encode.hip and for host code.
// Reference: src/encoders/wavpack.c (encode_block :613-866,
// roundtrip_block_parameters :485-522, correlate_1ch/2ch :1097-1284,
// write_bitstream :1431-1539, flush_residual :1553-1625, encode_residual
// :1627-1676, write_sub_block :868-898, write_block_header :542-588).
//
// Where C leaves the reference undefined it is defined here as in
// wavpack_common.h: int sums wrap in uint32_t, apply_weight multiplies in 64
// bits and truncates.
#pragma once
#include "wavpack_common.h"

namespace wve {

constexpr uint32_t kGroup = 16;       // a channel's stride in the work slot is padded to it
constexpr uint32_t kSampleWords = 104; // history values of the 16-term table, both channels

// uniform over a batch
struct EOpts {
    uint32_t channels, mask, bps, rate, rate_code;
    uint32_t passes, joint, false_stereo, wasted;
    uint32_t wave_bytes; // payload of the dummy / RIFF header sub-block
};

// one audio block of one stream.  The host fills the layout; k_wve_prep the
// block's own properties; k_wve_chain_wave bits and n_terms; the host byte_off.
struct EBlock {
    uint64_t pcm_start; // the block's first PCM frame in the batch
    uint64_t slot;      // its work slot (int32 index): two channels of `stride`
    uint64_t byte_off;  // its header in the output
    uint64_t bits;      // length of its bitstream
    uint32_t n, stride;
    uint32_t block_index, total;
    uint32_t crc, track;
    uint8_t first_ch, nch, first, last;
    uint8_t first_of_file, eff, is_false, wasted;
    uint8_t magnitude, n_terms, pad[2];
};

// a block's decorrelation and entropy sub-blocks as the file holds them
struct EMeta {
    int8_t term[wv::kMaxTerms];       // table order
    uint8_t weights[wv::kMaxTerms * 2]; // file order
    int16_t samples[kSampleWords];
    int16_t ent[6];
    int32_t medians[6]; // the state itself: the stored form need not restore to it
    uint32_t n_samples, n_weights;
};

// what a stream carries from block to block
struct EState {
    int32_t w[wv::kMaxTerms][2];
    // 1..8: oldest first; 17/18: [x[-1], x[-2]]; negative: h[.][0][0] is
    // channel 1's last sample, h[.][1][0] channel 0's (as the reference keeps them)
    int32_t h[wv::kMaxTerms][2][8];
    int32_t ent[2][3];
    uint32_t eff;
};

struct EStream {
    uint32_t first_block, n_blocks, step, nch;
};

struct ETables {
    const uint8_t *log2;
    const uint16_t *exp2;
};

// -------------------------------------------------------------------- prep
struct Scan {
    uint32_t or0, or1, amax, neq;
};

WV_HD uint32_t uabs(int32_t v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }

template <typename T>
WV_HD void scan_range(const T *__restrict__ pcm, uint32_t C, const EBlock &b, uint32_t t,
                      uint32_t nt, Scan &s)
{
    const T *src = pcm + b.pcm_start * C + b.first_ch;
    for (uint32_t i = t; i < b.n; i += nt) {
        const int32_t x0 = (int32_t)src[(uint64_t)i * C];
        const int32_t x1 = b.nch == 2 ? (int32_t)src[(uint64_t)i * C + 1] : x0;
        s.or0 |= (uint32_t)x0;
        s.or1 |= (uint32_t)x1;
        const uint32_t a0 = uabs(x0), a1 = uabs(x1);
        s.amax = a0 > s.amax ? a0 : s.amax;
        s.amax = a1 > s.amax ? a1 : s.amax;
        s.neq |= (uint32_t)(x0 != x1);
    }
}

WV_HD uint32_t low_zero_bits(uint32_t v) // of a non-zero value
{
    uint32_t n = 0;
    while (!(v & 1u)) {
        v >>= 1;
        ++n;
    }
    return n;
}

// magnitude is taken before the shift; -w takes the minimum over the coded
// channels, an all-zero channel counting as 0
WV_HD void decide(EBlock &b, const Scan &s, const EOpts &o)
{
    b.eff = (b.nch == 1 || (o.false_stereo && !s.neq)) ? 1 : 2;
    b.is_false = (b.nch == 2 && b.eff == 1) ? 1 : 0;
    b.magnitude = (uint8_t)wv::bit_length(s.amax);
    uint32_t w = 0;
    if (o.wasted) {
        w = s.or0 ? low_zero_bits(s.or0) : 0u;
        if (b.eff == 2) {
            const uint32_t w1 = s.or1 ? low_zero_bits(s.or1) : 0u;
            w = w1 < w ? w1 : w;
        }
    }
    b.wasted = (uint8_t)w;
}

// shift and joint stereo into the work slot
template <typename T>
WV_HD void transform_range(const T *__restrict__ pcm, uint32_t C, const EBlock &b,
                           const EOpts &o, int32_t *__restrict__ work, uint32_t t, uint32_t nt)
{
    const T *src = pcm + b.pcm_start * C + b.first_ch;
    int32_t *x0 = work + b.slot, *x1 = x0 + b.stride;
    const bool joint = b.eff == 2 && o.joint;
    for (uint32_t i = t; i < b.n; i += nt) {
        const int32_t a = (int32_t)src[(uint64_t)i * C] >> b.wasted;
        if (b.eff == 1) {
            x0[i] = a;
            continue;
        }
        const int32_t c = (int32_t)src[(uint64_t)i * C + 1] >> b.wasted;
        x0[i] = joint ? (int32_t)((uint32_t)a - (uint32_t)c) : a;
        x1[i] = joint ? (int32_t)((uint32_t)a + (uint32_t)c) >> 1 : c;
    }
}

WV_HD uint32_t pow3(uint64_t e)
{
    uint32_t r = 1, b = 3;
    for (; e; e >>= 1, b *= b)
        if (e & 1u)
            r *= b;
    return r;
}

// crc = 3 crc + s over the shifted samples in interleaved order is linear:
// the piece [j0, j1) contributes sum s_j 3^(j1-1-j), times 3^(m-j1) in the whole
template <typename T>
WV_HD uint32_t crc_piece(const T *__restrict__ pcm, uint32_t C, const EBlock &b, uint64_t j0,
                         uint64_t j1)
{
    const T *src = pcm + b.pcm_start * C + b.first_ch;
    uint32_t crc = 0;
    for (uint64_t j = j0; j < j1; ++j) {
        const uint64_t i = b.eff == 2 ? j >> 1 : j;
        const uint32_t c = b.eff == 2 ? (uint32_t)(j & 1u) : 0u;
        crc = 3u * crc + (uint32_t)((int32_t)src[i * C + c] >> b.wasted);
    }
    return crc * pow3((uint64_t)b.n * b.eff - j1);
}

// ------------------------------------------------------------------- passes
WV_HD int32_t residual_of(int32_t v, int32_t w, int64_t src)
{
    return (int32_t)((uint32_t)v - (uint32_t)wv::apply_weight(w, src));
}

// ---------------------------------------------------------------- bitstream
struct CountSink {
    uint64_t bits = 0;
    WV_HD void put(uint32_t nbits, uint64_t) { bits += nbits; }
};

// bytes through ordinary stores, least significant bit first
struct ByteSink {
    uint8_t *out;
    uint64_t pos = 0, acc = 0;
    uint32_t fill = 0;
    WV_HD void put(uint32_t nbits, uint64_t value) // nbits <= 33, fill < 8
    {
        acc |= value << fill;
        fill += nbits;
        while (fill >= 8u) {
            out[pos++] = (uint8_t)acc;
            acc >>= 8;
            fill -= 8u;
        }
    }
    WV_HD uint64_t finish()
    {
        if (fill)
            out[pos++] = (uint8_t)acc;
        fill = 0;
        return pos;
    }
};

template <class Sink>
WV_HD void put_unary(Sink &s, uint32_t v) // v <= 32 ones and a zero
{
    s.put(v + 1u, (1ull << v) - 1ull);
}

template <class Sink>
WV_HD void put_egc(Sink &s, uint32_t v)
{
    if (v <= 1u) {
        put_unary(s, v);
        return;
    }
    const uint32_t t = wv::bit_length(v);
    put_unary(s, t);
    s.put(t - 1u, v & ((1u << (t - 1u)) - 1u));
}

constexpr int32_t kUndef = -1;

struct Pending {
    int32_t zeroes, m;
    uint32_t offset, add, sign;
};

template <class Sink>
WV_HD int32_t flush_residual(Sink &s, int32_t u2, const Pending &p, int32_t m_i)
{
    if (p.zeroes != kUndef)
        put_egc(s, (uint32_t)p.zeroes);
    if (p.m == kUndef)
        return kUndef;
    const bool even = u2 == kUndef || (u2 & 1) == 0;
    const bool odd = u2 == kUndef || (u2 & 1) == 1;
    int32_t u;
    if (p.m > 0 && m_i > 0)
        u = even ? p.m * 2 + 1 : p.m * 2 - 1;
    else if (p.m == 0 && m_i > 0)
        u = odd ? 1 : kUndef;
    else if (p.m > 0)
        u = even ? p.m * 2 : (p.m - 1) * 2;
    else
        u = odd ? 0 : kUndef;
    if (u != kUndef) {
        if (u < 16) {
            put_unary(s, (uint32_t)u);
        } else {
            put_unary(s, 16u);
            put_egc(s, (uint32_t)u - 16u);
        }
    }
    if (p.add > 0u) {
        const uint32_t lg = wv::bit_length(p.add) - 1u;
        const uint32_t e = (uint32_t)((1ull << (lg + 1u)) - p.add - 1u);
        if (p.offset < e) {
            s.put(lg, p.offset);
        } else {
            s.put(lg, (p.offset + e) >> 1);
            s.put(1u, (p.offset + e) & 1u);
        }
    }
    s.put(1u, p.sign);
    return u;
}

// the three medians of a channel
struct Medians {
    int32_t a, b, c;
};

WV_HD int32_t madd(int32_t v, int32_t d) { return (int32_t)((uint32_t)v + (uint32_t)d); }

WV_HD void encode_residual(int32_t r, Medians &e, Pending &p)
{
    uint32_t u;
    if (r >= 0) {
        u = (uint32_t)r;
        p.sign = 0;
    } else {
        u = (uint32_t)(-(int64_t)r - 1);
        p.sign = 1;
    }
    const uint32_t m0 = (uint32_t)((e.a >> 4) + 1), m1 = (uint32_t)((e.b >> 4) + 1),
                   m2 = (uint32_t)((e.c >> 4) + 1);
    if (u < m0) {
        p.m = 0;
        p.offset = u;
        p.add = m0 - 1u;
        e.a = madd(e.a, -(madd(e.a, 126) >> 7) * 2);
    } else if (u - m0 < m1) {
        p.m = 1;
        p.offset = u - m0;
        p.add = m1 - 1u;
        e.a = madd(e.a, (madd(e.a, 128) >> 7) * 5);
        e.b = madd(e.b, -(madd(e.b, 62) >> 6) * 2);
    } else if (u - (m0 + m1) < m2) {
        p.m = 2;
        p.offset = u - (m0 + m1);
        p.add = m2 - 1u;
        e.a = madd(e.a, (madd(e.a, 128) >> 7) * 5);
        e.b = madd(e.b, (madd(e.b, 64) >> 6) * 5);
        e.c = madd(e.c, -(madd(e.c, 30) >> 5) * 2);
    } else {
        p.m = (int32_t)((u - (m0 + m1)) / m2 + 2u);
        p.offset = u - (m0 + m1 + ((uint32_t)p.m - 2u) * m2);
        p.add = m2 - 1u;
        e.a = madd(e.a, (madd(e.a, 128) >> 7) * 5);
        e.b = madd(e.b, (madd(e.b, 64) >> 6) * 5);
        e.c = madd(e.c, (madd(e.c, 32) >> 5) * 5);
    }
}

// write_bitstream: the zero-run and deferred-unary state lives for a block,
// the medians for the stream.  The zero-run test reads channel 1's first
// median in one-channel blocks too; starting a run clears both channels'.
template <class Sink>
struct Walker {
    Sink &s;
    Medians e0, e1;
    Pending prev{kUndef, kUndef, 0, 0, 0};
    int32_t u2 = kUndef;

    WV_HD void step(int32_t r, Medians &e)
    {
        const bool undefined =
            prev.m == kUndef || (prev.m == 0 && u2 != kUndef && (u2 & 1) == 0);
        if (e0.a < 2 && e1.a < 2 && undefined) {
            if (prev.zeroes != kUndef && prev.m == kUndef) { // in a run of zeroes
                if (r == 0)
                    ++prev.zeroes;
                else
                    encode_residual(r, e, prev);
            } else if (r == 0) { // a run starts
                u2 = flush_residual(s, u2, prev, 0);
                prev = Pending{1, kUndef, 0, 0, 0};
                e0 = Medians{0, 0, 0};
                e1 = Medians{0, 0, 0};
            } else { // false alarm
                Pending cur{0, kUndef, 0, 0, 0};
                encode_residual(r, e, cur);
                u2 = flush_residual(s, u2, prev, cur.m);
                prev = cur;
            }
        } else {
            Pending cur{kUndef, kUndef, 0, 0, 0};
            encode_residual(r, e, cur);
            u2 = flush_residual(s, u2, prev, cur.m);
            prev = cur;
        }
    }
    WV_HD void end() { flush_residual(s, u2, prev, 0); }
};

template <class Sink>
WV_HD void walk_block(Sink &s, const int32_t *x0, const int32_t *x1, uint32_t n, uint32_t eff,
                      int32_t ent[2][3])
{
    Walker<Sink> wk{s, Medians{ent[0][0], ent[0][1], ent[0][2]},
                    Medians{ent[1][0], ent[1][1], ent[1][2]}};
    for (uint32_t i = 0; i < n; ++i) {
        wk.step(x0[i], wk.e0);
        if (eff == 2)
            wk.step(x1[i], wk.e1);
    }
    wk.end();
    ent[0][0] = wk.e0.a, ent[0][1] = wk.e0.b, ent[0][2] = wk.e0.c;
    ent[1][0] = wk.e1.a, ent[1][1] = wk.e1.b, ent[1][2] = wk.e1.c;
}

// -------------------------------------------------------------------- chain
WV_HD int32_t table_len(uint32_t eff, uint32_t passes)
{
    return passes <= 2u ? (int32_t)passes : ((passes == 5u || eff == 1u) ? 5 : (int32_t)passes);
}

// A stream's block begins: the round trip (or the reset where the coded
// channel count changes) and the sub-blocks that hold the state as of now.
// ent in the entropy sub-block is the state at the block's start: the
// reference writes it before it codes the residuals.  -> number of terms
WV_HD int32_t begin_block(EBlock &b, EMeta &m, EState &st, const ETables &tb, uint32_t passes)
{
    const uint32_t eff = b.eff;
    const int32_t nt = wv::term_table(eff, passes, m.term);
    if (eff == st.eff) {
        for (int32_t p = 0; p < nt; ++p) {
            const uint32_t cnt = wv::term_samples(m.term[p]);
            for (uint32_t c = 0; c < eff; ++c) {
                st.w[p][c] = wv::restore_weight((uint8_t)wv::store_weight(st.w[p][c]));
                for (uint32_t j = 0; j < cnt; ++j)
                    st.h[p][c][j] = wv::roundtrip_value(tb.log2, tb.exp2, st.h[p][c][j]);
            }
        }
        for (uint32_t c = 0; c < eff; ++c)
            for (uint32_t j = 0; j < 3; ++j)
                st.ent[c][j] = wv::roundtrip_value(tb.log2, tb.exp2, st.ent[c][j]);
    } else {
        st.eff = eff;
        for (int32_t p = 0; p < wv::kMaxTerms; ++p)
            for (uint32_t c = 0; c < 2; ++c) {
                st.w[p][c] = 0;
                for (uint32_t j = 0; j < 8; ++j)
                    st.h[p][c][j] = 0;
            }
        for (uint32_t c = 0; c < 2; ++c)
            for (uint32_t j = 0; j < 3; ++j)
                st.ent[c][j] = 0;
    }
    // the sub-blocks, file order: the last table entry first
    uint32_t nw = 0, ns = 0;
    for (int32_t p = nt - 1; p >= 0; --p) {
        const int32_t t = m.term[p];
        for (uint32_t c = 0; c < eff; ++c)
            m.weights[nw++] = (uint8_t)wv::store_weight(st.w[p][c]);
        if (t > 8) {
            for (uint32_t c = 0; c < eff; ++c)
                for (uint32_t j = 0; j < 2; ++j)
                    m.samples[ns++] = (int16_t)wv::log2_value(tb.log2, st.h[p][c][j]);
        } else if (t > 0) {
            for (uint32_t j = 0; j < (uint32_t)t; ++j)
                for (uint32_t c = 0; c < eff; ++c)
                    m.samples[ns++] = (int16_t)wv::log2_value(tb.log2, st.h[p][c][j]);
        } else {
            m.samples[ns++] = (int16_t)wv::log2_value(tb.log2, st.h[p][0][0]);
            m.samples[ns++] = (int16_t)wv::log2_value(tb.log2, st.h[p][1][0]);
        }
    }
    m.n_weights = nw;
    m.n_samples = ns;
    for (uint32_t c = 0; c < eff; ++c)
        for (uint32_t j = 0; j < 3; ++j)
            m.ent[c * 3 + j] = (int16_t)wv::log2_value(tb.log2, st.ent[c][j]);
    for (uint32_t c = 0; c < 2; ++c)
        for (uint32_t j = 0; j < 3; ++j)
            m.medians[c * 3 + j] = st.ent[c][j];
    b.n_terms = (uint8_t)nt;
    return nt;
}

// The passes as a pipeline over the lanes of one wave: pass p at sample
// i needs only its own history and pass p - 1 at i, so lane l runs the l-th
// pass applied (table entry nt - 1 - l) on sample t - l at step t, both
// channels, and lane nt walks the residuals.  A lane's state: the weights and
// one delay line per channel whose front d[0] is the oldest sample the term
// looks at; a new sample goes in at d[ins] after the line moved up by one.
// Every term is the same straight-line code over selects, so the pass lanes
// do not diverge.  The pipeline drains at every block's end: the state
// between blocks is EState, in the reference's own layout.
struct PipeLane {
    int32_t w0, w1, d0[8], d1[8];
    int32_t ins;  // history length - 1
    int32_t kind; // 0: term 1..8, 1: 17, 2: 18, 3: -1, 4: -2, 5: -3

    WV_HD void load(int32_t term, const EState &st, int32_t p)
    {
        w0 = st.w[p][0];
        w1 = st.w[p][1];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            d0[j] = d1[j] = 0;
        if (term > 8) {
            kind = term == 17 ? 1 : 2;
            ins = 1;
            d0[0] = st.h[p][0][1], d0[1] = st.h[p][0][0];
            d1[0] = st.h[p][1][1], d1[1] = st.h[p][1][0];
        } else if (term > 0) {
            kind = 0;
            ins = term - 1;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < term) {
                    d0[j] = st.h[p][0][j];
                    d1[j] = st.h[p][1][j];
                }
        } else {
            kind = 2 - term;
            ins = 0;
            d0[0] = st.h[p][1][0]; // channel 0's last sample
            d1[0] = st.h[p][0][0];
        }
    }

    WV_HD void store(int32_t term, EState &st, int32_t p) const
    {
        st.w[p][0] = w0;
        st.w[p][1] = w1;
        if (term > 8) {
            st.h[p][0][0] = d0[1], st.h[p][0][1] = d0[0];
            st.h[p][1][0] = d1[1], st.h[p][1][1] = d1[0];
        } else if (term > 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < term) {
                    st.h[p][0][j] = d0[j];
                    st.h[p][1][j] = d1[j];
                }
        } else {
            st.h[p][1][0] = d0[0];
            st.h[p][0][0] = d1[0];
        }
    }

    WV_HD void step(int32_t in0, int32_t in1, int32_t &out0, int32_t &out1)
    {
        const uint32_t a0 = (uint32_t)d0[1], a1 = (uint32_t)d1[1];
        const int32_t lin0 = kind == 1 ? (int32_t)(2u * a0 - (uint32_t)d0[0])
                                       : (int32_t)(3u * a0 - (uint32_t)d0[0]) >> 1;
        const int32_t lin1 = kind == 1 ? (int32_t)(2u * a1 - (uint32_t)d1[0])
                                       : (int32_t)(3u * a1 - (uint32_t)d1[0]) >> 1;
        const int32_t s0 = kind == 0 ? d0[0] : (kind <= 2 ? lin0 : (kind == 4 ? in1 : d1[0]));
        const int32_t s1 = kind == 0 ? d1[0] : (kind <= 2 ? lin1 : (kind == 3 ? in0 : d0[0]));
        const int32_t r0 = residual_of(in0, w0, s0);
        const int32_t r1 = residual_of(in1, w1, s1);
        const int32_t n0 = (int32_t)((uint32_t)w0 + (uint32_t)wv::update_weight(s0, r0, wv::kDelta));
        const int32_t n1 = (int32_t)((uint32_t)w1 + (uint32_t)wv::update_weight(s1, r1, wv::kDelta));
        w0 = kind >= 3 ? wv::clamp_weight(n0) : n0;
        w1 = kind >= 3 ? wv::clamp_weight(n1) : n1;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            d0[j] = j == ins ? in0 : d0[j + 1];
            d1[j] = j == ins ? in1 : d1[j + 1];
        }
        d0[7] = ins == 7 ? in0 : d0[7];
        d1[7] = ins == 7 ? in1 : d1[7];
        out0 = r0;
        out1 = r1;
    }
};

// --------------------------------------------------------------------- pack
// bytes of a sub-block with `payload` bytes of data (write_sub_block)
WV_HD uint64_t sub_block_bytes(uint64_t payload) { return (payload > 510u ? 4u : 2u) + payload + (payload & 1u); }

struct Out {
    uint8_t *p;
    uint64_t pos = 0;
    WV_HD void u8(uint32_t v) { p[pos++] = (uint8_t)v; }
    WV_HD void u16(uint32_t v)
    {
        u8(v);
        u8(v >> 8);
    }
    WV_HD void u32(uint32_t v)
    {
        u16(v);
        u16(v >> 16);
    }
    WV_HD void sub_head(uint32_t function, uint32_t nondecoder, uint64_t payload)
    {
        const uint32_t odd = (uint32_t)(payload & 1u);
        const uint32_t words = (uint32_t)(payload / 2u) + odd;
        const uint32_t head = function | (nondecoder << 5) | (odd << 6);
        if (payload > 510u) {
            u8(head | 0x80u);
            u8(words);
            u8(words >> 8);
            u8(words >> 16);
        } else {
            u8(head);
            u8(words);
        }
    }
};

WV_HD uint32_t header_flags(const EOpts &o, uint32_t nch, uint32_t joint, uint32_t n_terms,
                            uint32_t wasted, uint32_t first, uint32_t last, uint32_t magnitude,
                            uint32_t is_false)
{
    return (o.bps / 8u - 1u) | ((2u - nch) << 2) | (joint << 4) | ((n_terms > 5u ? 1u : 0u) << 5) |
           ((wasted ? 1u : 0u) << 8) | (first << 11) | (last << 12) | (magnitude << 18) |
           (o.rate_code << 23) | (is_false << 30);
}

WV_HD void put_header(Out &w, uint32_t sub_bytes, uint32_t total, uint32_t index, uint32_t n,
                      uint32_t flags, uint32_t crc)
{
    w.u8('w'), w.u8('v'), w.u8('p'), w.u8('k');
    w.u32(sub_bytes + 24u);
    w.u16(0x407);
    w.u16(0);
    w.u32(total);
    w.u32(index);
    w.u32(n);
    w.u32(flags);
    w.u32(crc);
}

// bytes of a block's sub-blocks, from what prep and the chain found
WV_HD uint64_t block_sub_bytes(const EBlock &b, const EOpts &o)
{
    uint64_t s = 0;
    if (b.first_of_file)
        s += sub_block_bytes(o.wave_bytes);
    if (b.n_terms) {
        int8_t term[wv::kMaxTerms];
        const int32_t nt = wv::term_table(b.eff, o.passes, term);
        uint32_t ns = 0;
        for (int32_t p = 0; p < nt; ++p)
            ns += term[p] < 0 ? 2u : wv::term_samples(term[p]) * b.eff;
        s += sub_block_bytes((uint64_t)nt) + sub_block_bytes((uint64_t)nt * b.eff) +
             sub_block_bytes(2ull * ns);
    }
    if (b.wasted)
        s += sub_block_bytes(4);
    if (o.channels > 2)
        s += sub_block_bytes(5);
    if (o.rate_code == 15)
        s += sub_block_bytes(4);
    s += sub_block_bytes(6ull * b.eff);
    s += sub_block_bytes((b.bits + 7u) / 8u);
    return s;
}

// one block: header, sub-blocks in the reference's order, the bitstream.
WV_HD void pack_block(const EBlock &b, const EMeta &m, const EOpts &o, const int32_t *work,
                      uint32_t sub_bytes, uint8_t *out)
{
    Out w{out + b.byte_off};
    put_header(w, sub_bytes, b.total, b.block_index, b.n,
               header_flags(o, b.nch, (b.nch == 2 && o.joint) ? 1u : 0u, b.n_terms, b.wasted,
                            b.first, b.last, b.magnitude, b.is_false),
               b.crc);
    if (b.first_of_file) { // the dummy header: the real one goes over it at the end
        w.sub_head(0, 0, o.wave_bytes);
        for (uint32_t k = 0; k < o.wave_bytes; ++k)
            w.u8(0);
    }
    if (b.n_terms) {
        w.sub_head(2, 0, b.n_terms);
        for (int32_t p = (int32_t)b.n_terms - 1; p >= 0; --p)
            w.u8((uint32_t)(m.term[p] + 5) | ((uint32_t)wv::kDelta << 5));
        if (b.n_terms & 1u)
            w.u8(0);
        w.sub_head(3, 0, m.n_weights);
        for (uint32_t k = 0; k < m.n_weights; ++k)
            w.u8(m.weights[k]);
        if (m.n_weights & 1u)
            w.u8(0);
        w.sub_head(4, 0, 2ull * m.n_samples);
        for (uint32_t k = 0; k < m.n_samples; ++k)
            w.u16((uint16_t)m.samples[k]);
    }
    if (b.wasted) {
        w.sub_head(9, 0, 4);
        w.u8(0), w.u8(b.wasted), w.u8(0), w.u8(0);
    }
    if (o.channels > 2) {
        w.sub_head(13, 0, 5);
        w.u8(o.channels);
        w.u32(o.mask);
        w.u8(0);
    }
    if (o.rate_code == 15) {
        w.sub_head(7, 1, 4);
        w.u32(o.rate);
    }
    w.sub_head(5, 0, 6ull * b.eff);
    for (uint32_t k = 0; k < 3u * b.eff; ++k)
        w.u16((uint16_t)m.ent[k]);
    int32_t ent[2][3] = {{m.medians[0], m.medians[1], m.medians[2]},
                         {m.medians[3], m.medians[4], m.medians[5]}};
    const uint64_t payload = (b.bits + 7u) / 8u;
    w.sub_head(10, 0, payload);
    ByteSink bs{w.p + w.pos};
    walk_block(bs, work + b.slot, work + b.slot + b.stride, b.n, b.eff, ent);
    w.pos += bs.finish();
    if (payload & 1u)
        w.u8(0);
}

} // namespace wve
