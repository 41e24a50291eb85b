// mlp_common.h — what the MLP kernels share: the data of
// the format (CRC-8 polynomial, the three codebooks, the channel order), the
// bit reader, the access-unit record, the check data, the substream parser
// and the per-frame arithmetic of the reference's src/decoders/mlp.c.  Plain
// C++ over byte pointers, host and device alike.
#pragma once
#include <stdint.h>

#include "aob_common.h"

#define MLP_HD AOB_HD

constexpr uint32_t kMlpChannels = 6; // max_matrix_channel <= 5 (a limit)
constexpr uint32_t kMlpMatrices = 6;
constexpr uint8_t kMlpNotReached = 0xFF;

// CRC-8 of the check data: polynomial 0x63, most significant bit first
struct MlpCrc {
    uint8_t t[256];
};
constexpr MlpCrc mlp_crc_table()
{
    MlpCrc c = {};
    for (int i = 0; i < 256; ++i) {
        uint32_t v = (uint32_t)i;
        for (int k = 0; k < 8; ++k)
            v = (v & 0x80) ? ((v << 1) ^ 0x63) & 0xFF : v << 1;
        c.t[i] = (uint8_t)v;
    }
    return c;
}

// MLP channel c of assignment ca is RIFF WAVE channel mlp_wave_channel(ca, c):
// the identity but for 18, 19 (0 1 3 4 2) and 20 (0 1 4 5 2 3)
MLP_HD inline uint32_t mlp_wave_channel(uint32_t ca, uint32_t c)
{
    const uint32_t t = ca == 20 ? 0x325410u : (ca == 18 || ca == 19) ? 0x524310u : 0x543210u;
    return (t >> (4 * c)) & 15u;
}

// The three codebooks are one family.  Codebook k (1..3), e = 3 - k extra
// bits:  1 b(e)          -> 7 + b
//        01 0{z} 1       -> 7 + 2^e + z   (z = 0..6)
//        00 0{z} 1       -> 6 - z         (z = 0..6)
//        01 0000000, 00 0000000           invalid
// 18, 16 and 15 valid codewords of at most 9 bits.  From the 9 bits at the
// reader's position (zero padded): the value, or -1, and the code's length.
MLP_HD inline int mlp_codeword(uint32_t k, uint32_t w9, uint32_t *len)
{
    const uint32_t e = 3 - k;
    if (w9 & 0x100) {
        *len = 1 + e;
        return 7 + (int)((w9 >> (8 - e)) & ((1u << e) - 1));
    }
    const uint32_t low = w9 & 0x7F;
    if (!low) {
        *len = 9;
        return -1;
    }
    uint32_t z = 0;
    while (!(low & (0x40u >> z)))
        ++z;
    *len = 3 + z;
    return (w9 & 0x80) ? 7 + (1 << e) + (int)z : 6 - (int)z;
}

// big-endian bit reader over n bytes; a read past the end sets eof and gives 0
struct MlpBits {
    const uint8_t *p;
    uint32_t n_bits, pos;
    bool eof;
    MLP_HD MlpBits(const uint8_t *data, uint32_t n_bytes) : p(data), n_bits(8 * n_bytes), pos(0), eof(false) {}
    // the 24 bits at pos, zero padded past the end
    MLP_HD uint32_t peek24() const
    {
        const uint32_t b = pos >> 3, nb = n_bits >> 3;
        uint32_t w = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            w = (w << 8) | (b + i < nb ? p[b + i] : 0u);
        return (w << (pos & 7)) >> 8;
    }
    MLP_HD uint32_t read(uint32_t k)
    {
        if (eof || k > n_bits - pos) {
            eof = true;
            return 0;
        }
        if (!k)
            return 0;
        const uint32_t v = peek24() >> (24 - k); // k <= 24 for every field that fits
        pos += k;
        return v;
    }
    // the reference's read_signed: a sign bit, then k - 1 bits (k = 0 asks
    // for 2^32 - 1 bits, which is an I/O error)
    MLP_HD int32_t read_signed(uint32_t k)
    {
        const uint32_t s = read(1);
        const uint32_t v = read(k - 1);
        return eof ? 0 : (int32_t)(v - (s << (k - 1)));
    }
};

struct MlpChan {
    int32_t fir[8], iir[8], iir_state[8];
    int32_t offset;
    uint8_t fir_n, iir_n, fir_shift, iir_shift, codebook, lsbs, iir_set, pad;
};

struct MlpMatrix {
    int32_t coeff[8];
    uint8_t out, bypass, pad[2];
};

// one substream's parser state between restart headers
struct MlpState {
    MlpChan ch[kMlpChannels];
    MlpMatrix m[kMlpMatrices];
    uint32_t seed, block_size, n_matrices;
    uint8_t out_shift[8], quant[8];
    uint8_t started, lo, hi, mmc, noise_shift, flags, pad[2];
};

// what a worker knows of its title and substream
struct MlpWho {
    uint32_t index, substreams, channels;
    uint32_t range0; // lo | hi << 8 | mmc << 16 of the title's first restart header
};

// records of the storing parse
struct MlpChanRec {
    int32_t fir[8], iir[8], iir_state[8];
    uint8_t fir_n, iir_n, shift, quant, iir_set, pad[3];
};
struct MlpBlockRec {
    uint32_t frames, pad;
    MlpChanRec ch[kMlpChannels]; // channel lo + i of the substream
};
struct MlpUnitRec {
    uint32_t seed, frames;
    uint8_t n_matrices, noise_shift, mmc, noise; // noise: a matrix uses it
    uint8_t out_shift[8], quant[8];
    MlpMatrix m[kMlpMatrices];
};
// what the sizing parse leaves per (unit, substream)
struct MlpSize {
    uint16_t frames, blocks;
    uint8_t status, lo, hi, mmc;
};

MLP_HD inline uint32_t mlp_next_seed(uint32_t seed)
{
    const uint32_t shifted = (seed >> 7) & 0xFFFF;
    return (seed << 16) ^ shifted ^ (shifted << 5);
}

MLP_HD inline int32_t mlp_mask(int32_t x, uint32_t q) { return (int32_t)((uint32_t)(x >> q) << q); }

// ---- the access-unit record (everything but offset and size, which the walk
// found): s is the title's payload stream, u->offset / u->size are set
MLP_HD inline void mlp_fill_unit(const uint8_t *s, bool first, bool have0, const uint8_t *key0,
                                 atg_mlp_unit *u)
{
    const uint8_t *b = s + u->offset;
    const uint32_t size = u->size;
    uint32_t p = 4, status = ATG_MLP_OK, flags = 0;
    u->substream_end[0] = u->substream_end[1] = 0;
    u->substream_flags[0] = u->substream_flags[1] = 0;
    for (int i = 0; i < 8; ++i)
        u->reserved[i] = 0;
    if (size >= 32 && b[4] == 0xF8 && b[5] == 0x72 && b[6] == 0x6F && b[7] == 0xBB) {
        flags |= 1;
        p = 32;
        const uint32_t count = b[20] >> 4;
        if (count != 1 && count != 2)
            status = ATG_MLP_INVALID_MAJOR_SYNC;
        else if (first || (have0 && b[8] == key0[0] && b[9] == key0[1] &&
                           (b[11] & 31) == key0[2] && count == key0[3]))
            flags |= 2;
        else if (have0)
            status = ATG_MLP_INVALID_MAJOR_SYNC;
    }
    if (!have0)
        status = ATG_MLP_UNSUPPORTED;
    const uint32_t nss = have0 && (key0[3] == 1 || key0[3] == 2) ? key0[3] : 0;
    if (status == ATG_MLP_OK)
        for (uint32_t k = 0; k < nss; ++k) {
            if (p + 2 > size) {
                status = ATG_MLP_IO_ERROR;
                break;
            }
            const uint32_t info = ((uint32_t)b[p] << 8) | b[p + 1];
            p += 2;
            u->substream_flags[k] = (uint8_t)((info >> 15) | ((info >> 12) & 2));
            u->substream_end[k] = (uint16_t)(2 * (info & 0xFFF));
            if (info >> 15) {
                status = ATG_MLP_INVALID_EXTRAWORD;
                break;
            }
        }
    u->data_start = (uint16_t)p;
    if (status == ATG_MLP_OK) {
        uint32_t a = 0;
        for (uint32_t k = 0; k < nss; ++k) {
            const uint32_t e = u->substream_end[k];
            if (a < e && e <= size - p && (b[p + a] >> 6) == 3)
                u->substream_flags[k] |= 4;
            a = e;
        }
    }
    u->flags = (uint8_t)flags;
    u->status = (uint8_t)status;
}

// the bytes of substream k of a unit: false when the infos do not fit (an
// I/O error in the reference); *len excludes the two check bytes
MLP_HD inline bool mlp_substream_range(const atg_mlp_unit *u, uint32_t k, uint32_t *start,
                                       uint32_t *len)
{
    const uint32_t a = k ? u->substream_end[0] : 0, e = u->substream_end[k];
    const uint32_t check = (u->substream_flags[0] & 2) ? 2 : 0;
    if (e < a + check || (uint32_t)u->data_start + e > u->size)
        return false;
    *start = u->data_start + a;
    *len = e - a - check;
    return true;
}

// parity and CRC-8 of a substream (its two check bytes follow its len bytes)
MLP_HD inline uint32_t mlp_check_data(const uint8_t *d, uint32_t len, const uint8_t *crc_table)
{
    uint32_t parity = 0, crc = 0x3C, final = 0;
    for (uint32_t i = 0; i < len; ++i) {
        parity ^= d[i];
        final = crc ^ d[i];
        crc = crc_table[final];
    }
    if ((d[len] ^ parity) != 0xA9)
        return ATG_MLP_PARITY_MISMATCH;
    return final == d[len + 1] ? ATG_MLP_OK : ATG_MLP_CRC8_MISMATCH;
}

// ---- the parser.  R(v, k): read k bits into v or leave with an I/O error
#define MLP_R(v, k)                                                                      \
    do {                                                                                 \
        (v) = b.read(k);                                                                 \
        if (b.eof)                                                                       \
            return ATG_MLP_IO_ERROR;                                                     \
    } while (0)
#define MLP_RS(v, k)                                                                     \
    do {                                                                                 \
        (v) = b.read_signed(k);                                                          \
        if (b.eof)                                                                       \
            return ATG_MLP_IO_ERROR;                                                     \
    } while (0)

MLP_HD inline int mlp_read_filter(MlpBits &b, MlpChan &ch, bool iir)
{
    uint32_t order, shift = 0, bits, cshift, flag;
    int32_t coeff[8] = {0, 0, 0, 0, 0, 0, 0, 0}, state[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    MLP_R(order, 4);
    if (order > 8)
        return ATG_MLP_INVALID_CHANNEL_PARAMETERS;
    if (order) {
        MLP_R(shift, 4);
        MLP_R(bits, 5);
        if (bits < 1 || bits > 16)
            return ATG_MLP_INVALID_CHANNEL_PARAMETERS;
        MLP_R(cshift, 3);
        if (bits + cshift > 16)
            return ATG_MLP_INVALID_CHANNEL_PARAMETERS;
        for (uint32_t i = 0; i < order; ++i) {
            int32_t v;
            MLP_RS(v, bits);
            coeff[i] = (int32_t)((uint32_t)v << cshift);
        }
        MLP_R(flag, 1);
        if (flag) {
            if (!iir)
                return ATG_MLP_INVALID_CHANNEL_PARAMETERS;
            uint32_t sbits, sshift;
            MLP_R(sbits, 4);
            MLP_R(sshift, 4);
            for (uint32_t i = 0; i < order; ++i) {
                int32_t v;
                MLP_RS(v, sbits);
                state[i] = (int32_t)((uint32_t)v << sshift);
            }
        }
    }
    for (int i = 0; i < 8; ++i) {
        if (iir) {
            ch.iir[i] = coeff[i];
            ch.iir_state[i] = state[i];
        } else {
            ch.fir[i] = coeff[i];
        }
    }
    if (iir) {
        ch.iir_n = (uint8_t)order;
        ch.iir_shift = (uint8_t)shift;
        ch.iir_set = 1;
    } else {
        ch.fir_n = (uint8_t)order;
        ch.fir_shift = (uint8_t)shift;
    }
    return ATG_MLP_OK;
}

MLP_HD inline void mlp_default_fir(MlpChan &ch)
{
    ch.fir_n = ch.fir_shift = 0;
    for (int i = 0; i < 8; ++i)
        ch.fir[i] = 0;
}
MLP_HD inline void mlp_default_iir(MlpChan &ch)
{
    ch.iir_n = ch.iir_shift = 0;
    ch.iir_set = 1;
    for (int i = 0; i < 8; ++i)
        ch.iir[i] = ch.iir_state[i] = 0;
}

MLP_HD inline int mlp_read_restart(MlpBits &b, MlpState &st, const MlpWho &who)
{
    uint32_t sync, noise_type, skip, lo, hi, mmc, noise_shift, seed;
    MLP_R(sync, 13);
    MLP_R(noise_type, 1);
    MLP_R(skip, 16);
    MLP_R(lo, 4);
    MLP_R(hi, 4);
    MLP_R(mmc, 4);
    MLP_R(noise_shift, 4);
    MLP_R(seed, 23);
    MLP_R(skip, 19);
    MLP_R(skip, 1);
    MLP_R(skip, 8);
    MLP_R(skip, 16);
    st.noise_shift = (uint8_t)noise_shift;
    st.seed = seed;
    if (sync != 0x18F5 || noise_type || hi < lo || mmc < hi)
        return ATG_MLP_INVALID_RESTART_HEADER;
    if (mmc >= kMlpChannels)
        return ATG_MLP_UNSUPPORTED;
    for (uint32_t c = 0; c <= mmc; ++c) {
        MLP_R(skip, 6);
        if (skip > mmc)
            return ATG_MLP_INVALID_RESTART_HEADER;
    }
    MLP_R(skip, 8);
    st.lo = (uint8_t)lo;
    st.hi = (uint8_t)hi;
    st.mmc = (uint8_t)mmc;
    const bool last = who.index == who.substreams - 1;
    if ((who.index == 0 && lo != 0) || (last && (hi != mmc || mmc + 1 < who.channels)))
        return ATG_MLP_UNSUPPORTED;
    if (who.range0 != (lo | hi << 8 | mmc << 16))
        return ATG_MLP_UNSUPPORTED;
    return ATG_MLP_OK;
}

MLP_HD inline int mlp_read_parameters(MlpBits &b, MlpState &st, bool header)
{
    uint32_t bit, v;
    if (header) {
        MLP_R(bit, 1);
        if (bit)
            MLP_R(st.flags, 8);
        else
            st.flags = 0xFF;
    } else if (st.flags & 0x80) {
        MLP_R(bit, 1);
        if (bit)
            MLP_R(st.flags, 8);
    }
    // flags[i] of the reference is bit 7 - i here
    const uint32_t f = st.flags;
    bit = 0;
    if (f & 0x01)
        MLP_R(bit, 1);
    if (bit) {
        MLP_R(st.block_size, 9);
        if (st.block_size < 8)
            return ATG_MLP_INVALID_DECODING_PARAMETERS;
    } else if (header) {
        st.block_size = 8;
    }
    bit = 0;
    if (f & 0x02)
        MLP_R(bit, 1);
    if (bit) {
        uint32_t n;
        MLP_R(n, 4);
        if (n > kMlpMatrices)
            return ATG_MLP_UNSUPPORTED;
        st.n_matrices = n;
        for (uint32_t m = 0; m < n; ++m) {
            uint32_t out, frac, bypass;
            MLP_R(out, 4);
            if (out > st.mmc)
                return ATG_MLP_INVALID_MATRIX_PARAMETERS;
            MLP_R(frac, 4);
            if (frac > 14)
                return ATG_MLP_INVALID_MATRIX_PARAMETERS;
            MLP_R(bypass, 1);
            st.m[m].out = (uint8_t)out;
            st.m[m].bypass = (uint8_t)bypass;
            for (uint32_t c = 0; c < 8; ++c) {
                int32_t x = 0;
                if (c < st.mmc + 3u) {
                    MLP_R(v, 1);
                    if (v) {
                        MLP_RS(x, frac + 2);
                        x = (int32_t)((uint32_t)x << (14 - frac));
                    }
                }
                st.m[m].coeff[c] = x;
            }
        }
    } else if (header) {
        st.n_matrices = 0;
    }
    bit = 0;
    if (f & 0x04)
        MLP_R(bit, 1);
    if (bit) {
        for (uint32_t c = 0; c <= st.mmc; ++c) {
            int32_t x;
            MLP_RS(x, 4);
            if (x < 0)
                return ATG_MLP_UNSUPPORTED;
            st.out_shift[c] = (uint8_t)x;
        }
    } else if (header) {
        for (int c = 0; c < 8; ++c)
            st.out_shift[c] = 0;
    }
    bit = 0;
    if (f & 0x08)
        MLP_R(bit, 1);
    if (bit) {
        for (uint32_t c = 0; c <= st.hi; ++c) {
            MLP_R(v, 4);
            st.quant[c] = (uint8_t)v;
        }
    } else if (header) {
        for (int c = 0; c < 8; ++c)
            st.quant[c] = 0;
    }
    for (uint32_t c = st.lo; c <= st.hi; ++c) {
        MlpChan &ch = st.ch[c];
        MLP_R(bit, 1);
        if (bit) {
            int r;
            bit = 0;
            if (f & 0x10)
                MLP_R(bit, 1);
            if (bit) {
                if ((r = mlp_read_filter(b, ch, false)) != ATG_MLP_OK)
                    return r;
            } else if (header) {
                mlp_default_fir(ch);
            }
            bit = 0;
            if (f & 0x20)
                MLP_R(bit, 1);
            if (bit) {
                if ((r = mlp_read_filter(b, ch, true)) != ATG_MLP_OK)
                    return r;
            } else if (header) {
                mlp_default_iir(ch);
            }
            bit = 0;
            if (f & 0x40)
                MLP_R(bit, 1);
            if (bit)
                MLP_RS(ch.offset, 15);
            else if (header)
                ch.offset = 0;
            MLP_R(v, 2);
            ch.codebook = (uint8_t)v;
            MLP_R(v, 5);
            ch.lsbs = (uint8_t)v;
            if (v > 24)
                return ATG_MLP_INVALID_CHANNEL_PARAMETERS;
        } else if (header) {
            mlp_default_fir(ch);
            mlp_default_iir(ch);
            ch.offset = 0;
            ch.codebook = 0;
            ch.lsbs = 24;
        }
    }
    return ATG_MLP_OK;
}

// One block.  The sink takes block(state, frames), bypass(frame, bits) and
// residual(channel, frame, value); frame counts from the unit's start.
template <class Sink>
MLP_HD inline int mlp_read_block(MlpBits &b, MlpState &st, const MlpWho &who, uint32_t frame0,
                                 Sink &sink, uint32_t *frames)
{
    uint32_t bit;
    MLP_R(bit, 1);
    if (bit) {
        uint32_t header;
        int r;
        MLP_R(header, 1);
        if (header) {
            if ((r = mlp_read_restart(b, st, who)) != ATG_MLP_OK)
                return r;
            st.started = 1;
        } else if (!st.started) {
            return ATG_MLP_UNSUPPORTED;
        }
        if ((r = mlp_read_parameters(b, st, header != 0)) != ATG_MLP_OK)
            return r;
    } else if (!st.started) {
        return ATG_MLP_UNSUPPORTED;
    }
    const uint32_t n = st.block_size;
    if (frame0 + n > ATG_MLP_MAX_UNIT_FRAMES)
        return ATG_MLP_UNSUPPORTED;
    uint32_t lsb_bits[kMlpChannels];
    int32_t offs[kMlpChannels];
    for (uint32_t c = st.lo; c <= st.hi; ++c) {
        const MlpChan &ch = st.ch[c];
        const uint32_t lb = (uint32_t)ch.lsbs - st.quant[c];
        const uint32_t sign = ch.codebook ? lb + 2 - ch.codebook : lb - 1;
        uint32_t off = (uint32_t)ch.offset - (ch.codebook ? 7u << (lb & 31) : 0u);
        if (sign < 0x80000000u)
            off -= 1u << (sign & 31);
        lsb_bits[c] = lb;
        offs[c] = (int32_t)off;
    }
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t bits = 0;
        for (uint32_t m = 0; m < st.n_matrices; ++m)
            if (st.m[m].bypass) {
                MLP_R(bit, 1);
                bits |= bit << m;
            }
        sink.bypass(frame0 + i, bits);
        for (uint32_t c = st.lo; c <= st.hi; ++c) {
            const uint32_t k = st.ch[c].codebook;
            uint32_t msb = 0, lsb;
            if (k) {
                uint32_t len;
                const int v = mlp_codeword(k, b.peek24() >> 15, &len);
                if (b.eof || len > b.n_bits - b.pos)
                    return ATG_MLP_IO_ERROR;
                b.pos += len;
                if (v < 0)
                    return ATG_MLP_INVALID_BLOCK_DATA;
                msb = (uint32_t)v;
            }
            MLP_R(lsb, lsb_bits[c]);
            sink.residual(c, frame0 + i,
                          (int32_t)(((msb << lsb_bits[c]) + lsb + (uint32_t)offs[c])
                                    << st.quant[c]));
        }
    }
    for (uint32_t c = st.lo; c <= st.hi; ++c) {
        const MlpChan &ch = st.ch[c];
        if (ch.fir_n + ch.iir_n > 8)
            return ATG_MLP_INVALID_FILTER_PARAMETERS;
        if (ch.fir_shift && ch.iir_shift && ch.fir_shift != ch.iir_shift)
            return ATG_MLP_INVALID_FILTER_PARAMETERS;
    }
    sink.block(st, n);
    for (uint32_t c = st.lo; c <= st.hi; ++c)
        st.ch[c].iir_set = 0;
    *frames = n;
    return ATG_MLP_OK;
}

// A substream of one access unit: blocks until the last-block bit.
template <class Sink>
MLP_HD inline int mlp_read_substream(const uint8_t *data, uint32_t n_bytes, MlpState &st,
                                     const MlpWho &who, Sink &sink, uint32_t *frames,
                                     uint32_t *blocks)
{
    MlpBits b(data, n_bytes);
    uint32_t total = 0, nb = 0, least = 0xFFFFFFFFu, last;
    do {
        uint32_t n = 0;
        const int r = mlp_read_block(b, st, who, total, sink, &n);
        if (r != ATG_MLP_OK)
            return r;
        total += n;
        ++nb;
        least = st.n_matrices < least ? st.n_matrices : least;
        MLP_R(last, 1);
    } while (!last);
    if (st.n_matrices > least)
        return ATG_MLP_UNSUPPORTED;
    *frames = total;
    *blocks = nb;
    return ATG_MLP_OK;
}

// the filter's shift for a channel's parameters (filter_mlp_channel)
MLP_HD inline uint32_t mlp_filter_shift(const MlpChan &ch)
{
    if (ch.fir_shift && ch.iir_shift)
        return ch.fir_shift;
    return ch.fir_n ? ch.fir_shift : ch.iir_shift;
}

struct MlpSizeSink {
    MLP_HD void bypass(uint32_t, uint32_t) {}
    MLP_HD void residual(uint32_t, uint32_t, int32_t) {}
    MLP_HD void block(const MlpState &, uint32_t) {}
};

// the storing parse's sink: residual planes of `stride` frames each, the
// unit's first frame at frame0; block records from blk
struct MlpStoreSink {
    int32_t *res;
    uint8_t *byp; // NULL for a substream that does not rematrix
    uint64_t stride, frame0;
    MlpBlockRec *blk;
    MLP_HD void bypass(uint32_t f, uint32_t bits)
    {
        if (byp)
            byp[frame0 + f] = (uint8_t)bits;
    }
    MLP_HD void residual(uint32_t c, uint32_t f, int32_t v) { res[c * stride + frame0 + f] = v; }
    MLP_HD void block(const MlpState &st, uint32_t n)
    {
        MlpBlockRec &r = *blk++;
        r.frames = n;
        r.pad = 0;
        for (uint32_t c = st.lo; c <= st.hi; ++c) {
            const MlpChan &ch = st.ch[c];
            MlpChanRec &o = r.ch[c - st.lo];
            for (int i = 0; i < 8; ++i) {
                o.fir[i] = ch.fir[i];
                o.iir[i] = ch.iir[i];
                o.iir_state[i] = ch.iir_state[i];
            }
            o.fir_n = ch.fir_n;
            o.iir_n = ch.iir_n;
            o.shift = (uint8_t)mlp_filter_shift(ch);
            o.quant = st.quant[c];
            o.iir_set = ch.iir_set;
        }
    }
};

MLP_HD inline void mlp_unit_record(const MlpState &st, uint32_t seed, uint32_t frames,
                                   MlpUnitRec *r)
{
    r->seed = seed;
    r->frames = frames;
    r->n_matrices = (uint8_t)st.n_matrices;
    r->noise_shift = st.noise_shift;
    r->mmc = st.mmc;
    uint32_t noise = 0;
    for (uint32_t m = 0; m < kMlpMatrices; ++m) {
        r->m[m] = st.m[m];
        if (m < st.n_matrices)
            noise |= (uint32_t)(st.m[m].coeff[st.mmc + 1] | st.m[m].coeff[st.mmc + 2]);
    }
    r->noise = noise ? 1 : 0;
    for (int c = 0; c < 8; ++c) {
        r->out_shift[c] = st.out_shift[c];
        r->quant[c] = st.quant[c];
    }
}

// one step of filter_mlp_channel: h[0] is the newest state
MLP_HD inline int32_t mlp_filter_step(const MlpChanRec &p, int32_t *fir_h, int32_t *iir_h,
                                      int32_t residual)
{
    int64_t sum = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        sum += (int64_t)p.fir[j] * fir_h[j] + (int64_t)p.iir[j] * iir_h[j];
    const int32_t shifted = (int32_t)(sum >> p.shift);
    const int32_t v = mlp_mask((int32_t)((uint32_t)shifted + (uint32_t)residual), p.quant);
#pragma unroll
    for (int j = 7; j > 0; --j) {
        fir_h[j] = fir_h[j - 1];
        iir_h[j] = iir_h[j - 1];
    }
    fir_h[0] = v;
    iir_h[0] = (int32_t)((uint32_t)v - (uint32_t)shifted);
    return v;
}

// rematrix_mlp_channels and the output shift for one frame: ch[0..mmc] are
// the filtered channels, i the frame's index in its unit
MLP_HD inline void mlp_rematrix_frame(const MlpUnitRec &u, uint32_t i, uint32_t bypass,
                                      int32_t *ch)
{
    int32_t n0 = 0, n1 = 0;
    if (u.noise) {
        uint32_t seed = u.seed;
        for (uint32_t k = 0; k < i; ++k)
            seed = mlp_next_seed(seed);
        n0 = (int32_t)((uint32_t)(int32_t)(int8_t)(seed >> 15) << u.noise_shift);
        n1 = (int32_t)((uint32_t)(int32_t)(int8_t)(seed >> 7) << u.noise_shift);
    }
    for (uint32_t m = 0; m < u.n_matrices; ++m) {
        const MlpMatrix &x = u.m[m];
        int64_t sum = 0;
        for (uint32_t c = 0; c < kMlpChannels; ++c)
            if (c <= u.mmc)
                sum += (int64_t)ch[c] * x.coeff[c];
        sum += (int64_t)n0 * x.coeff[u.mmc + 1] + (int64_t)n1 * x.coeff[u.mmc + 2];
        const int32_t v = (int32_t)((uint32_t)mlp_mask((int32_t)(sum >> 14), u.quant[x.out]) +
                                    ((bypass >> m) & 1u));
        for (uint32_t c = 0; c < kMlpChannels; ++c)
            if (c == x.out)
                ch[c] = v;
    }
    for (uint32_t c = 0; c < kMlpChannels; ++c)
        if (c <= u.mmc)
            ch[c] = (int32_t)((uint32_t)ch[c] << u.out_shift[c]);
}
