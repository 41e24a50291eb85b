// pcm_files.h — header parsers of the two big-endian PCM containers, AIFF
// and Sun AU, over a whole file image.  Plain host code with no HIP in it:
// pcm_bytes.hip exports them as atg_aiff_read_info / atg_au_read_info, and
// tools/pcm_bytes_check.cpp builds them alone under the host sanitizers.
//
// atg_aiff_parse walks the chunks as the reference's AiffReader.__init__
// does (audiotools/aiff.py:353-432), but for one thing: an SSND chunk that
// comes before COMM is not refused there and then; the walk goes on to COMM
// and the sound data found first is reported, and "SSND chunk found before
// fmt" is left for a file that has no COMM after it.  The reference's quirks
// are kept: a COMM chunk is read as its 18 bytes whatever size it declares,
// other chunks are skipped by their declared size with no check that the
// file holds them, a pad byte that is missing is an error, and the SSND
// offset / block-size words are skipped, not applied.  atg_au_parse reads the
// 24-byte header (audiotools/au.py:35-59).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/atgpu.h"

static inline uint32_t pf_be32(const uint8_t *p)
{
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

static inline int pf_printable(const uint8_t *id)
{
    for (int i = 0; i < 4; ++i)
        if (id[i] < 0x20 || id[i] > 0x7E)
            return 0;
    return 1;
}

// The 80-bit extended value as int(mantissa * 2.0 ** (exponent - 16446)),
// the reference's parse_ieee_extended followed by int(): the mantissa is
// first rounded to 53 bits, half to even, as its conversion to a double
// does.  Returns 0 and sets *fits = 0 when the result is not in [0, 2^32).
static inline uint32_t pf_extended_to_u32(const uint8_t *p, int *fits)
{
    const uint32_t sign = p[0] >> 7;
    const uint32_t exponent = (((uint32_t)p[0] & 0x7Fu) << 8) | p[1];
    uint64_t mant = ((uint64_t)pf_be32(p + 2) << 32) | pf_be32(p + 6);
    *fits = 1;
    if (exponent == 0x7FFF) { // the reference's 1.79769313486231e+308
        *fits = 0;
        return 0;
    }
    if (mant == 0)
        return 0;
    int e = (int)exponent - 16383 - 63;
    int msb = 63;
    while (!(mant >> msb))
        --msb;
    if (msb > 52) {
        const int s = msb - 52;
        const uint64_t rem = mant & (((uint64_t)1 << s) - 1), half = (uint64_t)1 << (s - 1);
        mant >>= s;
        if (rem > half || (rem == half && (mant & 1)))
            ++mant;
        e += s;
    }
    // value = mant * 2^e, mant < 2^54
    uint64_t v;
    if (e >= 0) {
        if (e > 32 || (mant << e) >> e != mant || (mant << e) >> 32) {
            *fits = 0;
            return 0;
        }
        v = mant << e;
    } else {
        v = -e >= 64 ? 0 : mant >> -e;
        if (v >> 32) {
            *fits = 0;
            return 0;
        }
    }
    if (sign && v) {
        *fits = 0;
        return 0;
    }
    return (uint32_t)v;
}

static inline int atg_aiff_parse(const uint8_t *data, uint64_t len, atg_aiff_info *info)
{
    if (!info)
        return ATG_ERR_INVALID;
    memset(info, 0, sizeof *info);
    if (!data && len)
        return ATG_ERR_INVALID;
    if (len < 12)
        return ATG_AIFF_INVALID_AIFF;
    if (memcmp(data, "FORM", 4))
        return ATG_AIFF_NOT_AIFF;
    if (memcmp(data + 8, "AIFF", 4))
        return ATG_AIFF_INVALID_AIFF;
    int64_t total = (int64_t)pf_be32(data + 4) - 4;
    uint64_t pos = 12; // never above len
    int comm_read = 0, unsupported = 0, early_ssnd = 0;
    uint64_t early_offset = 0, early_bytes = 0;
    while (total > 0) {
        if (len - pos < 8)
            return ATG_AIFF_INVALID_AIFF;
        const uint8_t *id = data + pos;
        const uint64_t size = pf_be32(data + pos + 4);
        pos += 8;
        if (!pf_printable(id))
            return ATG_AIFF_INVALID_CHUNK_ID;
        total -= 8;
        if (!memcmp(id, "COMM", 4)) {
            if (len - pos < 18)
                return ATG_AIFF_IOERROR;
            const uint8_t *c = data + pos;
            int fits;
            info->channels = ((uint32_t)c[0] << 8) | c[1];
            info->total_pcm_frames = pf_be32(c + 2);
            info->bits_per_sample = ((uint32_t)c[6] << 8) | c[7];
            info->sample_rate = pf_extended_to_u32(c + 8, &fits);
            info->channel_mask = info->channels == 1 ? 0x4u : info->channels == 2 ? 0x3u : 0u;
            unsupported = !fits || (info->bits_per_sample != 8 && info->bits_per_sample != 16 &&
                                    info->bits_per_sample != 24);
            comm_read = 1;
            pos += 18;
            if (early_ssnd) { // the sound data came first: back to it
                info->ssnd_data_offset = early_offset;
                info->ssnd_data_bytes = early_bytes;
                return unsupported ? (int)ATG_ERR_UNSUPPORTED : (int)ATG_AIFF_OK;
            }
        } else if (!memcmp(id, "SSND", 4)) {
            pos += len - pos < 8 ? len - pos : 8;
            const uint64_t declared = size > 8 ? size - 8 : 0;
            const uint64_t present = declared < len - pos ? declared : len - pos;
            if (comm_read) {
                info->ssnd_data_offset = pos;
                info->ssnd_data_bytes = present;
                return unsupported ? (int)ATG_ERR_UNSUPPORTED : (int)ATG_AIFF_OK;
            }
            if (!early_ssnd) {
                early_ssnd = 1;
                early_offset = pos;
                early_bytes = present;
            }
            pos += present;
        } else {
            pos += len - pos < size ? len - pos : size;
        }
        if (size % 2) {
            if (pos >= len)
                return ATG_AIFF_INVALID_CHUNK;
            pos += 1;
            total -= (int64_t)size + 1;
        } else {
            total -= (int64_t)size;
        }
    }
    return early_ssnd ? ATG_AIFF_PREMATURE_SSND : ATG_AIFF_NO_SSND;
}

static inline int atg_au_parse(const uint8_t *data, uint64_t len, atg_au_info *info)
{
    if (!info)
        return ATG_ERR_INVALID;
    memset(info, 0, sizeof *info);
    if (!data && len)
        return ATG_ERR_INVALID;
    if (len < 24)
        return ATG_AU_IOERROR;
    if (memcmp(data, ".snd", 4))
        return ATG_AU_INVALID_HEADER;
    const uint32_t encoding = pf_be32(data + 12);
    if (encoding < 2 || encoding > 4)
        return ATG_AU_UNSUPPORTED_FORMAT;
    info->data_offset = pf_be32(data + 4);
    info->data_size = pf_be32(data + 8);
    info->bits_per_sample = (encoding - 1) * 8;
    info->sample_rate = pf_be32(data + 16);
    info->channels = pf_be32(data + 20);
    info->channel_mask = info->channels == 1 ? 0x4u : info->channels == 2 ? 0x3u : 0u;
    const uint64_t per_frame = (uint64_t)(info->bits_per_sample / 8) * info->channels;
    if (!per_frame)
        return ATG_ERR_UNSUPPORTED; // no channels: the reference divides by zero
    info->total_pcm_frames = info->data_size / per_frame;
    const uint64_t after = info->data_offset < len ? len - info->data_offset : 0;
    info->data_bytes = info->data_size < after ? info->data_size : after;
    return ATG_AU_OK;
}
