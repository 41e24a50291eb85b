// aob_common.h — what the DVD-Audio kernels and their host code share: the
// sector walk of an AOB file (MPEG program-stream pack header, PES packets,
// the private-stream-1 audio header), the attribute code tables, and the
// byte order of the packed-PCM codec.  The walk is plain C++ over a byte
// pointer, so the host runs the same function the lanes run.
#pragma once
#include <stdint.h>

#include "../../include/atgpu_dvda.h"

#ifdef __HIPCC__
#define AOB_HD __host__ __device__
#else
#define AOB_HD
#endif

constexpr uint32_t kAobSector = 2048;
constexpr uint32_t kAobBlock = 256;
// PCM pass: chunks (two frames each) per tile, and the bytes of the largest
// chunk (24 bit, 6 channels)
constexpr uint32_t kAobTileChunks = 512;
constexpr uint32_t kAobMaxChunk = 36;
constexpr uint32_t kAobStageBytes = kAobTileChunks * kAobMaxChunk;
// aligned 16-byte units per sector
constexpr uint32_t kAobUnits = kAobSector / 16;

// The 24-bit chunk layouts, one row per channel count: byte i of a chunk in
// the file is byte kAobOrder24[ch - 1][i] of the chunk's 2 * ch little-endian
// samples (frame 0's channels, then frame 1's).  The format stores the two
// high bytes of every sample first and gathers the low bytes behind them.
// The 16-bit layouts are big-endian samples in order and need no table.
constexpr uint8_t kAobOrder24[6][kAobMaxChunk] = {
    {2, 1, 5, 4, 0, 3},
    {2, 1, 5, 4, 8, 7, 11, 10, 0, 3, 6, 9},
    {8, 7, 17, 16, 6, 15, 2, 1, 5, 4, 11, 10, 14, 13, 0, 3, 9, 12},
    {8, 7, 11, 10, 20, 19, 23, 22, 6, 9, 18, 21, 2, 1, 5, 4, 14, 13, 17, 16, 0, 3, 12, 15},
    {8,  7, 11, 10, 14, 13, 23, 22, 26, 25, 29, 28, 6, 9,  12,
     21, 24, 27, 2,  1,  5,  4,  17, 16, 20, 19, 0,  3, 15, 18},
    {8,  7,  11, 10, 26, 25, 29, 28, 6,  9,  24, 27, 2,  1,  5, 4,  14, 13,
     17, 16, 20, 19, 23, 22, 32, 31, 35, 34, 0,  3,  12, 15, 18, 21, 30, 33},
};

// the inverse: byte p of the samples is byte inv[ch - 1][p] of the file's chunk
struct AobInverse24 {
    uint8_t at[6][kAobMaxChunk];
};
constexpr AobInverse24 aob_inverse24()
{
    AobInverse24 t = {};
    for (int c = 0; c < 6; ++c)
        for (int i = 0; i < 6 * (c + 1); ++i)
            t.at[c][kAobOrder24[c][i]] = (uint8_t)i;
    return t;
}

AOB_HD inline uint32_t aob_bits(uint32_t code) { return code == 0 ? 16 : code == 1 ? 20 : code == 2 ? 24 : 0; }

AOB_HD inline uint32_t aob_rate(uint32_t code)
{
    const uint32_t base = (code & 8) ? 44100 : 48000;
    return (code & 7) < 3 ? base << (code & 7) : 0;
}

// channel count and speaker mask per channel assignment 0..20; the counts
// are packed four bits each so the device needs no memory for them
AOB_HD inline uint32_t aob_channels(uint32_t ca)
{
    // 1 2 3 4 3 4 5 3 4 5 4 5 6 4 5 4 | 5 6 5 5 6, assignment 0 in the low bits
    const uint64_t lo = 0x4546545435434321ull; // assignments 0..15
    const uint32_t hi = 0x65565u;              // assignments 16..20
    if (ca > 20)
        return 0;
    return ca < 16 ? (uint32_t)(lo >> (4 * ca)) & 15u : (hi >> (4 * (ca - 16))) & 15u;
}

AOB_HD inline uint32_t aob_channel_mask(uint32_t ca)
{
    switch (ca) {
    case 0: return 0x4;
    case 1: return 0x3;
    case 2: return 0x103;
    case 3: return 0x33;
    case 4: return 0xB;
    case 5: return 0x10B;
    case 6: case 18: return 0x3B;
    case 7: return 0x7;
    case 8: case 13: return 0x107;
    case 9: case 14: case 19: return 0x37;
    case 10: case 15: return 0xF;
    case 11: case 16: return 0x10F;
    case 12: case 17: case 20: return 0x3F;
    default: return 0;
    }
}

// Walk one sector.  Every read is checked against the sector's end, so a
// lane never looks past its own 2048 bytes.
AOB_HD inline atg_aob_sector aob_walk_sector(const uint8_t *s)
{
    atg_aob_sector r = {};
    auto bad = [](uint8_t why) {
        atg_aob_sector b = {};
        b.status = why;
        return b;
    };
    if (s[0] != 0 || s[1] != 0 || s[2] != 1 || s[3] != 0xBA)
        return bad(ATG_AOB_SECTOR_SYNC);
    if ((s[4] >> 6) != 1 || !(s[4] & 4) || !(s[6] & 4) || !(s[8] & 4) || !(s[9] & 1) ||
        (s[12] & 3) != 3)
        return bad(ATG_AOB_SECTOR_MARKER);
    uint32_t pos = 14 + (s[13] & 7);
    bool found = false;
    while (pos < kAobSector) {
        if (kAobSector - pos < 6)
            return bad(ATG_AOB_SECTOR_SHORT);
        if (s[pos] != 0 || s[pos + 1] != 0 || s[pos + 2] != 1)
            return bad(ATG_AOB_SECTOR_START_CODE);
        const uint32_t id = s[pos + 3], len = ((uint32_t)s[pos + 4] << 8) | s[pos + 5];
        pos += 6;
        if (id != 0xBD) {
            if (len > kAobSector - pos)
                return bad(ATG_AOB_SECTOR_PACKET_END);
            pos += len;
            continue;
        }
        uint32_t q = pos;
        if (kAobSector - q < 3)
            return bad(ATG_AOB_SECTOR_AUDIO_HEADER);
        const uint32_t pad1 = s[q + 2];
        q += 3;
        if (pad1 > kAobSector - q)
            return bad(ATG_AOB_SECTOR_AUDIO_HEADER);
        q += pad1;
        if (kAobSector - q < 4)
            return bad(ATG_AOB_SECTOR_AUDIO_HEADER);
        const uint32_t codec = s[q], pad2 = s[q + 3];
        q += 4;
        if (codec == 0xA0) {
            if (kAobSector - q < 9 || pad2 < 9)
                return bad(ATG_AOB_SECTOR_AUDIO_HEADER);
            r.group_1_bps = s[q + 3] >> 4;
            r.group_1_rate = s[q + 4] >> 4;
            r.channel_assignment = s[q + 6];
            q += 9;
            if (pad2 - 9 > kAobSector - q)
                return bad(ATG_AOB_SECTOR_AUDIO_HEADER);
            q += pad2 - 9;
        } else {
            if (pad2 > kAobSector - q)
                return bad(ATG_AOB_SECTOR_AUDIO_HEADER);
            q += pad2;
        }
        const uint32_t header = 7 + pad1 + pad2;
        if (len < header)
            return bad(ATG_AOB_SECTOR_NEGATIVE);
        if (len - header > kAobSector - q)
            return bad(ATG_AOB_SECTOR_PACKET_END);
        r.codec_id = (uint8_t)codec;
        r.payload_offset = (uint16_t)q;
        r.payload_length = (uint16_t)(len - header);
        pos = q + (len - header);
        found = true;
    }
    if (!found)
        return bad(ATG_AOB_SECTOR_NO_AUDIO);
    return r;
}

// A title's result from its first sector's record, its first bad sector
// (n_sectors when none) and the payload bytes before it.
AOB_HD inline atg_aob_result aob_title_result(const atg_aob_sector *first, uint32_t n_sectors,
                                              uint32_t first_bad, uint64_t payload_bytes)
{
    atg_aob_result r = {};
    if (n_sectors == 0) {
        r.status = ATG_DVDA_EOF;
        return r;
    }
    if (first_bad == 0) {
        r.status = ATG_DVDA_BAD_SECTOR;
        return r;
    }
    if (first->codec_id != 0xA0) {
        r.status = first->codec_id == 0xA1 ? ATG_DVDA_MLP : ATG_DVDA_UNKNOWN_CODEC;
        return r;
    }
    r.channel_assignment = first->channel_assignment;
    r.bits_per_sample = aob_bits(first->group_1_bps);
    r.sample_rate = aob_rate(first->group_1_rate);
    r.channels = aob_channels(first->channel_assignment);
    r.channel_mask = aob_channel_mask(first->channel_assignment);
    if ((r.bits_per_sample != 16 && r.bits_per_sample != 24) || !r.sample_rate || !r.channels) {
        r.status = ATG_DVDA_UNSUPPORTED;
        return r;
    }
    const uint32_t chunk = r.bits_per_sample / 8 * r.channels * 2;
    r.good_frames = 2 * (payload_bytes / chunk);
    r.stop_sector = first_bad;
    r.status = first_bad < n_sectors ? ATG_DVDA_BAD_SECTOR : ATG_DVDA_OK;
    return r;
}
