// wavpack_common.h — WavPack arithmetic shared by the host reader and the
// decoder kernels (wavpack_decode.hip).  Reference: src/decoders/wavpack.c
// (apply_weight :1373-1378, update_weight :1380-1390,
// pop_decorrelation_weight :849-860, read_wv_exp2 :1082-1133).
//
// Everything that C leaves undefined in the reference is defined here: sums
// wrap at 32 bits in uint32_t, shift counts are masked to five bits.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define WV_HD __host__ __device__ __forceinline__
#else
#define WV_HD inline
#endif

namespace wv {

// header flag bits (the 32-bit word at byte 24 of a block header)
constexpr uint32_t kMono = 1u << 2, kJoint = 1u << 4, kExtended = 1u << 8, kInitial = 1u << 11,
                   kFinal = 1u << 12, kFalseStereo = 1u << 30, kReserved = 1u << 31;

// channels the block codes (1 or 2) and channels it puts out
WV_HD uint32_t coded_channels(uint32_t flags) { return (flags & (kMono | kFalseStereo)) ? 1u : 2u; }
WV_HD uint32_t out_channels(uint32_t flags)
{
    return ((flags & kMono) && !(flags & kFalseStereo)) ? 1u : 2u;
}

// the device's copy of one block of the host table
struct Block {
    uint64_t byte_off; // sub-block data (after the 32-byte header), in the batch buffer
    uint64_t rbase;    // the block's slot: coded channels x n int32, channel-major
    uint64_t pcm_base; // sample index of the set's first frame in the batch output
    uint32_t size;     // bytes of sub-block data
    uint32_t n;        // block_samples
    uint32_t flags, crc;
    uint16_t first_ch, track_ch; // first output channel, channels of the track
    uint32_t scratch;            // decoded for its status only: no PCM
};

constexpr int kMaxTerms = 16;

// what k_wvd_parse hands to k_wvd_decorr, in file order (the passes are
// applied from the last entry to the first)
struct Params {
    int32_t n_terms;         // -1: no terms sub-block
    int8_t term[kMaxTerms];
    uint8_t delta[kMaxTerms];
    int32_t weight[kMaxTerms][2];
    // samples before the block: terms 1..8 oldest first; 17/18 [out[-1],
    // out[-2]]; negative terms one sample
    int32_t hist[kMaxTerms][2][8];
    uint8_t ext[4]; // sent, zero, one, duplicate bits
    uint32_t has_ext;
};

WV_HD int32_t apply_weight(int32_t weight, int64_t sample)
{
    return (int32_t)(uint32_t)(uint64_t)(((int64_t)weight * sample + 512) >> 10);
}

WV_HD int32_t update_weight(int64_t source, int32_t result, int32_t delta)
{
    if (source == 0 || result == 0)
        return 0;
    return ((source ^ (int64_t)result) >= 0) ? delta : -delta;
}

WV_HD int32_t clamp_weight(int32_t w) { return w > 1024 ? 1024 : (w < -1024 ? -1024 : w); }

WV_HD int32_t restore_weight(uint8_t byte)
{
    const int32_t v = (int8_t)byte;
    if (v > 0)
        return (v << 3) + (((v << 3) + 64) >> 7);
    return v * 8;
}

// read_wv_exp2 of a signed 16-bit value; table[i] = floor(256 * 2^(i/256) + 0.5)
WV_HD int32_t exp2_value(const uint16_t *table, int32_t value)
{
    const uint32_t v = (uint32_t)(value < 0 ? -value : value);
    const uint32_t e = table[v & 0xFFu];
    uint32_t r;
    if (v <= 2304u)
        r = e >> (9u - (v >> 8));
    else
        r = e << (((v >> 8) - 9u) & 31u);
    return value < 0 ? (int32_t)(0u - r) : (int32_t)r;
}

} // namespace wv
