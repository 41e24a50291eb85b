// wavpack_common.h — WavPack arithmetic shared by the host reader and the
// decoder kernels (wavpack_decode.hip).  Reference: src/decoders/wavpack.c
// (apply_weight :1373-1378, update_weight :1380-1390,
// pop_decorrelation_weight :849-860, read_wv_exp2 :1082-1133).
//
// Everything that C leaves undefined in the reference is defined here: sums
// wrap at 32 bits in uint32_t, shift counts are masked to five bits.
#pragma once
#include <cstdint>
#include <initializer_list>

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

// ---- the forward arithmetic of the encoder (src/encoders/wavpack.c:
// store_weight :917-929, wv_log2 :1323-1376, reset_block_parameters :363-453,
// init_context :262-290)

WV_HD int32_t store_weight(int32_t w)
{
    w = clamp_weight(w);
    if (w > 0)
        return (w - ((w + 64) >> 7) + 4) >> 3;
    return w ? (w + 4) >> 3 : 0;
}

WV_HD uint32_t bit_length(uint32_t v)
{
#ifdef __HIP_DEVICE_COMPILE__
    return v ? 32u - (uint32_t)__clz(v) : 0u;
#else
    uint32_t n = 0;
    while (v) {
        ++n;
        v >>= 1;
    }
    return n;
#endif
}

// the 16-bit log form of a sample; table[i] = floor(256 * log2(1 + i/256) + 0.5).
// |INT32_MIN| is taken in uint32_t (abs() of it is undefined in the reference)
WV_HD int32_t log2_value(const uint8_t *table, int32_t value)
{
    const uint32_t m = value < 0 ? 0u - (uint32_t)value : (uint32_t)value;
    const uint32_t a = m + (m >> 9);
    const uint32_t c = bit_length(a);
    const uint32_t idx = a < 256u ? (a << (9u - c)) & 0xFFu : (a >> (c - 9u)) & 0xFFu;
    const int32_t r = (int32_t)((c << 8) + table[idx]);
    return value < 0 ? -r : r;
}

WV_HD int32_t roundtrip_value(const uint8_t *log_table, const uint16_t *exp_table, int32_t v)
{
    return exp2_value(exp_table, log2_value(log_table, v));
}

constexpr int32_t kDelta = 2; // every pass of the reference encoder

// the term table of a stream block: `eff` coded channels, `passes` the
// encoder option (0, 1, 2, 5, 10, 16).  A one-channel block has the five-term
// table for 5, 10 and 16 alike.  -> number of terms
WV_HD int32_t term_table(uint32_t eff, uint32_t passes, int8_t term[kMaxTerms])
{
    if (passes == 0)
        return 0;
    if (passes == 1) {
        term[0] = 18;
        return 1;
    }
    if (passes == 2) {
        term[0] = 17;
        term[1] = 18;
        return 2;
    }
    if (passes == 5 || eff == 1) {
        term[0] = 3, term[1] = 17, term[2] = 2, term[3] = 18, term[4] = 18;
        return 5;
    }
    if (passes == 10) {
        term[0] = 4, term[1] = 17, term[2] = -1, term[3] = 5, term[4] = 3;
        term[5] = 2, term[6] = -2, term[7] = 18, term[8] = 18, term[9] = 18;
        return 10;
    }
    term[0] = 2, term[1] = 18, term[2] = -1, term[3] = 8, term[4] = 6, term[5] = 3;
    term[6] = 5, term[7] = 7, term[8] = 4, term[9] = 2, term[10] = 18, term[11] = -2;
    term[12] = 3, term[13] = 2, term[14] = 18, term[15] = 18;
    return 16;
}

// history samples a term keeps per channel
WV_HD uint32_t term_samples(int32_t term) { return term > 8 ? 2u : (term > 0 ? (uint32_t)term : 1u); }

// the deepest history of a stream's own table (terms 17 and 18 keep two
// samples): the reference aborts on a non-final block shorter than its
// deepest term 1..8, and block sizes below this depth are refused
inline uint32_t term_depth(uint32_t stream_channels, uint32_t passes)
{
    int8_t term[kMaxTerms];
    const int32_t n = term_table(stream_channels, passes, term);
    uint32_t d = 0;
    for (int32_t k = 0; k < n; ++k)
        if (term[k] > 0 && term_samples(term[k]) > d)
            d = term_samples(term[k]);
    return d;
}

// the channel groups of a track -> number of streams (split[] holds 1 or 2);
// more than two channels without a known mask are coded one by one
inline uint32_t stream_split(uint32_t channels, uint32_t mask, uint8_t *split, uint32_t cap)
{
    auto set = [&](std::initializer_list<int> v) {
        uint32_t k = 0;
        for (int c : v)
            if (k < cap)
                split[k++] = (uint8_t)c;
        return (uint32_t)v.size();
    };
    if (channels <= 2)
        return set({(int)channels});
    switch (mask) {
    case 0x7: return set({2, 1});
    case 0x33: return set({2, 2});
    case 0x107: return set({2, 1, 1});
    case 0x37: return set({2, 1, 2});
    case 0x3F: return set({2, 1, 1, 2});
    default: break;
    }
    for (uint32_t k = 0; k < channels && k < cap; ++k)
        split[k] = 1;
    return channels;
}

} // namespace wv
