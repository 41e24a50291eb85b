// shn_decode.hip — Shorten (.shn) decoder for a batch of streams.
//
// Replaces the reference's audiotools.decoders.SHNDecoder
// (src/decoders/shn.c: read_shn_header :297, read_framelist :357, the DIFF
// and QLPC readers :489-657, pcm_split :193).  A .shn stream has no frame
// table: where command n starts is known only after every code before it has
// been walked.  So the decoder makes two passes.
//
//   k_shnd_index  one wave per stream walks the commands and records every
//                 audio unit (bit offset, command, block length, shift,
//                 channel, first frame) and every VERBATIM command; it ends
//                 with the stream's status and its PCM frame count.  The
//                 residual run of a unit is skipped by the whole wave: 64
//                 words are loaded, every lane builds for its word the map
//                 "a code search enters at bit o -> it leaves into the next
//                 word at bit o', having met k stop bits", the entry offset
//                 is chained through the 64 maps, and a prefix sum of the
//                 counts finds the word in which the run's last code ends.
//                 The lane-serial walker stays for code widths above 31 bits
//                 and short runs, and as the baseline (set_index_walk).
//   (host)        PCM and VERBATIM extents from the frame and byte counts.
//   k_shnd_parse  one lane per recorded entry: the residuals of an audio
//                 unit go to the unit's own output slots, a VERBATIM's bytes
//                 to the stream's header or footer bytes.
//   k_shnd_recon  one wave per (stream, channel), units in block order since
//                 history and means carry over: DIFF1-3 are one to three
//                 wrapping prefix sums per 64 samples seeded by the carried
//                 samples, QLPC is a recurrence and runs on one lane; then
//                 the mean, the history, shift and sign adjust, in place.
//
// Every read is bounded by the image: bits past its end read as an I/O
// error, as in the reference, and the stream's PCM ends before its first
// incomplete set of channels.
#include "handle_lock.h"
#include "host_common.h"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/atgpu.h"
#include "shn_common.h"
#include "table_search.h"
#include "wave.h"

namespace {

struct DTrack {
    uint64_t data_offset, data_bytes, start_bit;
    uint64_t ubase;  // first entry slot of the stream
    uint64_t pcm_at; // first output sample (after the index pass)
    uint64_t verb_at; // first VERBATIM byte (after the index pass)
    uint32_t ucap;   // entry slots
    uint32_t channels, block_length, max_lpc, mean_count;
    int32_t adjust; // 1 << (bps - 1) for the unsigned file types
};

struct DOut {
    uint64_t frames;
    uint32_t status;
    uint32_t committed; // entries up to the last complete set of channels
    uint32_t entries;   // entries met, recorded or not
    uint32_t header_bytes, footer_bytes;
    uint32_t dead_from; // audio entries from here on belong to a set QUIT cut short
};

// One recorded command.  Audio: bit = the energy field, length = the block
// length, frame = its first PCM frame.  VERBATIM: bit = its first byte code,
// length = its size, frame = bytes of the same kind before it.
struct Entry {
    uint32_t bit, length, frame, meta;
};
constexpr uint32_t kCmdMask = 15u;
constexpr uint32_t kShiftAt = 4;    // 5 bits
constexpr uint32_t kChannelAt = 9;  // 9 bits
constexpr uint32_t kFooter = 1u << 31;

constexpr uint32_t kHist = 32; // history kept per channel: min(max(3, max LPC), 32)

// --------------------------------------------------------------- index pass
__device__ __forceinline__ void serial_skip(shn::Bits &r, uint32_t n, uint32_t w)
{
    for (uint32_t i = 0; i < n && !r.bad; ++i)
        r.skip(w);
}

// Skip n codes of a stop bit and w (1..31) low bits with the whole wave.
// map[o * 64 + lane]: low byte the exit offset, high byte the stop bits met.
__device__ void coop_skip(shn::Bits &r, uint32_t n, uint32_t w, uint32_t lane, uint16_t *map)
{
    while (n && !r.bad) {
        const uint64_t base = r.pos >> 5;
        const uint32_t entry = (uint32_t)r.pos & 31u;
        if (base * 4u >= r.nbytes) {
            r.bad = true;
            break;
        }
        const uint32_t word = shn::be_word(r.img, r.nbytes, base + lane);
        for (int o = 31; o >= 0; --o) {
            const uint32_t m = word & (0xFFFFFFFFu >> o);
            uint32_t e = 0;
            if (m) {
                const uint32_t nx = (uint32_t)__clz((int)m) + 1u + w;
                if (nx >= 32u) {
                    e = (nx - 32u) | (1u << 8);
                } else {
                    const uint32_t p = map[nx * 64u + lane];
                    e = (p & 0xFFu) | (((p >> 8) + 1u) << 8);
                }
            }
            map[(uint32_t)o * 64u + lane] = (uint16_t)e;
        }
        __syncthreads();
        uint32_t e = entry, mine = 0;
        for (uint32_t l = 0; l < 64u; ++l) {
            if (l == lane)
                mine = e;
            e = map[e * 64u + l] & 0xFFu;
        }
        const uint32_t cnt = map[mine * 64u + lane] >> 8;
        const uint32_t inc = wave_incl_scan_u32(cnt, (int)lane);
        const uint32_t total = (uint32_t)__shfl((int)inc, 63, 64);
        if (total < n) {
            n -= total;
            r.pos = (base + 64u) * 32u + e;
        } else {
            const uint64_t ball = __ballot(inc >= n);
            const int who = __ffsll((long long)ball) - 1;
            uint32_t p = mine;
            if ((int)lane == who) {
                const uint32_t k = n - (inc - cnt);
                for (uint32_t j = 0; j < k; ++j) {
                    const uint32_t m = word & (0xFFFFFFFFu >> p);
                    p = (uint32_t)__clz((int)m) + 1u + w;
                }
            }
            p = (uint32_t)__shfl((int)p, who, 64);
            r.pos = (base + (uint32_t)who) * 32u + p;
            n = 0;
        }
        __syncthreads();
    }
    if (!r.bad && r.pos > r.nbits)
        r.bad = true;
}

constexpr uint32_t kCoopMin = 32; // shorter runs are not worth a 64-word step

__global__ __launch_bounds__(64) void k_shnd_index(const uint8_t *__restrict__ data,
                                                   const DTrack *__restrict__ tracks,
                                                   Entry *__restrict__ entries,
                                                   DOut *__restrict__ outs, int coop)
{
    __shared__ uint16_t map[32 * 64];
    const DTrack T = tracks[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    const uint32_t C = T.channels, mc = T.mean_count;
    shn::Bits r;
    r.open(data + T.data_offset, T.data_bytes, T.start_bit);
    Entry *mine = entries + T.ubase;
    uint32_t L = T.block_length, shift = 0, c = 0, set_len = 0;
    uint32_t nent = 0, committed = 0, hb = 0, fb = 0, chb = 0, cfb = 0;
    uint32_t set_start = 0, dead_from = 0xFFFFFFFFu;
    uint64_t frames = 0;
    bool seen = false;
    uint32_t status = ATG_SHN_OK;
    if (C < 1 || C > ATG_SHN_MAX_CHANNELS || mc > ATG_SHN_MAX_MEAN_COUNT)
        status = ATG_SHN_UNSUPPORTED;
    auto skip = [&](uint32_t n, uint32_t w) {
        if (coop && w <= 31u && n >= kCoopMin)
            coop_skip(r, n, w, lane, map);
        else
            serial_skip(r, n, w);
    };
    while (status == ATG_SHN_OK) {
        const uint32_t cmd = r.uns(shn::kCommandSize);
        if (r.bad)
            break;
        if (cmd <= shn::FN_DIFF3 || cmd == shn::FN_QLPC || cmd == shn::FN_ZERO) {
            if (L == 0 || ((cmd == shn::FN_DIFF0 || cmd == shn::FN_QLPC) && mc == 0) ||
                (c && L != set_len) || (frames + L) * C > ATG_SHN_MAX_TRACK_SAMPLES) {
                status = ATG_SHN_UNSUPPORTED;
                break;
            }
            set_len = L;
            seen = true;
            if (c == 0)
                set_start = nent;
            if (nent < T.ucap && lane == 0)
                mine[nent] = Entry{(uint32_t)r.pos, L, (uint32_t)frames,
                                   cmd | (shift << kShiftAt) | (c << kChannelAt)};
            ++nent;
            if (cmd != shn::FN_ZERO) {
                const uint32_t energy = r.uns(shn::kEnergySize);
                if (r.bad)
                    break;
                if (energy > 31u) {
                    status = ATG_SHN_UNSUPPORTED;
                    break;
                }
                if (cmd == shn::FN_QLPC) {
                    const uint32_t n = r.uns(shn::kLpcCountSize);
                    if (r.bad)
                        break;
                    if (n > ATG_SHN_MAX_LPC_COUNT) {
                        status = ATG_SHN_UNSUPPORTED;
                        break;
                    }
                    serial_skip(r, n, shn::kLpcCoeffSize + 1u);
                }
                skip(L, energy + 1u);
                if (r.bad)
                    break;
            }
            if (++c == C) {
                c = 0;
                frames += L;
                committed = nent;
                chb = hb;
                cfb = fb;
            }
        } else if (cmd == shn::FN_QUIT) {
            status = ATG_SHN_END_OF_STREAM;
            // the units of an unfinished set of channels have no frames to
            // go to; the VERBATIM commands among them still count
            committed = nent;
            chb = hb;
            cfb = fb;
            if (c)
                dead_from = set_start;
        } else if (cmd == shn::FN_BLOCKSIZE) {
            const uint32_t w = r.uns(2);
            if (r.bad)
                break;
            if (w > 32u) {
                status = ATG_SHN_UNSUPPORTED;
                break;
            }
            L = r.uns(w);
        } else if (cmd == shn::FN_BITSHIFT) {
            shift = r.uns(shn::kShiftSize);
            if (!r.bad && shift > 31u)
                status = ATG_SHN_UNSUPPORTED;
        } else if (cmd == shn::FN_VERBATIM) {
            const uint32_t size = r.uns(shn::kVerbatimChunkSize);
            if (r.bad)
                break;
            if (nent < T.ucap && lane == 0)
                mine[nent] = Entry{(uint32_t)r.pos, size, seen ? fb : hb,
                                   cmd | (seen ? kFooter : 0u)};
            ++nent;
            (seen ? fb : hb) += size;
            skip(size, shn::kVerbatimByteSize);
        } else {
            status = ATG_SHN_UNKNOWN_COMMAND;
        }
        if (r.bad)
            break;
    }
    if (r.bad && (status == ATG_SHN_OK))
        status = ATG_SHN_IOERROR;
    if (lane == 0) {
        DOut o;
        o.frames = frames;
        o.status = status;
        o.committed = committed;
        o.entries = nent;
        o.header_bytes = chb;
        o.footer_bytes = cfb;
        o.dead_from = dead_from;
        outs[blockIdx.x] = o;
    }
}

// -------------------------------------------------------------- parse pass
__device__ __forceinline__ uint32_t find_stream(const DTrack *__restrict__ tr, uint32_t n,
                                                uint64_t slot)
{
    return last_le(tr, n, slot, &DTrack::ubase);
}

__global__ __launch_bounds__(64) void k_shnd_parse(const uint8_t *__restrict__ data,
                                                   const DTrack *__restrict__ tracks,
                                                   uint32_t n_tracks,
                                                   const DOut *__restrict__ outs,
                                                   const Entry *__restrict__ entries,
                                                   uint64_t slots, int32_t *__restrict__ pcm,
                                                   uint8_t *__restrict__ verb)
{
    const uint64_t slot = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (slot >= slots)
        return;
    const uint32_t t = find_stream(tracks, n_tracks, slot);
    const DTrack T = tracks[t];
    const DOut O = outs[t];
    if (slot - T.ubase >= O.committed)
        return;
    const Entry U = entries[slot];
    const uint32_t cmd = U.meta & kCmdMask;
    shn::Window r; // the index pass has walked these codes: they end inside the image
    r.open(data + T.data_offset, T.data_bytes, U.bit);
    if (cmd == shn::FN_VERBATIM) {
        uint8_t *dst = verb + T.verb_at + ((U.meta & kFooter) ? O.header_bytes : 0u) + U.frame;
        for (uint32_t i = 0; i < U.length; ++i)
            dst[i] = (uint8_t)r.uns(shn::kVerbatimByteSize);
        return;
    }
    if (cmd == shn::FN_ZERO || slot - T.ubase >= O.dead_from)
        return;
    const uint32_t energy = r.uns(shn::kEnergySize);
    if (cmd == shn::FN_QLPC)
        for (uint32_t n = r.uns(shn::kLpcCountSize); n; --n)
            (void)r.uns(shn::kLpcCoeffSize + 1u);
    const uint32_t C = T.channels;
    int32_t *o = pcm + T.pcm_at + (uint64_t)U.frame * C + ((U.meta >> kChannelAt) & 0x1FFu);
    for (uint32_t i = 0; i < U.length; ++i)
        o[(uint64_t)i * C] = r.sgn(energy);
}

// -------------------------------------------------------------- recon pass
__device__ __forceinline__ int32_t shn_mean(int32_t half_plus_sum, int32_t n)
{
    return half_plus_sum / n; // C division: truncates toward zero
}

__global__ __launch_bounds__(64) void k_shnd_recon(const uint8_t *__restrict__ data,
                                                   const DTrack *__restrict__ tracks,
                                                   const DOut *__restrict__ outs,
                                                   const Entry *__restrict__ entries,
                                                   int32_t *__restrict__ pcm)
{
    __shared__ int32_t hist[kHist];
    __shared__ int32_t means[ATG_SHN_MAX_MEAN_COUNT];
    __shared__ int32_t coeff[ATG_SHN_MAX_LPC_COUNT];
    const DTrack T = tracks[blockIdx.x];
    const uint32_t c = blockIdx.y, lane = threadIdx.x;
    const uint32_t C = T.channels, mc = T.mean_count;
    const DOut O = outs[blockIdx.x];
    if (c >= C || !O.committed)
        return;
    const uint32_t K = min(max(3u, T.max_lpc), kHist);
    if (lane < ATG_SHN_MAX_MEAN_COUNT)
        means[lane] = 0;
    uint32_t histlen = 0;
    __syncthreads();
    const Entry *mine = entries + T.ubase;
    for (uint32_t k = 0; k < O.committed; ++k) {
        const Entry U = mine[k];
        const uint32_t cmd = U.meta & kCmdMask;
        if (cmd == shn::FN_VERBATIM || ((U.meta >> kChannelAt) & 0x1FFu) != c ||
            k >= O.dead_from)
            continue;
        const uint32_t L = U.length, shift = (U.meta >> kShiftAt) & 31u;
        int32_t *o = pcm + T.pcm_at + (uint64_t)U.frame * C + c;
        uint32_t offset = 0;
        if (cmd == shn::FN_DIFF0 || cmd == shn::FN_QLPC) {
            uint32_t s = mc / 2u;
            for (uint32_t j = 0; j < mc; ++j)
                s += (uint32_t)means[j];
            offset = (uint32_t)shn_mean((int32_t)s, (int32_t)mc);
        }
        // the carried samples, zeros in front of a short history
        const uint32_t h1 = histlen >= 1u ? (uint32_t)hist[histlen - 1u] : 0u;
        const uint32_t h2 = histlen >= 2u ? (uint32_t)hist[histlen - 2u] : 0u;
        const uint32_t h3 = histlen >= 3u ? (uint32_t)hist[histlen - 3u] : 0u;
        if (cmd == shn::FN_QLPC) {
            if (lane == 0) {
                shn::Bits r;
                r.open(data + T.data_offset, T.data_bytes, U.bit);
                (void)r.uns(shn::kEnergySize);
                const uint32_t n = r.uns(shn::kLpcCountSize);
                for (uint32_t j = 0; j < n; ++j)
                    coeff[j] = r.sgn(shn::kLpcCoeffSize);
                for (uint32_t i = 0; i < L; ++i) {
                    uint32_t sum = 32u;
                    for (uint32_t j = 0; j < n; ++j) {
                        uint32_t v;
                        if (i >= j + 1u) {
                            v = (uint32_t)o[(uint64_t)(i - j - 1u) * C];
                        } else {
                            // offset_samples[n + i - j - 1]: the last n carried
                            // samples, zeros in front
                            const uint32_t back = j + 1u - i; // 1..n from the end
                            v = (back <= histlen ? (uint32_t)hist[histlen - back] : 0u) - offset;
                        }
                        sum += (uint32_t)coeff[j] * v;
                    }
                    o[(uint64_t)i * C] =
                        (int32_t)((uint32_t)((int32_t)sum >> 5) + (uint32_t)o[(uint64_t)i * C]);
                }
            }
        }
        __syncthreads();
        const uint32_t keep = min(L, K);
        uint32_t c1 = h1, c2 = h1 - h2, c3 = (h1 - h2) - (h2 - h3); // sample, delta, delta of delta
        uint32_t total = 0;
        for (uint32_t i0 = 0; i0 < L; i0 += 64u) {
            const uint32_t i = i0 + lane;
            const bool valid = i < L;
            uint32_t x = (valid && cmd != shn::FN_ZERO) ? (uint32_t)o[(uint64_t)i * C] : 0u;
            if (cmd == shn::FN_DIFF0 || cmd == shn::FN_QLPC) {
                x += offset;
            } else if (cmd != shn::FN_ZERO) {
                if (cmd == shn::FN_DIFF3) {
                    x = wave_incl_scan_u32(x, (int)lane) + c3;
                    c3 = (uint32_t)__shfl((int)x, 63, 64);
                }
                if (cmd >= shn::FN_DIFF2) {
                    x = wave_incl_scan_u32(x, (int)lane) + c2;
                    c2 = (uint32_t)__shfl((int)x, 63, 64);
                }
                x = wave_incl_scan_u32(x, (int)lane) + c1;
                c1 = (uint32_t)__shfl((int)x, 63, 64);
            }
            if (valid) {
                total += x;
                if (i >= L - keep)
                    hist[i - (L - keep)] = (int32_t)x;
                o[(uint64_t)i * C] = (int32_t)((x << shift) - (uint32_t)T.adjust);
            }
        }
        histlen = keep;
        if (mc) {
            total = wave_sum_u32(total);
            const int32_t mean = shn_mean((int32_t)(L / 2u + total), (int32_t)L);
            __syncthreads();
            const int32_t next = lane + 1u < mc ? means[lane + 1u] : mean;
            __syncthreads();
            if (lane < mc)
                means[lane] = next;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------- host
thread_local ErrSlot g_shnd_err;
#define DHIP(expr) ATG_HIP_TRY(g_shnd_err, expr, #expr)

// "shnd_layout" is the host between the index and the parse: the copy of the
// streams' results, the PCM and VERBATIM extents and the second upload of
// the stream table
const int kDTimed = 5;
const char *kDNames[kDTimed] = {"shnd_index", "shnd_layout", "shnd_parse", "shnd_recon",
                                "shnd_total"};

// host reader for the header
struct HBits {
    const uint8_t *p;
    uint64_t nbits, pos = 0;
    bool bad = false;
    uint32_t read(uint32_t count)
    {
        uint32_t v = 0;
        if (bad || pos + count > nbits) {
            bad = true;
            return 0;
        }
        for (uint32_t k = 0; k < count; ++k, ++pos)
            v = (v << 1) | ((p[pos >> 3] >> (7u - (pos & 7u))) & 1u);
        return v;
    }
    uint32_t uns(uint32_t c)
    {
        uint32_t run = 0;
        for (;;) {
            if (bad || pos >= nbits) {
                bad = true;
                return 0;
            }
            if (read(1))
                break;
            ++run;
        }
        const uint32_t low = read(c);
        return (c < 32u ? run << c : 0u) | low;
    }
};

uint32_t le32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | (p[1] << 16) | (p[2] << 8) | p[3]; }

uint32_t ieee_extended(const uint8_t *b)
{
    const uint32_t sign = b[0] >> 7, exponent = ((b[0] & 0x7Fu) << 8) | b[1];
    uint64_t mantissa = 0;
    for (int i = 2; i < 10; ++i)
        mantissa = (mantissa << 8) | b[i];
    if (!exponent && !mantissa)
        return 0;
    if (exponent == 0x7FFF)
        return 0x7FFFFFFFu;
    const double f = (double)mantissa * std::pow(2.0, (double)exponent - 16383 - 63);
    if (!(f < 2147483648.0))
        return 0x7FFFFFFFu;
    const int32_t v = (int32_t)f;
    return (uint32_t)(sign ? -v : v);
}

// read_wave_header / read_aiff_header over the first VERBATIM's bytes
bool wave_fmt(const std::vector<uint8_t> &v, uint32_t *rate, uint32_t *mask)
{
    static const uint8_t pcm_guid[16] = {0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x10, 0x00,
                                         0x80, 0x00, 0x00, 0xaa, 0x00, 0x38, 0x9b, 0x71};
    static const uint32_t masks[7] = {0, 0x4, 0x3, 0x7, 0x33, 0x37, 0x3F};
    const size_t n = v.size();
    if (n < 12 || std::memcmp(&v[0], "RIFF", 4) || std::memcmp(&v[8], "WAVE", 4))
        return false;
    size_t p = 12;
    int64_t left = (int64_t)n - 12;
    while (left > 0) {
        if (p + 8 > n)
            return false;
        uint64_t size = le32(&v[p + 4]);
        const bool fmt = !std::memcmp(&v[p], "fmt ", 4);
        p += 8;
        left -= 8;
        if (fmt) {
            if (p + 16 > n)
                return false;
            const uint32_t comp = v[p] | (v[p + 1] << 8), ch = v[p + 2] | (v[p + 3] << 8);
            const uint32_t r = le32(&v[p + 4]);
            if (comp == 1) {
                *rate = r;
                *mask = ch < 7 ? masks[ch] : 0;
                return true;
            }
            if (comp == 0xFFFE) {
                if (p + 40 > n || std::memcmp(&v[p + 24], pcm_guid, 16))
                    return false;
                *rate = r;
                *mask = le32(&v[p + 20]);
                return true;
            }
            return false;
        }
        size += size & 1u;
        if (p + size > n)
            return false;
        p += size;
        left -= (int64_t)size;
    }
    return false;
}

bool aiff_comm(const std::vector<uint8_t> &v, uint32_t *rate, uint32_t *mask)
{
    const size_t n = v.size();
    if (n < 12 || std::memcmp(&v[0], "FORM", 4) || std::memcmp(&v[8], "AIFF", 4))
        return false;
    size_t p = 12;
    int64_t left = (int64_t)n - 12;
    while (left > 0) {
        if (p + 8 > n)
            return false;
        uint64_t size = be32(&v[p + 4]);
        const bool comm = !std::memcmp(&v[p], "COMM", 4);
        p += 8;
        left -= 8;
        if (comm) {
            if (p + 18 > n)
                return false;
            const uint32_t ch = (v[p] << 8) | v[p + 1];
            *rate = ieee_extended(&v[p + 8]);
            *mask = ch == 1 ? 0x4 : ch == 2 ? 0x3 : 0;
            return true;
        }
        size += size & 1u;
        if (p + size > n)
            return false;
        p += size;
        left -= (int64_t)size;
    }
    return false;
}

// the frame count audiotools/shn.py takes from a data / SSND chunk
uint64_t iff_total_frames(const std::vector<uint8_t> &v, uint32_t channels, uint32_t bps)
{
    uint64_t total = 0;
    const uint64_t per = (uint64_t)channels * (bps / 8);
    const size_t n = v.size();
    for (int aiff = 0; aiff < 2; ++aiff) {
        if (n < 12 || std::memcmp(&v[0], aiff ? "FORM" : "RIFF", 4) ||
            std::memcmp(&v[8], aiff ? "AIFF" : "WAVE", 4))
            continue;
        size_t p = 12;
        int64_t left = (int64_t)n - 12;
        while (left >= 8 && p + 8 <= n) {
            uint64_t size = aiff ? be32(&v[p + 4]) : le32(&v[p + 4]);
            const bool audio = !std::memcmp(&v[p], aiff ? "SSND" : "data", 4);
            const uint64_t sub = aiff ? 8 : 0;
            p += 8;
            left -= 8;
            if (audio) {
                if (per && size >= sub)
                    total = (size - sub) / per;
                continue;
            }
            size += size & 1u;
            if (p + size > n)
                break;
            p += size;
            left -= (int64_t)size;
        }
    }
    return total;
}

} // namespace

struct atg_shn_decoder : StageHandle<kDTimed> {
    DevBuf tracks, outs, entries, pcm, verb, h_data;
    uint64_t samples = 0, verb_bytes = 0;
    int coop = 1;
    std::vector<DTrack> last_tracks; // of the last decode, for fetch_blocks
    std::vector<DOut> last_outs;
};

namespace {

atg_status shnd_run(atg_shn_decoder *dec, const uint8_t *d_data, uint64_t len,
                    const atg_shn_dec_track *tracks, uint32_t n, atg_shn_dec_result *res,
                    uint64_t *total_samples)
{
    hipStream_t s = dec->s;
    std::vector<DTrack> T(n);
    for (uint32_t t = 0; t < n; ++t) {
        const atg_shn_dec_track &in = tracks[t];
        if (in.data_offset & 3u)
            return g_shnd_err.fail(ATG_ERR_INVALID, "images must start 4-byte aligned");
        if (in.data_offset > len || in.data_bytes > len - in.data_offset)
            return g_shnd_err.fail(ATG_ERR_INVALID, "an image lies outside the data");
        if (in.data_bytes >= (1ull << 29))
            return g_shnd_err.fail(ATG_ERR_UNSUPPORTED, "an image of 512 MiB or more");
        if (in.first_command_bit > in.data_bytes * 8u)
            return g_shnd_err.fail(ATG_ERR_INVALID, "first_command_bit outside the image");
        if (in.file_type < 1 || in.file_type > 6)
            return g_shnd_err.fail(ATG_ERR_INVALID, "file type must be 1..6");
        DTrack &D = T[t];
        std::memset(&D, 0, sizeof(D));
        D.data_offset = in.data_offset;
        D.data_bytes = in.data_bytes;
        D.start_bit = in.first_command_bit;
        D.channels = in.channels;
        D.block_length = in.block_length;
        D.max_lpc = in.max_lpc;
        D.mean_count = in.mean_count;
        const bool sgn = in.file_type == 1 || in.file_type == 3 || in.file_type == 5;
        D.adjust = sgn ? 0 : (in.file_type <= 2 ? 128 : 32768);
        // a guess at the commands: an audio command of L residuals takes at
        // least 5 + 2 L bits; a stream with more (ZERO commands, smaller
        // blocks) reports its count and the index pass runs again
        const uint64_t guess = in.data_bytes * 8u / (5u + 2ull * std::min(in.block_length, 4096u)) + 64u;
        D.ucap = (uint32_t)std::min<uint64_t>(guess, 0x7FFFFFFFu);
    }
    DHIP(dec->tracks.ensure(sizeof(DTrack) * std::max<uint32_t>(n, 1)));
    DHIP(dec->outs.ensure(sizeof(DOut) * std::max<uint32_t>(n, 1)));
    std::vector<DOut> O(n);
    uint64_t slots = 0;
    for (int pass = 0; pass < 2; ++pass) {
        slots = 0;
        for (uint32_t t = 0; t < n; ++t) {
            T[t].ubase = slots;
            slots += T[t].ucap;
        }
        DHIP(dec->entries.ensure(sizeof(Entry) * std::max<uint64_t>(slots, 1)));
        if (n)
            DHIP(hipMemcpyAsync(dec->tracks.p, T.data(), sizeof(DTrack) * n,
                                hipMemcpyHostToDevice, s));
        DHIP(hipEventRecord(dec->ev[0], s));
        if (n)
            hipLaunchKernelGGL(k_shnd_index, dim3(n), dim3(64), 0, s, d_data,
                               (const DTrack *)dec->tracks.p, (Entry *)dec->entries.p,
                               (DOut *)dec->outs.p, dec->coop);
        DHIP(hipGetLastError());
        DHIP(hipEventRecord(dec->ev[1], s));
        if (n)
            DHIP(hipMemcpyAsync(O.data(), dec->outs.p, sizeof(DOut) * n, hipMemcpyDeviceToHost,
                                s));
        DHIP(hipStreamSynchronize(s));
        bool again = false;
        for (uint32_t t = 0; t < n; ++t)
            if (O[t].entries > T[t].ucap) {
                T[t].ucap = O[t].entries;
                again = true;
            }
        if (!again)
            break;
    }
    uint64_t samples = 0, vbytes = 0;
    for (uint32_t t = 0; t < n; ++t) {
        atg_shn_dec_result &r = res[t];
        T[t].pcm_at = samples;
        T[t].verb_at = vbytes;
        r.pcm_offset = samples;
        r.pcm_frames = O[t].frames;
        r.status = (int32_t)O[t].status;
        r.header_bytes = O[t].header_bytes;
        r.footer_bytes = O[t].footer_bytes;
        r.verbatim_offset = vbytes;
        samples += O[t].frames * T[t].channels;
        vbytes += (uint64_t)O[t].header_bytes + O[t].footer_bytes;
    }
    dec->samples = samples;
    dec->verb_bytes = vbytes;
    dec->last_tracks = T;
    dec->last_outs = O;
    if (total_samples)
        *total_samples = samples;
    DHIP(dec->pcm.ensure(sizeof(int32_t) * std::max<uint64_t>(samples, 1)));
    DHIP(dec->verb.ensure(std::max<uint64_t>(vbytes, 1)));
    if (n)
        DHIP(hipMemcpyAsync(dec->tracks.p, T.data(), sizeof(DTrack) * n, hipMemcpyHostToDevice,
                            s));
    DHIP(hipEventRecord(dec->ev[2], s));
    if (slots > 0x7FFFFFFFull * 64u)
        return g_shnd_err.fail(ATG_ERR_UNSUPPORTED, "too many Shorten commands in one batch");
    if (n && slots)
        hipLaunchKernelGGL(k_shnd_parse, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, s,
                           d_data, (const DTrack *)dec->tracks.p, n, (const DOut *)dec->outs.p,
                           (const Entry *)dec->entries.p, slots, (int32_t *)dec->pcm.p,
                           (uint8_t *)dec->verb.p);
    DHIP(hipGetLastError());
    DHIP(hipEventRecord(dec->ev[3], s));
    uint32_t maxc = 0;
    for (uint32_t t = 0; t < n; ++t)
        if (O[t].committed)
            maxc = std::max(maxc, T[t].channels);
    if (maxc)
        hipLaunchKernelGGL(k_shnd_recon, dim3(n, maxc), dim3(64), 0, s, d_data,
                           (const DTrack *)dec->tracks.p, (const DOut *)dec->outs.p,
                           (const Entry *)dec->entries.p, (int32_t *)dec->pcm.p);
    DHIP(hipGetLastError());
    DHIP(hipEventRecord(dec->ev[4], s));
    DHIP(hipStreamSynchronize(s));
    dec->finish_times();
    return ATG_OK;
}

} // namespace

extern "C" {

const char *atg_shn_decoder_last_error(void) { return g_shnd_err.msg.c_str(); }

int atg_shn_read_info(const uint8_t *data, uint64_t len, atg_shn_info *info)
{
    if (!data || !info)
        return ATG_SHN_IOERROR;
    std::memset(info, 0, sizeof(*info));
    HBits r{data, len * 8u};
    uint8_t magic[4];
    for (int i = 0; i < 4; ++i)
        magic[i] = (uint8_t)r.read(8);
    const uint32_t version = r.read(8);
    if (r.bad)
        return ATG_SHN_IOERROR;
    if (std::memcmp(magic, "ajkg", 4))
        return ATG_SHN_INVALID_MAGIC_NUMBER;
    if (version != 2)
        return ATG_SHN_INVALID_SHORTEN_VERSION;
    uint32_t f[6];
    for (int i = 0; i < 6; ++i) {
        const uint32_t w = r.uns(2);
        if (r.bad)
            return ATG_SHN_IOERROR;
        if (w > 32u)
            return ATG_SHN_UNSUPPORTED;
        f[i] = r.uns(w);
        if (r.bad)
            return ATG_SHN_IOERROR;
    }
    if (r.pos + 8ull * f[5] > r.nbits)
        return ATG_SHN_IOERROR;
    r.pos += 8ull * f[5];
    info->file_type = f[0];
    info->channels = f[1];
    info->block_length = f[2];
    info->max_lpc = f[3];
    info->mean_count = f[4];
    info->bytes_to_skip = f[5];
    if (f[0] >= 1 && f[0] <= 2) {
        info->bits_per_sample = 8;
        info->signed_samples = f[0] == 1;
    } else if (f[0] >= 3 && f[0] <= 6) {
        info->bits_per_sample = 16;
        info->signed_samples = f[0] == 3 || f[0] == 5;
    } else {
        return ATG_SHN_UNSUPPORTED_FILE_TYPE;
    }
    info->sample_rate = 44100;
    info->channel_mask = 0;
    info->first_command_bit = r.pos;
    const uint32_t cmd = r.uns(shn::kCommandSize);
    if (r.bad)
        return ATG_SHN_IOERROR;
    if (cmd == shn::FN_VERBATIM) {
        const uint32_t size = r.uns(shn::kVerbatimChunkSize);
        std::vector<uint8_t> v;
        for (uint32_t i = 0; i < size && !r.bad; ++i)
            v.push_back((uint8_t)r.uns(shn::kVerbatimByteSize));
        if (r.bad)
            return ATG_SHN_IOERROR;
        uint32_t rate = 0, mask = 0;
        if (wave_fmt(v, &rate, &mask) || aiff_comm(v, &rate, &mask)) {
            info->sample_rate = rate;
            info->channel_mask = mask;
        }
        info->total_pcm_frames = iff_total_frames(v, info->channels, info->bits_per_sample);
    }
    return ATG_SHN_OK;
}

atg_status atg_shn_decoder_create(int device, atg_shn_decoder **out)
{
    return open_handle(device, out, g_shnd_err, "decoder create");
}

void atg_shn_decoder_destroy(atg_shn_decoder *d)
{
    if (!d)
        return;
    d->close({&d->tracks, &d->outs, &d->entries, &d->pcm, &d->verb, &d->h_data});
    delete d;
}

atg_status atg_shn_decoder_set_index_walk(atg_shn_decoder *d, int cooperative)
{
    ATG_HANDLE_LOCK(d);
    if (!d)
        return g_shnd_err.fail(ATG_ERR_INVALID, "NULL argument");
    d->coop = cooperative ? 1 : 0;
    return ATG_OK;
}

atg_status atg_shn_decode_device(atg_shn_decoder *d, const void *d_data, uint64_t len,
                                 const atg_shn_dec_track *tracks, uint32_t n_tracks,
                                 atg_shn_dec_result *results, const int32_t **d_pcm,
                                 uint64_t *total_samples)
{
    ATG_HANDLE_LOCK(d);
    if (!d || (!tracks && n_tracks) || (!results && n_tracks) || (!d_data && len))
        return g_shnd_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (((uintptr_t)d_data) & 3)
        return g_shnd_err.fail(ATG_ERR_INVALID, "d_data must be 4-byte aligned");
    DHIP(hipSetDevice(d->device));
    atg_status st = shnd_run(d, (const uint8_t *)d_data, len, tracks, n_tracks, results,
                             total_samples);
    if (st == ATG_OK && d_pcm)
        *d_pcm = (const int32_t *)d->pcm.p;
    return st;
}

atg_status atg_shn_decode_host(atg_shn_decoder *d, const uint8_t *data, uint64_t len,
                               const atg_shn_dec_track *tracks, uint32_t n_tracks,
                               atg_shn_dec_result *results, uint64_t *total_samples)
{
    ATG_HANDLE_LOCK(d);
    if (!d || (!tracks && n_tracks) || (!results && n_tracks) || (!data && len))
        return g_shnd_err.fail(ATG_ERR_INVALID, "NULL argument");
    DHIP(hipSetDevice(d->device));
    DHIP(d->h_data.ensure(std::max<uint64_t>(len, 4)));
    if (len)
        DHIP(hipMemcpyAsync(d->h_data.p, data, len, hipMemcpyHostToDevice, d->s));
    return shnd_run(d, (const uint8_t *)d->h_data.p, len, tracks, n_tracks, results,
                    total_samples);
}

atg_status atg_shn_decode_fetch(atg_shn_decoder *d, int32_t *pcm, uint64_t pcm_cap)
{
    ATG_HANDLE_LOCK(d);
    if (!d || (!pcm && d->samples))
        return g_shnd_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (pcm_cap < d->samples)
        return g_shnd_err.fail(ATG_ERR_CAPACITY, "pcm buffer smaller than the decoded batch");
    DHIP(hipSetDevice(d->device));
    if (d->samples)
        DHIP(hipMemcpy(pcm, d->pcm.p, sizeof(int32_t) * d->samples, hipMemcpyDeviceToHost));
    return ATG_OK;
}

atg_status atg_shn_decode_fetch_verbatim(atg_shn_decoder *d, uint8_t *bytes, uint64_t cap)
{
    ATG_HANDLE_LOCK(d);
    if (!d || (!bytes && d->verb_bytes))
        return g_shnd_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (cap < d->verb_bytes)
        return g_shnd_err.fail(ATG_ERR_CAPACITY, "buffer smaller than the VERBATIM bytes");
    DHIP(hipSetDevice(d->device));
    if (d->verb_bytes)
        DHIP(hipMemcpy(bytes, d->verb.p, d->verb_bytes, hipMemcpyDeviceToHost));
    return ATG_OK;
}

atg_status atg_shn_decode_fetch_blocks(atg_shn_decoder *d, uint32_t track, uint32_t *lengths,
                                       uint64_t cap, uint64_t *n_blocks)
{
    ATG_HANDLE_LOCK(d);
    if (!d || !n_blocks || (!lengths && cap))
        return g_shnd_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (track >= d->last_tracks.size())
        return g_shnd_err.fail(ATG_ERR_INVALID, "no such stream in the last decode");
    DHIP(hipSetDevice(d->device));
    const uint32_t n = d->last_outs[track].committed;
    std::vector<Entry> e(n);
    if (n)
        DHIP(hipMemcpy(e.data(), (const Entry *)d->entries.p + d->last_tracks[track].ubase,
                       sizeof(Entry) * n, hipMemcpyDeviceToHost));
    uint64_t k = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const Entry &u = e[i];
        if ((u.meta & kCmdMask) == shn::FN_VERBATIM || ((u.meta >> kChannelAt) & 0x1FFu) ||
            i >= d->last_outs[track].dead_from)
            continue;
        if (k < cap)
            lengths[k] = u.length;
        ++k;
    }
    *n_blocks = k;
    if (k > cap)
        return g_shnd_err.fail(ATG_ERR_CAPACITY, "lengths holds fewer entries than the stream "
                                                 "has blocks");
    return ATG_OK;
}

int atg_shn_decoder_kernel_times(atg_shn_decoder *d, const char **names, float *ms, int cap)
{
    ATG_HANDLE_LOCK(d);
    return d ? d->report(kDNames, names, ms, cap) : 0;
}

} // extern "C"
