// flac_index.hip — the frame starts inside byte ranges of FLAC frame data
// (include/atgpu_flac_index.h): the table a FLAC stream does not carry, made
// on the device so that a window of a long file can start at the frame that
// holds it.  One call covers a ragged table of ranges; the listing rule is in
// the header and, restated in numpy, in tests/flac_index_port.py.
//
// Three passes, shaped as the decoder's front (flac_decode.hip K1, K1b, K2s):
//
//   k_ix_sync     lane per 16 input bytes, over host-listed segments of the
//                 ranges only: every byte that starts a sync code (0xFF, then
//                 0xF8 or 0xF9) is listed with its range.  Hits gather in LDS
//                 and leave with one global atomic per workgroup.
//   k_ix_header   lane per hit: the frame header parse with CRC-8 and the
//                 STREAMINFO checks the decoder makes, keeping what the
//                 decoder drops -- the blocking-strategy bit and the UTF-8
//                 number.  Survivors are the candidates; each sets its bit in
//                 a bitmap laid out range after range.
//   k_ix_confirm  wave per candidate p: the later candidates q of the range
//                 in turn (the bitmap walk), then the range's end, as far as
//                 the frame bound; the CRC-16 state over [p, q) is carried
//                 from q to q (crc(A || B) = advance(crc(A), |B|) ^ crc(B)),
//                 so a candidate costs one pass over the bound at most.  The
//                 first q with a zero residue whose number follows p's lists p.
//
// The counts stay on the device; a list that overflows its capacity is
// answered by one re-run with room for all.  Entries leave unordered and the
// host sorts them by (range, byte offset).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/atgpu.h"
#include "crc_common.h"
#include "host_common.h"

namespace {

thread_local ErrSlot g_ix_err;
#define IHIP(expr) ATG_HIP_TRY(g_ix_err, expr, #expr)

constexpr uint32_t kBlock = 256;
constexpr uint32_t kSegChunks = 4096; // 16-byte chunks of a segment: 64 KB
constexpr uint32_t kMaxBlocks = 2048;
constexpr uint32_t kLocal = 1024;     // hits a workgroup gathers in LDS
constexpr uint32_t kMinFrame = 9;     // bytes: header, a subframe byte, CRC-16
constexpr uint64_t kMaxFrame = 1ull << 22;
constexpr int kStages = 3;
const char *const kStageNames[kStages] = {"sync", "header", "confirm"};
thread_local StageTimes<kStages> g_ix_times;

struct IxTables {
    uint16_t crc16[4][256]; // slicing by 4
    uint16_t adv[24][16];   // the state after 2^m zero bytes
    uint8_t crc8[256];
};

// what the kernels know of a range
struct IxRange {
    uint64_t start, end; // absolute bytes of the buffer
    uint64_t bit0;       // its first bit of the candidate bitmap (a multiple of 64)
    uint32_t rate, channels, bps, max_bs, fixed_bs;
    uint32_t bound;      // frame bound, bytes
};

struct IxSeg {
    uint64_t c0; // first 16-byte chunk of the buffer
    uint32_t n;  // chunks
    uint32_t range;
};

struct IxHit {
    uint64_t pos;
    uint32_t range, pad;
};

// a candidate, and with `number` turned into the first sample an entry
struct IxCand {
    uint64_t pos;    // absolute byte
    uint64_t number; // frame number (fixed blocking) or sample number
    uint32_t bs;
    uint32_t range;  // bit 31: variable blocking
};

struct IxCounts {
    uint32_t hits, cands, entries, pad;
};

struct IxCtx {
    DevBuf tables, ranges, segs, hits, cands, entries, bits, counts;
    bool have_tables = false;
    hipEvent_t ev[kStages + 1] = {};
};
DeviceContexts<IxCtx> g_ctxs;

__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// 0xFF then 0xF8/0xF9 at byte k of the big-endian pair a:b
__device__ __forceinline__ bool sync_at(uint32_t a, uint32_t b, int k)
{
    const uint64_t pair = ((uint64_t)a << 32) | b;
    return ((uint32_t)(pair >> (48 - 8 * k)) & 0xFFFEu) == 0xFFF8u;
}

__global__ __launch_bounds__(kBlock) void k_ix_sync(const uint32_t *__restrict__ w, uint64_t nw,
                                                    const IxRange *__restrict__ rg,
                                                    const IxSeg *__restrict__ segs, uint32_t nseg,
                                                    IxCounts *__restrict__ cnt, uint32_t hcap,
                                                    IxHit *__restrict__ hits)
{
    __shared__ IxHit lhit[kLocal];
    __shared__ uint32_t lcnt, lbase;
    if (threadIdx.x == 0)
        lcnt = 0;
    __syncthreads();
    const bool a16 = ((uintptr_t)w & 15u) == 0; // the API promises 4-byte alignment only
    for (uint32_t sg = blockIdx.x; sg < nseg; sg += gridDim.x) {
        const IxSeg S = segs[sg];
        const uint64_t r0 = rg[S.range].start, r1 = rg[S.range].end;
        for (uint64_t c = S.c0 + threadIdx.x, ce = S.c0 + S.n; c < ce; c += blockDim.x) {
            uint32_t v[5];
            if (a16 && 4 * c + 4 <= nw) {
                const uint4 q = *(const uint4 *)(w + 4 * c);
                v[0] = q.x;
                v[1] = q.y;
                v[2] = q.z;
                v[3] = q.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    v[i] = 4 * c + i < nw ? w[4 * c + i] : 0u;
            }
            v[4] = 4 * c + 4 < nw ? w[4 * c + 4] : 0u;
            uint32_t m = 0; // bit 4j+k: a sync pattern at byte 4j+k of the chunk
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t a = bswap32(v[j]), b = bswap32(v[j + 1]);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    m |= sync_at(a, b, k) ? 1u << (4 * j + k) : 0u;
            }
            while (m) {
                const int bit = __builtin_ctz(m);
                m &= m - 1;
                const uint64_t p = 16 * c + (uint64_t)bit;
                if (p < r0 || p + 2 > r1) // the chunks round the range outwards
                    continue;
                IxHit h;
                h.pos = p;
                h.range = S.range;
                h.pad = 0;
                const uint32_t i = atomicAdd(&lcnt, 1u);
                if (i < kLocal) {
                    lhit[i] = h;
                } else { // a dense run of patterns: straight to the list
                    const uint32_t g = atomicAdd(&cnt->hits, 1u);
                    if (g < hcap) // over capacity: the host runs again with room for all
                        hits[g] = h;
                }
            }
        }
    }
    __syncthreads();
    const uint32_t nl = min(lcnt, kLocal);
    if (threadIdx.x == 0)
        lbase = nl ? atomicAdd(&cnt->hits, nl) : 0u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nl; i += blockDim.x)
        if (lbase + i < hcap)
            hits[lbase + i] = lhit[i];
}

// The frame header at byte p of range R (flac.c:710-851 as the decoder reads
// it: the reserved bit after the sample size and the form of the UTF-8
// continuation bytes are not checked), at most 16 bytes: 4 fixed, 1-7 of the
// number, 0-2 of the block size, 0-2 of the rate, CRC-8.  False unless it
// parses inside the range, passes CRC-8 and agrees with STREAMINFO.
__device__ bool ix_header(const uint32_t *__restrict__ w, uint64_t last, uint64_t p,
                          const IxRange &R, const uint8_t *__restrict__ crc8, IxCand &c)
{
    if (p + 6 > R.end)
        return false;
    const uint64_t hi = ((uint64_t)be32_at(w, last, p) << 32) | be32_at(w, last, p + 4);
    const uint64_t lo = ((uint64_t)be32_at(w, last, p + 8) << 32) | be32_at(w, last, p + 12);
    auto B = [&](uint32_t i) -> uint32_t {
        return (uint32_t)((i < 8 ? hi >> (56 - 8 * i) : lo >> (120 - 8 * i)) & 0xFFu);
    };
    if (B(0) != 0xFFu || (B(1) & 0xFEu) != 0xF8u)
        return false;
    const uint32_t variable = B(1) & 1u;
    const uint32_t bs_bits = B(2) >> 4, sr_bits = B(2) & 15u;
    const uint32_t assign = B(3) >> 4;
    const uint32_t ch = (assign >= 8 && assign <= 10) ? 2u : assign + 1u;
    uint32_t bps;
    switch ((B(3) >> 1) & 7u) {
    case 0: bps = R.bps; break;
    case 1: bps = 8; break;
    case 2: bps = 12; break;
    case 4: bps = 16; break;
    case 5: bps = 20; break;
    case 6: bps = 24; break;
    default: return false;
    }
    // the number: leading 1 bits of the first byte count the bytes
    const uint32_t b4 = B(4);
    const uint32_t ones = __builtin_clz(~(b4 << 24) | 1u);
    if (ones > 7)
        return false;
    uint64_t number = ones >= 7 ? 0u : b4 & (0x7Fu >> ones);
    uint32_t n = 5;
    for (uint32_t k = 1; k < ones; ++k)
        number = (number << 6) | (B(n++) & 0x3Fu);
    uint32_t bs;
    switch (bs_bits) {
    case 0: bs = R.max_bs; break;
    case 1: bs = 192; break;
    case 2: case 3: case 4: case 5: bs = 576u << (bs_bits - 2); break;
    case 6: bs = B(n) + 1; n += 1; break;
    case 7: bs = ((B(n) << 8) | B(n + 1)) + 1; n += 2; break;
    default: bs = 256u << (bs_bits - 8); break;
    }
    uint32_t rate;
    switch (sr_bits) {
    case 0: rate = R.rate; break;
    case 1: rate = 88200; break;
    case 2: rate = 176400; break;
    case 3: rate = 192000; break;
    case 4: rate = 8000; break;
    case 5: rate = 16000; break;
    case 6: rate = 22050; break;
    case 7: rate = 24000; break;
    case 8: rate = 32000; break;
    case 9: rate = 44100; break;
    case 10: rate = 48000; break;
    case 11: rate = 96000; break;
    case 12: rate = B(n) * 1000; n += 1; break;
    case 13: rate = (B(n) << 8) | B(n + 1); n += 2; break;
    case 14: rate = ((B(n) << 8) | B(n + 1)) * 10; n += 2; break;
    default: return false;
    }
    n += 1; // CRC-8
    if (p + n > R.end)
        return false;
    uint32_t crc = 0;
    for (uint32_t i = 0; i < n; ++i)
        crc = crc8[crc ^ B(i)];
    if (crc || rate != R.rate || ch != R.channels || bps != R.bps || bs > R.max_bs)
        return false;
    c.pos = p;
    c.number = number;
    c.bs = bs;
    c.range = variable << 31;
    return true;
}

__global__ __launch_bounds__(kBlock) void k_ix_header(const uint32_t *__restrict__ w, uint64_t nw,
                                                      const IxRange *__restrict__ rg,
                                                      const IxTables *__restrict__ tab,
                                                      IxCounts *__restrict__ cnt, uint32_t hcap,
                                                      const IxHit *__restrict__ hits,
                                                      uint32_t ccap, IxCand *__restrict__ cands,
                                                      unsigned long long *__restrict__ bits)
{
    const uint32_t n = min(cnt->hits, hcap);
    for (uint32_t h = blockIdx.x * blockDim.x + threadIdx.x; h < n;
         h += gridDim.x * blockDim.x) {
        const IxHit H = hits[h];
        const IxRange R = rg[H.range];
        IxCand c;
        if (!ix_header(w, nw - 1, H.pos, R, tab->crc8, c))
            continue;
        c.range |= H.range;
        const uint32_t i = atomicAdd(&cnt->cands, 1u);
        if (i < ccap) // over capacity: the host runs again with room for all
            cands[i] = c;
        const uint64_t b = R.bit0 + (H.pos - R.start);
        atomicOr(&bits[b >> 6], 1ull << (b & 63u));
    }
}

// The first set bit of the bitmap in [from, to), or `to`: 64 words a step,
// one per lane.  Wave-uniform arguments and result.
__device__ __forceinline__ uint64_t next_bit(const unsigned long long *__restrict__ bits,
                                             uint64_t from, uint64_t to, uint32_t lane)
{
    uint64_t wi = from >> 6;
    bool first = true;
    while (wi * 64u < to) {
        const uint64_t k = wi + lane;
        unsigned long long x = k * 64u < to ? bits[k] : 0ull;
        if (first && lane == 0)
            x &= ~0ull << (from & 63u);
        first = false;
        const unsigned long long b = __ballot(x != 0ull);
        if (b) {
            const uint32_t f = (uint32_t)__builtin_ctzll(b);
            const unsigned long long xf = (unsigned long long)__shfl((long long)x, (int)f, 64);
            const uint64_t q = (wi + f) * 64u + (uint64_t)__builtin_ctzll(xf);
            return q < to ? q : to;
        }
        wi += 64u;
    }
    return to;
}

__device__ __forceinline__ uint32_t crc16_word(const uint16_t (*T)[256], uint32_t crc, uint32_t x)
{
    const uint32_t t = x ^ (crc << 16);
    return (uint32_t)T[3][t >> 24] ^ T[2][(t >> 16) & 0xFFu] ^ T[1][(t >> 8) & 0xFFu] ^
           T[0][t & 0xFFu];
}

// CRC-16 (zero start) of bytes [pos, pos + L), 0 < L <= 2^22, on one wave:
// the image is given a virtual prefix of zero bytes (which leave a zero state
// unchanged) up to 64 chunks of Lc = 2^m >= 4 bytes, a lane takes a chunk by
// 4-byte words, and the lanes' states combine in a tree with the advance
// matrices.  Wave-uniform arguments; the result is in every lane.
__device__ uint32_t wave_crc16(const uint32_t *__restrict__ w, uint64_t last, uint64_t pos,
                               uint32_t L, const uint16_t (*T)[256],
                               const uint16_t (*__restrict__ adv)[16], uint32_t lane)
{
    uint32_t lc_log = 2;
    while ((64u << lc_log) < L)
        lc_log++;
    const uint32_t Lc = 1u << lc_log;
    const int64_t z = (int64_t)(64u << lc_log) - (int64_t)L;
    uint32_t crc = 0;
    int64_t q = (int64_t)lane * Lc - z; // image byte of this lane's first word
    const int64_t qe = q + Lc;
    if (q < 0) {
        q += ((-q) >> 2) << 2; // words inside the prefix; now -4 < q <= 0
        if (q < 0 && q < qe) { // the word the image starts in
            crc = crc16_word(T, 0u, be32_at(w, last, pos) >> (8u * (uint32_t)(-q)));
            q += 4;
        }
    }
    for (; q + 32 <= qe; q += 32) { // eight loads in flight
        uint32_t x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            x[u] = be32_at(w, last, pos + (uint64_t)(q + 4 * u));
#pragma unroll
        for (int u = 0; u < 8; ++u)
            crc = crc16_word(T, crc, x[u]);
    }
    for (; q < qe; q += 4)
        crc = crc16_word(T, crc, be32_at(w, last, pos + (uint64_t)q));
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t other = (uint32_t)__shfl_down((int)crc, 1 << k, 64);
        if ((lane & ((2u << k) - 1u)) == 0)
            crc = crc_advance<16>(adv[lc_log + k], crc) ^ other;
    }
    return (uint32_t)__shfl((int)crc, 0, 64);
}

// the state after n more zero bytes, n < 2^24
__device__ __forceinline__ uint32_t crc16_skip(const uint16_t (*__restrict__ adv)[16],
                                               uint32_t crc, uint32_t n)
{
    for (uint32_t m = 0; n; ++m, n >>= 1)
        if (n & 1u)
            crc = crc_advance<16>(adv[m], crc);
    return crc;
}

__global__ __launch_bounds__(kBlock) void k_ix_confirm(const uint32_t *__restrict__ w, uint64_t nw,
                                                       const IxRange *__restrict__ rg,
                                                       const IxTables *__restrict__ tab,
                                                       IxCounts *__restrict__ cnt, uint32_t ccap,
                                                       const IxCand *__restrict__ cands,
                                                       const unsigned long long *__restrict__ bits,
                                                       IxCand *__restrict__ entries)
{
    __shared__ uint16_t T[4][256];
    for (uint32_t i = threadIdx.x; i < 4 * 256; i += blockDim.x)
        T[i >> 8][i & 255] = tab->crc16[i >> 8][i & 255];
    __syncthreads();
    const uint32_t n = min(cnt->cands, ccap);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t last = nw - 1;
    for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += gridDim.x * 4u) {
        const IxCand P = cands[i]; // wave-uniform from here on
        const IxRange R = rg[P.range & 0x7FFFFFFFu];
        const uint64_t p = P.pos;
        const uint64_t to = R.bit0 + (R.end - R.start);
        uint64_t prev = p;
        uint32_t crc = 0;
        bool listed = false;
        while (!listed && prev < R.end) {
            const uint64_t qb = next_bit(bits, R.bit0 + (prev - R.start) + 1u, to, lane);
            const uint64_t q = R.start + (qb - R.bit0);
            if (q - p > R.bound)
                break;
            const uint32_t L = (uint32_t)(q - prev);
            crc = crc16_skip(tab->adv, crc, L) ^ wave_crc16(w, last, prev, L, T, tab->adv, lane);
            prev = q;
            if (crc || q - p < kMinFrame)
                continue;
            if (q == R.end) {
                listed = true;
            } else {
                IxCand Q;
                if (ix_header(w, last, q, R, tab->crc8, Q) && (Q.range >> 31) == (P.range >> 31))
                    listed = Q.number == P.number + ((P.range >> 31) ? (uint64_t)P.bs : 1u);
            }
        }
        if (listed && lane == 0) {
            IxCand E = P;
            E.range &= 0x7FFFFFFFu;
            if (!(P.range >> 31))
                E.number = P.number * R.fixed_bs;
            entries[atomicAdd(&cnt->entries, 1u)] = E; // entries hold ccap, and n <= ccap
        }
    }
}

atg_status check_args(const void *data, uint64_t len, const atg_flac_index_range *ranges,
                      uint32_t n, const atg_flac_index_entry *entries, uint64_t cap,
                      const uint64_t *n_entries, uint64_t *scan_bytes)
{
    if (n && !ranges)
        return g_ix_err.fail(ATG_ERR_INVALID, "ranges is NULL with n_ranges > 0");
    if (!n_entries)
        return g_ix_err.fail(ATG_ERR_INVALID, "n_entries is NULL");
    if (cap && !entries)
        return g_ix_err.fail(ATG_ERR_INVALID, "entries is NULL with entry_cap > 0");
    if (n >= (1u << 31))
        return g_ix_err.fail(ATG_ERR_UNSUPPORTED, "2^31 ranges or more");
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const atg_flac_index_range &r = ranges[i];
        const std::string at = "range " + std::to_string(i) + ": ";
        if (r.data_offset > len || r.data_bytes > len - r.data_offset)
            return g_ix_err.fail(ATG_ERR_INVALID, at + "data_offset + data_bytes passes len");
        if (r.channels < 1 || r.channels > 8)
            return g_ix_err.fail(ATG_ERR_INVALID, at + "channels outside 1..8");
        if (r.bits_per_sample < 4 || r.bits_per_sample > 32)
            return g_ix_err.fail(ATG_ERR_INVALID, at + "bits_per_sample outside 4..32");
        if (r.max_block_size < 1 || r.max_block_size > 65535)
            return g_ix_err.fail(ATG_ERR_INVALID, at + "max_block_size outside 1..65535");
        if (r.min_block_size > r.max_block_size)
            return g_ix_err.fail(ATG_ERR_INVALID, at + "min_block_size above max_block_size");
        if (r.reserved)
            return g_ix_err.fail(ATG_ERR_INVALID, at + "reserved must be 0");
        if (r.data_bytes >= kMinFrame)
            total += r.data_bytes;
        if (total >= (1ull << 40))
            return g_ix_err.fail(ATG_ERR_UNSUPPORTED, "2^40 bytes of ranges or more");
    }
    if (total && !data)
        return g_ix_err.fail(ATG_ERR_INVALID, "data is NULL with bytes to scan");
    *scan_bytes = total;
    return ATG_OK;
}

uint32_t frame_bound(const atg_flac_index_range &r)
{
    const uint64_t sub = ((uint64_t)r.max_block_size * (r.bits_per_sample + 1) + 7) / 8 + 8;
    return (uint32_t)std::min<uint64_t>(kMaxFrame, 64 + 2 * r.channels * sub);
}

uint32_t grid_for(uint64_t items, uint32_t per_block)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block,
                                                               kMaxBlocks));
}

} // namespace

extern "C" {

const char *atg_flac_index_last_error(void) { return g_ix_err.msg.c_str(); }

atg_status atg_flac_index_device(const void *d_data, uint64_t len,
                                 const atg_flac_index_range *ranges, uint32_t n_ranges,
                                 atg_flac_index_entry *entries, uint64_t entry_cap,
                                 uint64_t *n_entries, void *stream)
{
    uint64_t scan = 0;
    atg_status st = check_args(d_data, len, ranges, n_ranges, entries, entry_cap, n_entries, &scan);
    if (st != ATG_OK)
        return st;
    if (scan && ((uintptr_t)d_data & 3u))
        return g_ix_err.fail(ATG_ERR_INVALID, "d_data must be 4-byte aligned");
    *n_entries = 0;
    if (!scan)
        return ATG_OK;
    hipStream_t s = (hipStream_t)stream;
    DeviceContexts<IxCtx>::Held held; // where the data is
    if ((st = g_ctxs.hold(d_data, g_ix_err, held)) != ATG_OK)
        return st;
    IxCtx &c = *held;
    if (!c.have_tables) {
        IxTables t;
        crc_build_tables<8>(0x07u, t.crc8, 1);
        crc_build_tables<16>(0x8005u, &t.crc16[0][0], 4);
        crc_build_advance<16>(t.crc16[0], &t.adv[0][0], 24);
        IHIP(c.tables.ensure(sizeof(IxTables)));
        IHIP(hipMemcpy(c.tables.p, &t, sizeof(IxTables), hipMemcpyHostToDevice));
        c.have_tables = true;
    }
    // the ranges as the kernels see them, and their 64 KB segments
    std::vector<IxRange> rg(n_ranges);
    std::vector<IxSeg> segs;
    uint64_t nbits = 0;
    for (uint32_t i = 0; i < n_ranges; ++i) {
        const atg_flac_index_range &r = ranges[i];
        IxRange &R = rg[i];
        R.start = r.data_offset;
        R.end = r.data_offset + r.data_bytes;
        R.bit0 = nbits;
        R.rate = r.sample_rate;
        R.channels = r.channels;
        R.bps = r.bits_per_sample;
        R.max_bs = r.max_block_size;
        R.fixed_bs = r.min_block_size ? r.min_block_size : r.max_block_size;
        R.bound = frame_bound(r);
        if (r.data_bytes < kMinFrame)
            continue;
        nbits += (r.data_bytes + 63) & ~63ull;
        for (uint64_t c0 = R.start / 16, ce = (R.end + 15) / 16; c0 < ce; c0 += kSegChunks)
            segs.push_back({c0, (uint32_t)std::min<uint64_t>(kSegChunks, ce - c0), i});
    }
    if (segs.size() >= (1ull << 31))
        return g_ix_err.fail(ATG_ERR_UNSUPPORTED, "too many segments in one call");
    const uint64_t nw = (len + 3) / 4;
    const uint32_t *w = (const uint32_t *)d_data;
    IHIP(ensure_events(c.ev));
    IHIP(c.ranges.ensure(sizeof(IxRange) * rg.size()));
    IHIP(c.segs.ensure(sizeof(IxSeg) * segs.size()));
    IHIP(c.bits.ensure(nbits / 8 + 8));
    IHIP(c.counts.ensure(sizeof(IxCounts)));
    // the two small tables go up before anything is enqueued: no copy from
    // these local vectors is in flight on any way out of the function
    IHIP(hipMemcpy(c.ranges.p, rg.data(), sizeof(IxRange) * rg.size(), hipMemcpyHostToDevice));
    IHIP(hipMemcpy(c.segs.p, segs.data(), sizeof(IxSeg) * segs.size(), hipMemcpyHostToDevice));
    // a sync pattern per 32 KB of noise, a frame per few KB of music: room
    // for a hit and a candidate per 64 bytes, and one more run when a stream
    // of tiny frames passes that
    uint64_t hcap = scan / 64 + 4096, ccap = hcap;
    IxCounts got = {};
    for (int run = 0; run < 2; ++run) {
        if (hcap >= (1ull << 32) || ccap >= (1ull << 32))
            return g_ix_err.fail(ATG_ERR_UNSUPPORTED, "too many frame starts in one call");
        IHIP(c.hits.ensure(sizeof(IxHit) * hcap));
        IHIP(c.cands.ensure(sizeof(IxCand) * ccap));
        IHIP(c.entries.ensure(sizeof(IxCand) * ccap));
        IHIP(hipMemsetAsync(c.counts.p, 0, sizeof(IxCounts), s));
        IHIP(hipMemsetAsync(c.bits.p, 0, nbits / 8 + 8, s));
        IHIP(hipEventRecord(c.ev[0], s));
        hipLaunchKernelGGL(k_ix_sync, dim3(grid_for(segs.size(), 1)), dim3(kBlock), 0, s, w, nw,
                           (const IxRange *)c.ranges.p, (const IxSeg *)c.segs.p,
                           (uint32_t)segs.size(), (IxCounts *)c.counts.p, (uint32_t)hcap,
                           (IxHit *)c.hits.p);
        IHIP(hipEventRecord(c.ev[1], s));
        hipLaunchKernelGGL(k_ix_header, dim3(grid_for(hcap, kBlock)), dim3(kBlock), 0, s, w, nw,
                           (const IxRange *)c.ranges.p, (const IxTables *)c.tables.p,
                           (IxCounts *)c.counts.p, (uint32_t)hcap, (const IxHit *)c.hits.p,
                           (uint32_t)ccap, (IxCand *)c.cands.p, (unsigned long long *)c.bits.p);
        IHIP(hipEventRecord(c.ev[2], s));
        hipLaunchKernelGGL(k_ix_confirm, dim3(grid_for(ccap, 4)), dim3(kBlock), 0, s, w, nw,
                           (const IxRange *)c.ranges.p, (const IxTables *)c.tables.p,
                           (IxCounts *)c.counts.p, (uint32_t)ccap, (const IxCand *)c.cands.p,
                           (const unsigned long long *)c.bits.p, (IxCand *)c.entries.p);
        IHIP(hipGetLastError());
        IHIP(hipEventRecord(c.ev[3], s));
        IHIP(hipStreamSynchronize(s));
        IHIP(hipMemcpy(&got, c.counts.p, sizeof(IxCounts), hipMemcpyDeviceToHost));
        if (got.hits <= hcap && got.cands <= ccap)
            break;
        if (run == 1)
            return g_ix_err.fail(ATG_ERR_DEVICE, "the lists overflowed twice");
        // the header pass saw the listed hits only: where those overflowed,
        // its count is short, and the hits bound the candidates
        ccap = std::max<uint64_t>(ccap, got.hits > hcap ? got.hits : got.cands);
        hcap = std::max<uint64_t>(hcap, got.hits);
    }
    StageTimes<kStages> tm;
    for (int k = 0; k < kStages; ++k)
        if (hipEventElapsedTime(&tm.ms[k], c.ev[k], c.ev[k + 1]) != hipSuccess)
            tm.ms[k] = -1.f;
    tm.n = kStages;
    g_ix_times = tm;
    *n_entries = got.entries;
    if (got.entries > entry_cap)
        return g_ix_err.fail(ATG_ERR_CAPACITY, "entry_cap is below the " +
                                                   std::to_string(got.entries) + " entries found");
    std::vector<IxCand> found(got.entries);
    if (got.entries)
        IHIP(hipMemcpy(found.data(), c.entries.p, sizeof(IxCand) * got.entries,
                       hipMemcpyDeviceToHost));
    std::sort(found.begin(), found.end(), [](const IxCand &a, const IxCand &b) {
        return a.range != b.range ? a.range < b.range : a.pos < b.pos;
    });
    for (uint32_t i = 0; i < got.entries; ++i) {
        const IxCand &e = found[i];
        entries[i].byte_offset = e.pos - rg[e.range].start;
        entries[i].first_sample = e.number;
        entries[i].block_size = e.bs;
        entries[i].range = e.range;
    }
    return ATG_OK;
}

atg_status atg_flac_index_host(int device, const uint8_t *data, uint64_t len,
                               const atg_flac_index_range *ranges, uint32_t n_ranges,
                               atg_flac_index_entry *entries, uint64_t entry_cap,
                               uint64_t *n_entries)
{
    uint64_t scan = 0;
    atg_status st = check_args(data, len, ranges, n_ranges, entries, entry_cap, n_entries, &scan);
    if (st != ATG_OK)
        return st;
    *n_entries = 0;
    if (!scan)
        return ATG_OK;
    if ((st = use_device(device, g_ix_err)) != ATG_OK)
        return st;
    // the span the ranges cover, from a 16-byte boundary, ranges rebased to it
    uint64_t lo = len, hi = 0;
    for (uint32_t i = 0; i < n_ranges; ++i)
        if (ranges[i].data_bytes >= kMinFrame) {
            lo = std::min(lo, ranges[i].data_offset);
            hi = std::max(hi, ranges[i].data_offset + ranges[i].data_bytes);
        }
    lo &= ~15ull;
    std::vector<atg_flac_index_range> moved(ranges, ranges + n_ranges);
    for (atg_flac_index_range &r : moved)
        r.data_offset = r.data_bytes >= kMinFrame ? r.data_offset - lo : 0;
    DevTemp d;
    ATG_HIP_TRY(g_ix_err, d.alloc(hi - lo + 16), "hipMalloc(&d, hi - lo + 16)");
    ATG_HIP_TRY(g_ix_err, hipMemcpy(d.p, data + lo, hi - lo, hipMemcpyHostToDevice), "hipMemcpy");
    return atg_flac_index_device(d.p, hi - lo, moved.data(), n_ranges, entries, entry_cap,
                                 n_entries, nullptr);
}

int atg_flac_index_kernel_times(const char **names, float *ms, int cap)
{
    return copy_times(kStageNames, g_ix_times.ms, g_ix_times.n, names, ms, cap);
}

} // extern "C"
