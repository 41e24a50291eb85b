// mlp_decode.hip — MLP titles of DVD-Audio discs on the device (the
// reference's src/decoders/mlp.c and the MLP branches of aob.c), batched over
// a ragged table of titles.  The arithmetic lives in mlp_common.h; the passes:
//   sectors  the AOB sector pass (aob_passes.h), a lane per sector.
//   layout   a workgroup per title: first bad sector, payload prefix sum
//            (aob_layout_title), the major sync at byte 4 of the first payload.
//   gather   the title's payload stream contiguous in scratch, a lane per
//            aligned 16-byte unit of it.
//   walk     a wave per title chases the 4-byte unit headers through a 4 KiB
//            LDS window of the stream (one global round trip per window, not
//            per hop), then a lane per unit fills its record.  Run twice:
//            counting, then storing into a table the host sized.
//   check    a lane per (unit, substream): parity and CRC-8.
//   parse    a lane per (unit, substream) that opens with a restart header
//            (or is the title's first) parses on to the next such unit: the
//            restart header re-establishes the whole parser state.  Sizing:
//            frames, blocks and status per (unit, substream).
//   resolve  a wave per title: the first failing unit by the reference's
//            order of checks, the units delivered (those ending in a sector
//            before the one the failing unit ends in), prefix sums of their
//            frames and blocks.  The host reads the table once here: this is
//            the round trip that sizes the output.
//   store    the parse again over the delivered units: residuals channel
//            planar, a record per block (filters, shift, quantiser step, IIR
//            state when stated) and per unit (matrices, output shifts, steps
//            as they stand at its end, noise seed, frames).
//   filter   FIR + IIR recursion.  The FIR state is never reset, so the chain
//            is serial per (title, channel) across the whole title: a wave
//            per title, a lane per channel, residuals staged through LDS in
//            tiles of kMlpTile frames.  This pass bounds the decode of long
//            titles: its time is title frames * one dependent step.
//   output   a lane per frame: noise, matrices in order, LSB bypass, output
//            shift, WAVE channel order, interleaved store.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/atgpu.h"
#include "aob_common.h"
#include "aob_passes.h"
#include "host_common.h"
#include "mlp_common.h"
#include "table_search.h"
#include "wave.h"

namespace {

thread_local ErrSlot g_mlp_err;
#define MHIP(expr) ATG_HIP_TRY(g_mlp_err, expr, #expr)

constexpr uint32_t kMaxBlocks = 4096;
constexpr int kStages = 10;
const char *const kStageNames[kStages] = {"sectors", "layout", "gather", "walk",   "check",
                                          "parse",   "resolve", "store", "filter", "output"};
thread_local StageTimes<kStages> g_mlp_times;

constexpr uint32_t kMlpWindow = 4096; // bytes of stream per LDS window of the walk
constexpr uint32_t kMlpTile = 256;    // frames per LDS tile of the filter pass

// a title on the device; who fills what: (h) host, (l) layout, (w) walk,
// (r) resolve
struct MlpTitle {
    uint64_t byte_offset;       // h
    uint32_t n_sectors, sec0;   // h
    uint32_t n_valid, status;   // l: first bad sector; ATG_MLP_OK = decode on
    uint64_t stream_bytes;      // l
    uint32_t sample_rate, bits, channels, mask, assignment; // l
    uint32_t nss;               // w (store): substreams of the first major sync
    uint32_t n_units, walk_status, walk_sector; // w
    uint32_t range0[2];         // w (store): lo | hi << 8 | mmc << 16 of unit 0's restart headers
    uint32_t unit0;             // h, after the counting walk
    uint32_t stop_unit, stop_sector, n_good, final_status; // r
    uint64_t good_frames;       // r
    uint64_t blocks[2];         // r
    uint64_t frame0, blk0[2], sample_offset; // h, after resolve
};

__constant__ MlpCrc c_crc = mlp_crc_table();

__global__ __launch_bounds__(kAobBlock) void k_mlp_layout(const uint8_t *__restrict__ bytes,
                                                          const AobTitle *__restrict__ at,
                                                          const atg_aob_sector *__restrict__ sectors,
                                                          AobPrefix *__restrict__ prefix,
                                                          MlpTitle *__restrict__ mt)
{
    const AobTitle t = at[blockIdx.x];
    const atg_aob_sector *sec = sectors + t.sec0;
    uint32_t bad;
    uint64_t total;
    aob_layout_title(t, sec, prefix + t.sec0, &bad, &total);
    if (threadIdx.x)
        return;
    MlpTitle &m = mt[blockIdx.x];
    m.n_valid = bad;
    m.stream_bytes = total;
    m.sample_rate = m.bits = m.channels = m.mask = m.assignment = 0;
    if (t.n_sectors == 0) {
        m.status = ATG_MLP_EOF;
    } else if (bad == 0) {
        m.status = ATG_MLP_BAD_SECTOR;
    } else if (sec[0].codec_id != 0xA1) {
        m.status = ATG_MLP_NOT_MLP;
    } else {
        // aob.c reads the attributes from the first packet alone: 18 bytes
        const uint8_t *p = bytes + t.byte_offset + sec[0].payload_offset;
        if (sec[0].payload_length < 18 || p[4] != 0xF8 || p[5] != 0x72 || p[6] != 0x6F ||
            p[7] != 0xBB) {
            m.status = ATG_MLP_NO_MAJOR_SYNC;
        } else {
            const uint32_t ca = p[11] & 31u;
            m.assignment = ca;
            m.bits = aob_bits(p[8] >> 4);
            m.sample_rate = aob_rate(p[9] >> 4);
            m.channels = aob_channels(ca);
            m.mask = aob_channel_mask(ca);
            m.status = ((m.bits != 16 && m.bits != 24) || !m.sample_rate || !m.channels)
                           ? ATG_MLP_UNSUPPORTED
                           : ATG_MLP_OK;
        }
    }
    if (m.status != ATG_MLP_OK)
        m.stream_bytes = 0;
}

// a lane per aligned 16-byte unit of the scratch stream; a title's stream
// starts at byte sec0 * 2048 of it
__global__ __launch_bounds__(kAobBlock) void k_mlp_gather(const uint8_t *__restrict__ bytes,
                                                          const atg_aob_sector *__restrict__ sectors,
                                                          const AobPrefix *__restrict__ prefix,
                                                          const MlpTitle *__restrict__ mt,
                                                          uint32_t n_titles, uint64_t n_units16,
                                                          uint8_t *__restrict__ stream)
{
    for (uint64_t g = (uint64_t)blockIdx.x * kAobBlock + threadIdx.x; g < n_units16;
         g += (uint64_t)gridDim.x * kAobBlock) {
        const MlpTitle &t = mt[last_le(mt, n_titles, (uint32_t)(g / kAobUnits), &MlpTitle::sec0)];
        const uint64_t pos = (g - (uint64_t)t.sec0 * kAobUnits) * 16;
        if (pos >= t.stream_bytes)
            continue;
        const AobPrefix *pre = prefix + t.sec0;
        const atg_aob_sector *sec = sectors + t.sec0;
        uint32_t s = last_le(pre, t.n_valid, pos, &AobPrefix::start);
        uint32_t w[4] = {0, 0, 0, 0};
        for (uint32_t k = 0; k < 16 && pos + k < t.stream_bytes; ++k) {
            while (pos + k >= pre[s].start + sec[s].payload_length)
                ++s; // ends before n_valid: pos + k is below the stream's length
            const uint8_t b = bytes[t.byte_offset + (uint64_t)s * kAobSector +
                                    sec[s].payload_offset + (uint32_t)(pos + k - pre[s].start)];
            w[k >> 2] |= (uint32_t)b << (8 * (k & 3));
        }
        *reinterpret_cast<uint4 *>(stream + (uint64_t)t.sec0 * kAobSector + pos) =
            make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// A wave per title.  STORE == false counts the whole units; true writes their
// records into units[unit0 ...].
template <bool STORE>
__global__ __launch_bounds__(64) void k_mlp_walk(const uint8_t *__restrict__ stream,
                                                 const AobPrefix *__restrict__ prefix,
                                                 MlpTitle *__restrict__ mt,
                                                 atg_mlp_unit *__restrict__ units)
{
    __shared__ uint4 s_win4[kMlpWindow / 16];
    const uint8_t *win = reinterpret_cast<const uint8_t *>(s_win4);
    MlpTitle &t = mt[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    if (t.status != ATG_MLP_OK) {
        if (lane == 0) {
            t.n_units = 0;
            t.walk_status = ATG_MLP_OK;
            t.walk_sector = 0;
            t.nss = 0;
        }
        return;
    }
    const uint8_t *s = stream + (uint64_t)t.sec0 * kAobSector;
    const AobPrefix *pre = prefix + t.sec0;
    const uint64_t n = t.stream_bytes, n16 = (n + 15) & ~15ull;
    atg_mlp_unit *out = STORE ? units + t.unit0 : nullptr;
    uint64_t pos = 0, w0 = ~0ull;
    uint32_t count = 0, wstatus = ATG_MLP_OK, wsector = 0;
    while (n - pos >= 4) {
        if (w0 == ~0ull || pos < w0 || pos + 2 > w0 + kMlpWindow) {
            __syncthreads(); // every lane has read the old window
            w0 = pos & ~15ull;
            for (uint32_t i = lane; i < kMlpWindow / 16; i += 64)
                if (w0 + 16ull * i < n16)
                    s_win4[i] = *reinterpret_cast<const uint4 *>(s + w0 + 16ull * i);
            __syncthreads();
        }
        const uint32_t words = ((uint32_t)(win[pos - w0] & 15) << 8) | win[pos - w0 + 1];
        if (words < 2) {
            wstatus = ATG_MLP_UNSUPPORTED;
            wsector = last_le(pre, t.n_valid, pos + 3, &AobPrefix::start);
            break;
        }
        const uint32_t size = 2 * words;
        if (n - pos < size)
            break;
        if (STORE && lane == 0) {
            out[count].offset = pos;
            out[count].size = (uint16_t)size;
        }
        ++count;
        pos += size;
    }
    if (!STORE) {
        if (lane == 0) {
            t.n_units = count;
            t.walk_status = wstatus;
            t.walk_sector = wsector;
        }
        return;
    }
    __syncthreads(); // lane 0's offsets and sizes
    // the first unit's major sync is the title's
    uint8_t key0[4] = {0, 0, 0, 0};
    bool have0 = false;
    if (count) {
        have0 = out[0].size >= 32 && s[4] == 0xF8 && s[5] == 0x72 && s[6] == 0x6F && s[7] == 0xBB;
        if (have0) {
            key0[0] = s[8];
            key0[1] = s[9];
            key0[2] = s[11] & 31;
            key0[3] = s[20] >> 4;
        }
    }
    for (uint32_t u = lane; u < count; u += 64) {
        atg_mlp_unit *r = out + u;
        r->end_sector = last_le(pre, t.n_valid, r->offset + r->size - 1, &AobPrefix::start);
        mlp_fill_unit(s, u == 0, have0, key0, r);
    }
    __syncthreads();
    if (lane == 0) {
        t.nss = have0 && (key0[3] == 1 || key0[3] == 2) ? key0[3] : 0;
        t.range0[0] = t.range0[1] = 0xFFFFFFFFu;
        for (uint32_t k = 0; count && k < t.nss; ++k) {
            uint32_t start, len;
            if (out[0].status == ATG_MLP_OK && (out[0].substream_flags[k] & 4) &&
                mlp_substream_range(out, k, &start, &len) && len >= 6) {
                const uint8_t *d = s + start;
                t.range0[k] = (uint32_t)(d[4] >> 4) | (uint32_t)(d[4] & 15) << 8 |
                              (uint32_t)(d[5] >> 4) << 16;
            }
        }
    }
}

// a lane per (unit, substream) of the batch
__global__ __launch_bounds__(kAobBlock) void k_mlp_check(const uint8_t *__restrict__ stream,
                                                         const MlpTitle *__restrict__ mt,
                                                         uint32_t n_titles,
                                                         const atg_mlp_unit *__restrict__ units,
                                                         uint32_t n_units, uint8_t *__restrict__ chk)
{
    const uint32_t id = blockIdx.x * kAobBlock + threadIdx.x;
    if (id >= 2 * n_units)
        return;
    const uint32_t g = id >> 1, k = id & 1;
    const MlpTitle &t = mt[last_le(mt, n_titles, g, &MlpTitle::unit0)];
    const atg_mlp_unit &u = units[g];
    uint32_t st = ATG_MLP_OK, start, len;
    if (k < t.nss && u.status == ATG_MLP_OK) {
        if (!mlp_substream_range(&u, k, &start, &len))
            st = ATG_MLP_IO_ERROR;
        else if (u.substream_flags[0] & 2)
            st = mlp_check_data(stream + (uint64_t)t.sec0 * kAobSector + u.offset + start, len,
                                c_crc.t);
    }
    chk[id] = (uint8_t)st;
}

// A lane per (unit, substream); the lanes of units that open a restart
// segment parse on to the segment's end.
template <bool STORE>
__global__ __launch_bounds__(64) void k_mlp_parse(
    const uint8_t *__restrict__ stream, const MlpTitle *__restrict__ mt, uint32_t n_titles,
    const atg_mlp_unit *__restrict__ units, uint32_t n_units, const uint8_t *__restrict__ chk,
    MlpSize *__restrict__ sizes, const uint64_t *__restrict__ uframe0,
    const uint64_t *__restrict__ ublk0, int32_t *__restrict__ res, uint8_t *__restrict__ byp,
    uint64_t stride, MlpBlockRec *__restrict__ blocks, MlpUnitRec *__restrict__ urec)
{
    const uint32_t id = blockIdx.x * 64 + threadIdx.x;
    if (id >= 2 * n_units)
        return;
    const uint32_t g0 = id >> 1, k = id & 1;
    const MlpTitle &t = mt[last_le(mt, n_titles, g0, &MlpTitle::unit0)];
    const uint32_t u0 = g0 - t.unit0, limit = STORE ? t.n_good : t.n_units;
    if (k >= t.nss || u0 >= limit || (u0 && !(units[g0].substream_flags[k] & 4)))
        return;
    const uint8_t *s = stream + (uint64_t)t.sec0 * kAobSector;
    const MlpWho who = {k, t.nss, t.channels, t.range0[k]};
    const bool last = k == t.nss - 1;
    MlpState st = {};
    for (uint32_t v = u0; v < limit; ++v) {
        const uint32_t g = t.unit0 + v;
        const atg_mlp_unit &u = units[g];
        if (v != u0 && (u.substream_flags[k] & 4))
            break; // the next segment's
        uint32_t start, len;
        if (u.status != ATG_MLP_OK || chk[2 * g + k] != ATG_MLP_OK ||
            !mlp_substream_range(&u, k, &start, &len))
            break;
        uint32_t frames = 0, nb = 0;
        int r;
        if (STORE) {
            MlpStoreSink sink = {res, last ? byp : nullptr, stride, t.frame0 + uframe0[g],
                                 blocks + t.blk0[k] + ublk0[2 * g + k]};
            r = mlp_read_substream(s + u.offset + start, len, st, who, sink, &frames, &nb);
        } else {
            MlpSizeSink sink;
            r = mlp_read_substream(s + u.offset + start, len, st, who, sink, &frames, &nb);
            MlpSize z = {(uint16_t)frames, (uint16_t)nb, (uint8_t)r, st.lo, st.hi, st.mmc};
            sizes[2 * g + k] = z;
        }
        if (r != ATG_MLP_OK)
            break;
        if (last) {
            // the reference rematrixes once per unit with the seed its restart
            // headers left, and the noise of the unit's frames advances it
            if (STORE)
                mlp_unit_record(st, st.seed, frames, urec + g);
            for (uint32_t i = 0; i < frames; ++i)
                st.seed = mlp_next_seed(st.seed);
        }
    }
}

// the status of unit g by the reference's order of checks
__device__ uint32_t mlp_unit_status(const MlpTitle &t, const atg_mlp_unit *units,
                                    const uint8_t *chk, const MlpSize *sizes, uint32_t g)
{
    if (units[g].status)
        return units[g].status;
    for (uint32_t k = 0; k < t.nss; ++k) {
        if (chk[2 * g + k])
            return chk[2 * g + k];
        if (sizes[2 * g + k].status)
            return sizes[2 * g + k].status;
    }
    if (t.nss == 2) {
        const MlpSize &a = sizes[2 * g], &b = sizes[2 * g + 1];
        if (a.frames != b.frames || b.lo != a.hi + 1u)
            return ATG_MLP_UNSUPPORTED;
    }
    return ATG_MLP_OK;
}

__global__ __launch_bounds__(64) void k_mlp_resolve(MlpTitle *__restrict__ mt,
                                                    const atg_mlp_unit *__restrict__ units,
                                                    const uint8_t *__restrict__ chk,
                                                    const MlpSize *__restrict__ sizes,
                                                    uint64_t *__restrict__ uframe0,
                                                    uint64_t *__restrict__ ublk0)
{
    MlpTitle &t = mt[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    if (t.status != ATG_MLP_OK) {
        if (lane == 0) {
            t.final_status = t.status;
            t.stop_unit = t.stop_sector = t.n_good = 0;
            t.good_frames = t.blocks[0] = t.blocks[1] = 0;
        }
        return;
    }
    const uint32_t n = t.n_units;
    uint32_t f = n;
    for (uint32_t u = lane; u < n; u += 64)
        if (mlp_unit_status(t, units, chk, sizes, t.unit0 + u)) {
            f = u;
            break;
        }
    f = wave_min_u32(f);
    uint32_t status = ATG_MLP_OK, sector = 0;
    if (f < n) {
        status = mlp_unit_status(t, units, chk, sizes, t.unit0 + f);
        sector = units[t.unit0 + f].end_sector;
    } else if (t.walk_status) {
        status = t.walk_status;
        sector = t.walk_sector;
    }
    // delivered: the units before f that end in a sector before `sector`
    uint32_t good = 0;
    for (uint32_t u = lane; u < f; u += 64)
        good += !status || units[t.unit0 + u].end_sector < sector;
    good = wave_sum_u32(good);
    const uint32_t last = t.nss ? t.nss - 1 : 0;
    uint64_t carry[3] = {0, 0, 0};
    for (uint32_t base = 0; base < good; base += 64) {
        const uint32_t u = base + lane, g = t.unit0 + u;
        uint64_t v[3] = {0, 0, 0};
        if (u < good) {
            v[0] = sizes[2 * g + last].frames;
            v[1] = sizes[2 * g].blocks;
            v[2] = t.nss == 2 ? sizes[2 * g + 1].blocks : 0;
        }
        for (int j = 0; j < 3; ++j) {
            const uint64_t incl = wave_incl_scan_u64(v[j], (int)lane);
            const uint64_t excl = carry[j] + incl - v[j];
            carry[j] += readlane_u64(incl, 63);
            v[j] = excl;
        }
        if (u < good) {
            uframe0[g] = v[0];
            ublk0[2 * g] = v[1];
            ublk0[2 * g + 1] = v[2];
        }
    }
    if (lane == 0) {
        t.n_good = good;
        t.good_frames = carry[0];
        t.blocks[0] = carry[1];
        t.blocks[1] = carry[2];
        t.stop_unit = status ? f : n;
        t.stop_sector = status ? sector : t.n_valid;
        t.final_status =
            status ? status : (t.n_valid < t.n_sectors ? ATG_MLP_BAD_SECTOR : ATG_MLP_OK);
    }
}

// A wave per title, a lane per channel: filter_mlp_channel over the whole
// title, in place in the residual planes.
__global__ __launch_bounds__(64) void k_mlp_filter(const MlpTitle *__restrict__ mt,
                                                   const MlpBlockRec *__restrict__ blocks,
                                                   int32_t *__restrict__ res, uint64_t stride)
{
    __shared__ int32_t s_tile[kMlpChannels][kMlpTile + 1];
    const MlpTitle &t = mt[blockIdx.x];
    if (t.final_status > ATG_MLP_UNSUPPORTED || !t.good_frames || !t.nss)
        return;
    const uint32_t lane = threadIdx.x;
    const uint32_t nch = min((t.range0[t.nss - 1] >> 16) + 1u, kMlpChannels);
    const uint32_t hi0 = (t.range0[0] >> 8) & 255u;
    // channel `lane` is channel ci of substream k
    const uint32_t k = (t.nss == 2 && lane > hi0) ? 1 : 0;
    const uint32_t ci = min(k ? lane - hi0 - 1 : lane, kMlpChannels - 1);
    const MlpBlockRec *blk = blocks + t.blk0[k];
    const uint64_t n_blk = t.blocks[k];
    uint64_t bi = 0;
    uint32_t rem = 0;
    MlpChanRec p = {};
    int32_t fir_h[8] = {0, 0, 0, 0, 0, 0, 0, 0}, iir_h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t f0 = 0; f0 < t.good_frames; f0 += kMlpTile) {
        const uint32_t nt = (uint32_t)min((uint64_t)kMlpTile, t.good_frames - f0);
        for (uint32_t c = 0; c < nch; ++c)
            for (uint32_t i = lane; i < nt; i += 64)
                s_tile[c][i] = res[c * stride + t.frame0 + f0 + i];
        __syncthreads();
        if (lane < nch)
            for (uint32_t i = 0; i < nt; ++i) {
                if (!rem) {
                    if (bi >= n_blk)
                        break;
                    p = blk[bi].ch[ci];
                    rem = blk[bi].frames;
                    ++bi;
                    if (p.iir_set)
                        for (int j = 0; j < 8; ++j)
                            iir_h[j] = p.iir_state[j];
                }
                s_tile[lane][i] = mlp_filter_step(p, fir_h, iir_h, s_tile[lane][i]);
                --rem;
            }
        __syncthreads();
        for (uint32_t c = 0; c < nch; ++c)
            for (uint32_t i = lane; i < nt; i += 64)
                res[c * stride + t.frame0 + f0 + i] = s_tile[c][i];
        __syncthreads();
    }
}

// a lane per frame of the batch
template <typename T>
__global__ __launch_bounds__(kAobBlock) void k_mlp_output(
    const MlpTitle *__restrict__ mt, uint32_t n_titles, const uint64_t *__restrict__ uframe0,
    const MlpUnitRec *__restrict__ urec, const int32_t *__restrict__ res,
    const uint8_t *__restrict__ byp, uint64_t stride, T *__restrict__ out)
{
    for (uint64_t F = (uint64_t)blockIdx.x * kAobBlock + threadIdx.x; F < stride;
         F += (uint64_t)gridDim.x * kAobBlock) {
        const MlpTitle &t = mt[last_le(mt, n_titles, F, &MlpTitle::frame0)];
        const uint64_t f = F - t.frame0;
        if (f >= t.good_frames)
            continue;
        // the last delivered unit whose first frame is at or below f
        const uint64_t *uf = uframe0 + t.unit0;
        uint32_t lo = 0, hi = t.n_good;
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (uf[mid] <= f)
                lo = mid;
            else
                hi = mid;
        }
        const MlpUnitRec &u = urec[t.unit0 + lo];
        int32_t ch[kMlpChannels];
#pragma unroll
        for (uint32_t c = 0; c < kMlpChannels; ++c)
            ch[c] = c <= u.mmc ? res[c * stride + F] : 0;
        mlp_rematrix_frame(u, (uint32_t)(f - uf[lo]), byp[F], ch);
        T *dst = out + t.sample_offset + f * t.channels;
        const uint32_t sh = 32 - t.bits;
#pragma unroll
        for (uint32_t c = 0; c < kMlpChannels; ++c)
            if (c < t.channels)
                dst[mlp_wave_channel(t.assignment, c)] =
                    (T)((int32_t)((uint32_t)ch[c] << sh) >> sh);
    }
}

// per device: the tables and the events that time the passes
struct MlpCtx {
    DevBuf at, mt, sectors, prefix, stream, units, chk, sizes, uframe0, ublk0, urec, res, byp,
        blocks;
    hipEvent_t ev[14] = {};
};
DeviceContexts<MlpCtx> g_ctxs;

uint32_t grid_for(uint64_t items, uint32_t block)
{
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + block - 1) / block, 1),
                                        0x7FFFFFFFull);
}

// Every pass, on a held context.  d_pcm == NULL: stop after resolve (the
// scan).  units (host, may be NULL) receives the unit table.
atg_status run_locked(MlpCtx &c, const void *d_bytes, const atg_aob_title *titles, uint32_t n,
                      uint64_t n_sectors, int format, atg_mlp_result *results,
                      uint64_t *total_samples, atg_mlp_unit *units, uint64_t units_cap,
                      bool decode, void *d_pcm, uint64_t pcm_cap, hipStream_t s)
{
    ATG_HIP_TRY(g_mlp_err, ensure_events(c.ev), "hipEventCreate(&e)");
    std::vector<AobTitle> at(n);
    std::vector<MlpTitle> mt(n);
    uint32_t sec0 = 0;
    for (uint32_t i = 0; i < n; ++i) {
        at[i] = {titles[i].byte_offset, titles[i].n_sectors, sec0};
        mt[i] = MlpTitle{};
        mt[i].byte_offset = titles[i].byte_offset;
        mt[i].n_sectors = titles[i].n_sectors;
        mt[i].sec0 = sec0;
        sec0 += titles[i].n_sectors;
    }
    MHIP(c.at.ensure(sizeof(AobTitle) * n));
    MHIP(c.mt.ensure(sizeof(MlpTitle) * n));
    MHIP(c.sectors.ensure(sizeof(atg_aob_sector) * n_sectors));
    MHIP(c.prefix.ensure(sizeof(AobPrefix) * n_sectors));
    MHIP(c.stream.ensure((size_t)kAobSector * n_sectors));
    MHIP(hipMemcpyAsync(c.at.p, at.data(), sizeof(AobTitle) * n, hipMemcpyHostToDevice, s));
    MHIP(hipMemcpyAsync(c.mt.p, mt.data(), sizeof(MlpTitle) * n, hipMemcpyHostToDevice, s));
    const uint8_t *bytes = (const uint8_t *)d_bytes;
    const AobTitle *d_at = (const AobTitle *)c.at.p;
    MlpTitle *d_mt = (MlpTitle *)c.mt.p;
    atg_aob_sector *d_sec = (atg_aob_sector *)c.sectors.p;
    AobPrefix *d_pre = (AobPrefix *)c.prefix.p;
    uint8_t *d_stream = (uint8_t *)c.stream.p;

    MHIP(hipEventRecord(c.ev[0], s));
    if (n_sectors)
        hipLaunchKernelGGL(k_aob_sectors,
                           dim3(std::min(grid_for(n_sectors, kAobBlock), kMaxBlocks)),
                           dim3(kAobBlock), 0, s, bytes, d_at, n, (uint32_t)n_sectors, d_sec);
    MHIP(hipEventRecord(c.ev[1], s));
    hipLaunchKernelGGL(k_mlp_layout, dim3(n), dim3(kAobBlock), 0, s, bytes, d_at,
                       (const atg_aob_sector *)d_sec, d_pre, d_mt);
    MHIP(hipEventRecord(c.ev[2], s));
    if (n_sectors)
        hipLaunchKernelGGL(k_mlp_gather,
                           dim3(std::min(grid_for(n_sectors * kAobUnits, kAobBlock), kMaxBlocks)),
                           dim3(kAobBlock), 0, s, bytes, (const atg_aob_sector *)d_sec,
                           (const AobPrefix *)d_pre, (const MlpTitle *)d_mt, n,
                           n_sectors * kAobUnits, d_stream);
    MHIP(hipEventRecord(c.ev[3], s));
    hipLaunchKernelGGL(k_mlp_walk<false>, dim3(n), dim3(64), 0, s, (const uint8_t *)d_stream,
                       (const AobPrefix *)d_pre, d_mt, (atg_mlp_unit *)nullptr);
    MHIP(hipGetLastError());
    MHIP(hipEventRecord(c.ev[4], s));
    MHIP(hipMemcpyAsync(mt.data(), d_mt, sizeof(MlpTitle) * n, hipMemcpyDeviceToHost, s));
    MHIP(hipStreamSynchronize(s));

    // the unit table, sized by the counting walk
    uint64_t n_units = 0;
    for (uint32_t i = 0; i < n; ++i) {
        mt[i].unit0 = (uint32_t)n_units;
        n_units += mt[i].n_units;
    }
    if (n_units > 0x3FFFFFFFull)
        return g_mlp_err.fail(ATG_ERR_UNSUPPORTED, "more than 2^30 - 1 access units in one batch");
    MHIP(c.units.ensure(sizeof(atg_mlp_unit) * n_units));
    MHIP(c.chk.ensure(2 * n_units));
    MHIP(c.sizes.ensure(sizeof(MlpSize) * 2 * n_units));
    MHIP(c.uframe0.ensure(sizeof(uint64_t) * n_units));
    MHIP(c.ublk0.ensure(sizeof(uint64_t) * 2 * n_units));
    MHIP(hipMemcpyAsync(d_mt, mt.data(), sizeof(MlpTitle) * n, hipMemcpyHostToDevice, s));
    MHIP(hipMemsetAsync(c.sizes.p, kMlpNotReached, std::max<size_t>(sizeof(MlpSize) * 2 * n_units, 1),
                        s));
    atg_mlp_unit *d_units = (atg_mlp_unit *)c.units.p;
    uint8_t *d_chk = (uint8_t *)c.chk.p;
    MlpSize *d_sizes = (MlpSize *)c.sizes.p;
    uint64_t *d_uframe0 = (uint64_t *)c.uframe0.p, *d_ublk0 = (uint64_t *)c.ublk0.p;
    const uint32_t nu = (uint32_t)n_units;
    MHIP(hipEventRecord(c.ev[5], s));
    hipLaunchKernelGGL(k_mlp_walk<true>, dim3(n), dim3(64), 0, s, (const uint8_t *)d_stream,
                       (const AobPrefix *)d_pre, d_mt, d_units);
    MHIP(hipEventRecord(c.ev[6], s));
    if (nu)
        hipLaunchKernelGGL(k_mlp_check, dim3(grid_for(2ull * nu, kAobBlock)), dim3(kAobBlock), 0, s,
                           (const uint8_t *)d_stream, (const MlpTitle *)d_mt, n,
                           (const atg_mlp_unit *)d_units, nu, d_chk);
    MHIP(hipEventRecord(c.ev[7], s));
    if (nu)
        hipLaunchKernelGGL(k_mlp_parse<false>, dim3(grid_for(2ull * nu, 64)), dim3(64), 0, s,
                           (const uint8_t *)d_stream, (const MlpTitle *)d_mt, n,
                           (const atg_mlp_unit *)d_units, nu, (const uint8_t *)d_chk, d_sizes,
                           (const uint64_t *)nullptr, (const uint64_t *)nullptr,
                           (int32_t *)nullptr, (uint8_t *)nullptr, 0ull, (MlpBlockRec *)nullptr,
                           (MlpUnitRec *)nullptr);
    MHIP(hipEventRecord(c.ev[8], s));
    hipLaunchKernelGGL(k_mlp_resolve, dim3(n), dim3(64), 0, s, d_mt,
                       (const atg_mlp_unit *)d_units, (const uint8_t *)d_chk,
                       (const MlpSize *)d_sizes, d_uframe0, d_ublk0);
    MHIP(hipGetLastError());
    MHIP(hipEventRecord(c.ev[9], s));
    MHIP(hipMemcpyAsync(mt.data(), d_mt, sizeof(MlpTitle) * n, hipMemcpyDeviceToHost, s));
    MHIP(hipStreamSynchronize(s));

    // the one round trip that sizes the output
    const uint64_t group = format == ATG_PCM_S16 ? 8 : 4;
    uint64_t samples = 0, frames = 0, blk[2] = {0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        MlpTitle &t = mt[i];
        atg_mlp_result &r = results[i];
        r = atg_mlp_result{};
        r.status = (int32_t)t.final_status;
        r.stop_sector = t.stop_sector;
        r.stop_unit = t.stop_unit;
        r.access_units = t.n_units;
        r.sample_rate = t.sample_rate;
        r.bits_per_sample = t.bits;
        r.channels = t.channels;
        r.channel_mask = t.mask;
        r.channel_assignment = t.assignment;
        r.substreams = t.nss;
        r.good_frames = t.good_frames;
        r.sample_offset = t.sample_offset = samples;
        samples += (t.good_frames * t.channels + group - 1) / group * group;
        t.frame0 = frames;
        frames += t.good_frames;
        for (int k = 0; k < 2; ++k) {
            t.blk0[k] = blk[k];
            blk[k] += t.blocks[k];
        }
    }
    // substream 1's block records follow substream 0's
    for (uint32_t i = 0; i < n; ++i)
        mt[i].blk0[1] += blk[0];
    if (total_samples)
        *total_samples = samples;
    auto times = [&](int upto) {
        const int pairs[kStages][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4},  {6, 7},
                                       {7, 8}, {8, 9}, {10, 11}, {11, 12}, {12, 13}};
        for (int k = 0; k < kStages; ++k) {
            float &ms = g_mlp_times.ms[k] = 0.f;
            if (k < upto)
                (void)hipEventElapsedTime(&ms, c.ev[pairs[k][0]], c.ev[pairs[k][1]]);
        }
        float again = 0.f; // the storing walk
        if (hipEventElapsedTime(&again, c.ev[5], c.ev[6]) == hipSuccess)
            g_mlp_times.ms[3] += again;
        g_mlp_times.n = upto;
    };
    times(7);
    if (units) {
        if (units_cap < n_units)
            return g_mlp_err.fail(ATG_ERR_CAPACITY, "units_cap is below the batch's access units");
        if (n_units)
            MHIP(hipMemcpy(units, d_units, sizeof(atg_mlp_unit) * n_units, hipMemcpyDeviceToHost));
    }
    if (!decode)
        return ATG_OK;
    if (samples > pcm_cap)
        return g_mlp_err.fail(ATG_ERR_CAPACITY, "pcm_cap_samples is below the batch's samples");
    for (uint32_t i = 0; i < n; ++i)
        if (format == ATG_PCM_S16 && mt[i].good_frames && mt[i].bits != 16)
            return g_mlp_err.fail(ATG_ERR_INVALID, "ATG_PCM_S16 cannot hold a 24-bit title");
    if (!frames)
        return ATG_OK;
    MHIP(c.urec.ensure(sizeof(MlpUnitRec) * n_units));
    MHIP(c.res.ensure(sizeof(int32_t) * kMlpChannels * frames));
    MHIP(c.byp.ensure(frames));
    MHIP(c.blocks.ensure(sizeof(MlpBlockRec) * (blk[0] + blk[1])));
    MHIP(hipMemcpyAsync(d_mt, mt.data(), sizeof(MlpTitle) * n, hipMemcpyHostToDevice, s));
    int32_t *d_res = (int32_t *)c.res.p;
    uint8_t *d_byp = (uint8_t *)c.byp.p;
    MlpBlockRec *d_blocks = (MlpBlockRec *)c.blocks.p;
    MlpUnitRec *d_urec = (MlpUnitRec *)c.urec.p;
    MHIP(hipEventRecord(c.ev[10], s));
    hipLaunchKernelGGL(k_mlp_parse<true>, dim3(grid_for(2ull * nu, 64)), dim3(64), 0, s,
                       (const uint8_t *)d_stream, (const MlpTitle *)d_mt, n,
                       (const atg_mlp_unit *)d_units, nu, (const uint8_t *)d_chk, d_sizes,
                       (const uint64_t *)d_uframe0, (const uint64_t *)d_ublk0, d_res, d_byp,
                       frames, d_blocks, d_urec);
    MHIP(hipEventRecord(c.ev[11], s));
    hipLaunchKernelGGL(k_mlp_filter, dim3(n), dim3(64), 0, s, (const MlpTitle *)d_mt,
                       (const MlpBlockRec *)d_blocks, d_res, frames);
    MHIP(hipEventRecord(c.ev[12], s));
    const dim3 grid(std::min(grid_for(frames, kAobBlock), kMaxBlocks)), block(kAobBlock);
    if (format == ATG_PCM_S16)
        hipLaunchKernelGGL(k_mlp_output<int16_t>, grid, block, 0, s, (const MlpTitle *)d_mt, n,
                           (const uint64_t *)d_uframe0, (const MlpUnitRec *)d_urec,
                           (const int32_t *)d_res, (const uint8_t *)d_byp, frames,
                           (int16_t *)d_pcm);
    else
        hipLaunchKernelGGL(k_mlp_output<int32_t>, grid, block, 0, s, (const MlpTitle *)d_mt, n,
                           (const uint64_t *)d_uframe0, (const MlpUnitRec *)d_urec,
                           (const int32_t *)d_res, (const uint8_t *)d_byp, frames,
                           (int32_t *)d_pcm);
    MHIP(hipGetLastError());
    MHIP(hipEventRecord(c.ev[13], s));
    MHIP(hipStreamSynchronize(s));
    times(kStages);
    return ATG_OK;
}

} // namespace

extern "C" {

const char *atg_mlp_last_error(void) { return g_mlp_err.msg.c_str(); }

int atg_mlp_kernel_times(const char **names, float *ms, int cap)
{
    return copy_times(kStageNames, g_mlp_times.ms, g_mlp_times.n, names, ms, cap);
}

atg_status atg_mlp_scan_device(const void *d_bytes, uint64_t bytes_cap,
                               const atg_aob_title *titles, uint32_t n_titles,
                               atg_pcm_format format, atg_mlp_result *results,
                               uint64_t *total_samples, atg_mlp_unit *units,
                               uint64_t units_cap, void *stream)
{
    uint64_t n_sectors = 0;
    atg_status st = aob_check_args(g_mlp_err, true, d_bytes, bytes_cap, titles, n_titles,
                                   (int)format, results, &n_sectors);
    if (st != ATG_OK)
        return st;
    if (total_samples)
        *total_samples = 0;
    if (!n_titles)
        return ATG_OK;
    DeviceContexts<MlpCtx>::Held c;
    if ((st = g_ctxs.hold(d_bytes, g_mlp_err, c)) != ATG_OK)
        return st;
    return run_locked(*c, d_bytes, titles, n_titles, n_sectors, (int)format, results,
                      total_samples, units, units_cap, false, nullptr, 0, (hipStream_t)stream);
}

atg_status atg_mlp_decode_device(const void *d_bytes, uint64_t bytes_cap,
                                 const atg_aob_title *titles, uint32_t n_titles, void *d_pcm,
                                 atg_pcm_format format, uint64_t pcm_cap_samples,
                                 atg_mlp_result *results, void *stream)
{
    uint64_t n_sectors = 0;
    atg_status st = aob_check_args(g_mlp_err, true, d_bytes, bytes_cap, titles, n_titles,
                                   (int)format, results, &n_sectors);
    if (st != ATG_OK)
        return st;
    if (n_titles && pcm_cap_samples && !d_pcm)
        return g_mlp_err.fail(ATG_ERR_INVALID, "NULL argument");
    if ((uintptr_t)d_pcm & 15u)
        return g_mlp_err.fail(ATG_ERR_INVALID, "d_pcm must be 16-byte aligned");
    if (!n_titles)
        return ATG_OK;
    DeviceContexts<MlpCtx>::Held c;
    if ((st = g_ctxs.hold(d_bytes, g_mlp_err, c)) != ATG_OK)
        return st;
    return run_locked(*c, d_bytes, titles, n_titles, n_sectors, (int)format, results, nullptr,
                      nullptr, 0, true, d_pcm, pcm_cap_samples, (hipStream_t)stream);
}

atg_status atg_mlp_decode_host(int device, const void *bytes, uint64_t n_bytes,
                               const atg_aob_title *titles, uint32_t n_titles, void *pcm,
                               atg_pcm_format format, uint64_t pcm_cap_samples,
                               atg_mlp_result *results)
{
    uint64_t n_sectors = 0;
    atg_status st = aob_check_args(g_mlp_err, false, bytes, n_bytes, titles, n_titles,
                                   (int)format, results, &n_sectors);
    if (st != ATG_OK)
        return st;
    if (n_titles && pcm_cap_samples && !pcm)
        return g_mlp_err.fail(ATG_ERR_INVALID, "NULL argument");
    if (!n_titles)
        return ATG_OK;
    if ((st = use_device(device, g_mlp_err)) != ATG_OK)
        return st;
    const uint64_t ssize = format == ATG_PCM_S16 ? 2 : 4;
    DevTemp d_bytes, d_pcm;
    ATG_HIP_TRY(g_mlp_err, d_bytes.alloc(std::max<uint64_t>(n_bytes, 16)),
                "hipMalloc(&d_bytes, std::max<uint64_t>(n_bytes, 16))");
    hipError_t e = d_pcm.alloc(std::max<uint64_t>(pcm_cap_samples * ssize, 16));
    if (e == hipSuccess)
        e = hipMemcpy(d_bytes.p, bytes, n_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        st = atg_mlp_decode_device(d_bytes.p, n_bytes, titles, n_titles, d_pcm.p, format,
                                   pcm_cap_samples, results, nullptr);
        // only the titles' own sample ranges are written
        for (uint32_t i = 0; st == ATG_OK && e == hipSuccess && i < n_titles; ++i) {
            const uint64_t n = results[i].good_frames * results[i].channels;
            if (n)
                e = hipMemcpy((char *)pcm + results[i].sample_offset * ssize,
                              (const char *)d_pcm.p + results[i].sample_offset * ssize,
                              n * ssize, hipMemcpyDeviceToHost);
        }
    }
    if (e != hipSuccess)
        return g_mlp_err.fail(ATG_ERR_DEVICE, std::string("staging: ") + hipGetErrorString(e));
    return st;
}

} // extern "C"
