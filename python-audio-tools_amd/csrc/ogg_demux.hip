// ogg_demux.hip — the Ogg container of the MI355X batch Ogg FLAC decoder: the
// reference's page reader and packet iterator (src/ogg.c:24-119, 203-254)
// for a whole batch of .oga images at once.
//
// An Ogg stream stores what native FLAC does not -- where every frame starts
// and ends: one packet is one frame, and the lacing tables give each
// packet's length before a Rice code is read.  The passes:
//
//   k_ogg_walk     wave per stream, serial over its pages, cooperative inside
//                  a page: the lanes load the 27-byte header and the lacing
//                  table (4 values per lane), reduce the body length and
//                  count the packet terminators (values below 255).  Magic,
//                  version and premature-EOF checks in the reference's read
//                  order.  Pass 1 counts; after the host's prefix over
//                  streams pass 2 writes one record per page.  Nothing is
//                  sized from what a stream claims, and no byte outside the
//                  stream's image is read: a lacing table that promises more
//                  than the image holds is an EOF.
//   k_ogg_crc      lane per 256 bytes of a page: CRC-32 (0x04C11DB7, init 0,
//                  MSB first, no final xor, bytes 22-25 as zero) of the
//                  chunk by slicing tables in LDS, advanced over the rest of
//                  the page with "state after 2^m zero bytes" matrices and
//                  xor-ed into the page's word (the CRC is linear).  Work is
//                  per byte, so a stream of one-segment pages costs a lane
//                  per page, a 65,307-byte page 256 lanes.
//   k_ogg_summary  wave per stream: the first page whose checksum differs
//                  (a min-reduction), merged with the walk's failure -- the
//                  earliest in file order wins -- and what is delivered
//                  before it: a page is checked whole before any of its
//                  segments is handed out.
//   k_ogg_packets  wave per delivered page: a segmented scan over its lacing
//                  values gives every packet that ends in it (position in the
//                  compacted stream, length).
//   k_ogg_gather   page bodies to the compacted per-stream buffer the FLAC
//                  bit reader needs: a lane per 16 output bytes, sources
//                  unaligned (two aligned words funnel-shifted), 16-byte
//                  coalesced stores.
#include <hip/hip_runtime.h>

#include "../../include/atgpu.h"
#include "crc_common.h"
#include "ogg_demux.h"
#include "table_search.h"
#include "wave.h"

namespace {

__device__ uint32_t g_ogg_crc[4][256]; // slicing tables
__device__ uint32_t g_ogg_adv[17][32]; // state advanced by 2^m zero bytes (column images)

__device__ __forceinline__ uint32_t rd_byte(const uint8_t *d, uint64_t i, uint64_t end)
{
    return i < end ? (uint32_t)d[i] : 0u;
}

// K1: the page walk
__global__ __launch_bounds__(64) void k_ogg_walk(const uint8_t *__restrict__ data,
                                                 const OggStream *__restrict__ streams,
                                                 uint32_t n, int pass, OggWalk *__restrict__ walk,
                                                 OggPage *__restrict__ pages)
{
    const uint32_t t = blockIdx.x;
    if (t >= n)
        return;
    const int lane = (int)threadIdx.x;
    const OggStream st = streams[t];
    // pass 2 walks exactly the pages pass 1 counted
    const uint32_t limit = pass == 2 ? walk[t].pages : 0xFFFFFFFFu;
    uint64_t pos = st.start, body_off = 0, chunks = 0;
    uint32_t pg = 0, pk = 0, carry = 0;
    int32_t status = ATG_OGG_OK;
    while (pg < limit) {
        const uint64_t rem = st.end - pos;
        // the 27 header bytes that exist (lane = byte)
        const uint32_t hb = lane < 27 ? rd_byte(data, pos + (uint64_t)lane, st.end) : 0u;
        const uint32_t b0 = (uint32_t)__shfl((int)hb, 0, 64), b1 = (uint32_t)__shfl((int)hb, 1, 64);
        const uint32_t b2 = (uint32_t)__shfl((int)hb, 2, 64), b3 = (uint32_t)__shfl((int)hb, 3, 64);
        // the reference's read order (ogg.c:30-68): magic, version, the rest
        // of the header, the lacing table, the body
        if (rem < 4) { status = ATG_OGG_PREMATURE_EOF; break; }
        if (b0 != 'O' || b1 != 'g' || b2 != 'g' || b3 != 'S') { status = ATG_OGG_MAGIC; break; }
        if (rem < 5) { status = ATG_OGG_PREMATURE_EOF; break; }
        if ((uint32_t)__shfl((int)hb, 4, 64) != 0u) { status = ATG_OGG_VERSION; break; }
        if (rem < 27) { status = ATG_OGG_PREMATURE_EOF; break; }
        const uint32_t flags = (uint32_t)__shfl((int)hb, 5, 64);
        const uint32_t crc = (uint32_t)__shfl((int)hb, 22, 64) |
                             ((uint32_t)__shfl((int)hb, 23, 64) << 8) |
                             ((uint32_t)__shfl((int)hb, 24, 64) << 16) |
                             ((uint32_t)__shfl((int)hb, 25, 64) << 24);
        const uint32_t nseg = (uint32_t)__shfl((int)hb, 26, 64);
        if (rem < 27ull + nseg) { status = ATG_OGG_PREMATURE_EOF; break; }
        // lacing values 4 lane .. 4 lane + 3
        uint32_t sum = 0, terms = 0, tail = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t i = 4u * (uint32_t)lane + (uint32_t)k;
            const bool on = i < nseg;
            const uint32_t v = on ? rd_byte(data, pos + 27u + i, st.end) : 0u;
            sum += v;
            tail = on && v < 255u ? 0u : tail + v; // bytes after the lane's last terminator
            terms += on && v < 255u ? 1u : 0u;
        }
        const uint32_t body = wave_sum_u32(sum);
        const uint32_t nterm = wave_sum_u32(terms);
        if (rem < 27ull + nseg + body) { status = ATG_OGG_PREMATURE_EOF; break; }
        // bytes of an unfinished packet after the page's last terminator
        const uint32_t excl = wave_excl_scan_u32(sum, lane);
        const uint64_t tm = __ballot(terms != 0u);
        uint32_t carry_out = carry + body;
        if (tm) {
            const int L = 63 - __builtin_clzll(tm);
            const uint32_t upto = (uint32_t)__shfl((int)(excl + sum), L, 64);
            carry_out = (uint32_t)__shfl((int)tail, L, 64) + (body - upto);
        }
        const uint64_t size = 27ull + nseg + body;
        if (pass == 2 && lane == 0) {
            OggPage p;
            p.off = pos;
            p.body_off = body_off;
            p.chunk_base = st.chunk_base + chunks;
            p.nseg = nseg;
            p.body = body;
            p.flags = flags;
            p.crc = crc;
            p.first_pkt = pk;
            p.carry = carry;
            p.stream = t;
            p.pad = 0;
            pages[st.page_base + pg] = p;
        }
        chunks += (size + kOggCrcChunk - 1) / kOggCrcChunk;
        pk += nterm;
        body_off += body;
        carry = carry_out;
        pos += size;
        ++pg;
        if (flags & 4u) // the end-of-stream page: nothing after it is read
            break;
    }
    if (pass == 1 && lane == 0) {
        OggWalk o;
        o.pages = pg;
        o.status = status;
        o.fail_off = pos - st.start;
        o.packets = pk;
        o.pad = 0;
        o.body_bytes = body_off;
        o.chunks = chunks;
        walk[t] = o;
    }
}

// K2: page checksums, a lane per chunk
__global__ __launch_bounds__(256) void k_ogg_crc(const uint32_t *__restrict__ w, uint64_t nw,
                                                 const OggPage *__restrict__ pages,
                                                 uint64_t npages, uint64_t nchunks,
                                                 uint32_t *__restrict__ acc)
{
    __shared__ uint32_t T[4][256];
    for (uint32_t i = threadIdx.x; i < 1024; i += blockDim.x)
        T[i >> 8][i & 255] = g_ogg_crc[i >> 8][i & 255];
    __syncthreads();
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks || !npages)
        return;
    // the chunk's page: the last one with chunk_base <= c
    const uint64_t lo = last_le(pages, npages, c, &OggPage::chunk_base);
    const OggPage p = pages[lo];
    const uint32_t size = 27u + p.nseg + p.body;
    const uint32_t from = (uint32_t)(c - p.chunk_base) * kOggCrcChunk;
    if (from >= size)
        return;
    const uint32_t upto = from + kOggCrcChunk < size ? from + kOggCrcChunk : size;
    uint32_t crc = 0, q = from;
    for (; q + 4 <= upto; q += 4) {
        uint32_t x = be32_at(w, nw - 1, p.off + q);
        // the checksum field (bytes 22-25) counts as zero
        x = q == 20u ? x & 0xFFFF0000u : (q == 24u ? x & 0x0000FFFFu : x);
        x ^= crc;
        crc = T[3][x >> 24] ^ T[2][(x >> 16) & 0xFFu] ^ T[1][(x >> 8) & 0xFFu] ^ T[0][x & 0xFFu];
    }
    if (q < upto) { // the page's last 1-3 bytes (of a 27-byte page: 24, 25 of the field, 26)
        const uint32_t x = be32_at(w, nw - 1, p.off + q);
        for (uint32_t k = 0; q < upto; ++q, ++k) {
            const uint32_t b = q >= 22u && q < 26u ? 0u : (x >> (24u - 8u * k)) & 0xFFu;
            crc = (crc << 8) ^ T[0][(crc >> 24) ^ b];
        }
    }
    // advance over the rest of the page
    uint32_t z = size - upto;
    for (int m = 0; z; ++m, z >>= 1)
        if (z & 1u)
            crc = crc_advance<32>(g_ogg_adv[m], crc);
    if (crc)
        atomicXor(&acc[lo], crc);
}

// K3: per stream, the first failing page and what is delivered before it
__global__ __launch_bounds__(64) void k_ogg_summary(const OggStream *__restrict__ streams,
                                                    uint32_t n, const OggWalk *__restrict__ walk,
                                                    const OggPage *__restrict__ pages,
                                                    const uint32_t *__restrict__ acc,
                                                    OggSum *__restrict__ sum)
{
    const uint32_t t = blockIdx.x;
    if (t >= n)
        return;
    const OggStream st = streams[t];
    const OggWalk wk = walk[t];
    uint32_t bad = kOggNoPage;
    for (uint32_t i = threadIdx.x; i < wk.pages; i += 64u)
        if (bad == kOggNoPage && acc[st.page_base + i] != pages[st.page_base + i].crc)
            bad = i;
    bad = wave_min_u32(bad);
    if (threadIdx.x != 0)
        return;
    OggSum o;
    if (bad != kOggNoPage) { // earlier in file order than whatever stopped the walk
        const OggPage p = pages[st.page_base + bad];
        o.pages = bad;
        o.packets = p.first_pkt;
        o.bytes = p.body_off;
        o.fail_page = bad;
        o.status = ATG_OGG_CHECKSUM;
        o.fail_off = p.off - st.start;
    } else {
        o.pages = wk.pages;
        o.packets = wk.packets;
        o.bytes = wk.body_bytes;
        o.fail_page = wk.status == ATG_OGG_OK ? kOggNoPage : wk.pages;
        o.status = wk.status;
        o.fail_off = wk.status == ATG_OGG_OK ? 0 : wk.fail_off;
    }
    sum[t] = o;
}

// K4: the packets that end in each delivered page (wave per page)
__global__ __launch_bounds__(256) void k_ogg_packets(const uint8_t *__restrict__ data,
                                                     const OggStream *__restrict__ streams,
                                                     const OggSum *__restrict__ sum,
                                                     const OggPage *__restrict__ pages,
                                                     uint64_t npages, uint64_t *__restrict__ pk_pos,
                                                     uint32_t *__restrict__ pk_len,
                                                     uint32_t *__restrict__ pk_trk)
{
    const uint64_t pi = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (pi >= npages)
        return;
    const int lane = (int)(threadIdx.x & 63u);
    const OggPage p = pages[pi];
    const OggStream st = streams[p.stream];
    if (pi - st.page_base >= sum[p.stream].pages) // the failing page and those after it
        return;
    uint32_t v[4], s = 0, terms = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t i = 4u * (uint32_t)lane + (uint32_t)k;
        const bool on = i < p.nseg; // inside the image: the walk checked the table
        v[k] = on ? (uint32_t)data[p.off + 27u + i] : 255u;
        s += on ? v[k] : 0u;
        terms += on && v[k] < 255u ? 1u : 0u;
    }
    const uint32_t excl = wave_excl_scan_u32(s, lane);
    const uint32_t rank = wave_excl_scan_u32(terms, lane);
    // where the packet open at this lane's first value began: the end of the
    // last terminator in the lanes below, or the carried bytes before the page
    uint32_t my_last = 0, run = excl; // page-relative end of the lane's last terminator
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool on = 4u * (uint32_t)lane + (uint32_t)k < p.nseg;
        run += on ? v[k] : 0u;
        my_last = on && v[k] < 255u ? run : my_last;
    }
    const uint64_t tm = __ballot(terms != 0u) & ((1ull << lane) - 1ull);
    const int src = tm ? 63 - __builtin_clzll(tm) : 0;
    const uint32_t below = (uint32_t)__shfl((int)my_last, src, 64);
    // page-relative, offset by the carry so that it cannot go negative
    uint64_t begin = tm ? (uint64_t)p.carry + below : 0u;
    const uint64_t base = st.out_base + p.body_off - p.carry;
    uint32_t r = rank;
    run = excl;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool on = 4u * (uint32_t)lane + (uint32_t)k < p.nseg;
        run += on ? v[k] : 0u;
        if (on && v[k] < 255u) {
            const uint64_t end = (uint64_t)p.carry + run;
            const uint64_t slot = st.pkt_base + p.first_pkt + r;
            pk_pos[slot] = base + begin;
            pk_len[slot] = (uint32_t)(end - begin);
            pk_trk[slot] = p.stream;
            begin = end;
            ++r;
        }
    }
}

// K5: the delivered pages' bodies, compacted (grid.y strides the streams)
__global__ __launch_bounds__(256) void k_ogg_gather(const uint32_t *__restrict__ w, uint64_t nw,
                                                    const OggStream *__restrict__ streams,
                                                    const OggSum *__restrict__ sum,
                                                    const OggPage *__restrict__ pages, uint32_t n,
                                                    uint32_t *__restrict__ out)
{
    for (uint32_t t = blockIdx.y; t < n; t += gridDim.y) {
        const OggStream st = streams[t];
        const OggSum sm = sum[t];
        const uint64_t cap = (sm.bytes + 15u) & ~15ull; // the stream's slot, padding zeroed
        const uint64_t b0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16u;
        if (b0 >= cap)
            continue;
        uint32_t q[4] = {0, 0, 0, 0};
        if (b0 < sm.bytes) {
            // the page holding byte b0: the last delivered one with body_off <= b0
            const OggPage *pg = pages + st.page_base;
            uint32_t pi = last_le(pg, sm.pages, b0, &OggPage::body_off);
            OggPage p = pg[pi];
            for (int k = 0; k < 4; ++k) {
                const uint64_t b = b0 + 4u * (uint32_t)k;
                if (b >= sm.bytes)
                    break;
                while (b >= p.body_off + p.body && pi + 1 < sm.pages) // (empty bodies too)
                    p = pg[++pi];
                if (b + 4 <= p.body_off + p.body) { // the whole word inside one page
                    const uint64_t src = p.off + 27u + p.nseg + (b - p.body_off);
                    q[k] = __builtin_bswap32(be32_at(w, nw - 1, src));
                } else { // a page boundary (or the stream's end) inside the word
                    uint32_t x = 0, pj = pi;
                    OggPage pp = p;
                    for (uint32_t j = 0; j < 4 && b + j < sm.bytes; ++j) {
                        while (b + j >= pp.body_off + pp.body && pj + 1 < sm.pages)
                            pp = pg[++pj];
                        const uint64_t src = pp.off + 27u + pp.nseg + (b + j - pp.body_off);
                        x |= (be32_at(w, nw - 1, src) >> 24) << (8u * j);
                    }
                    q[k] = x;
                }
            }
        }
        *(uint4 *)(out + (st.out_base + b0) / 4u) = make_uint4(q[0], q[1], q[2], q[3]);
    }
}

} // namespace

hipError_t ogg_upload_tables()
{
    static uint32_t tab[4][256];
    static uint32_t adv[17][32];
    crc_build_tables<32>(0x04C11DB7u, &tab[0][0], 4);
    crc_build_advance<32>(tab[0], &adv[0][0], 17);
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_ogg_crc), tab, sizeof(tab));
    if (e == hipSuccess)
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_ogg_adv), adv, sizeof(adv));
    return e;
}

hipError_t ogg_crc_tables(const uint32_t **crc, const uint32_t **adv)
{
    hipError_t e = hipGetSymbolAddress((void **)crc, HIP_SYMBOL(g_ogg_crc));
    if (e == hipSuccess)
        e = hipGetSymbolAddress((void **)adv, HIP_SYMBOL(g_ogg_adv));
    return e;
}

hipError_t launch_ogg_walk(const uint8_t *data, const OggStream *streams, uint32_t n, int pass,
                           OggWalk *walk, OggPage *pages, hipStream_t s)
{
    if (n)
        hipLaunchKernelGGL(k_ogg_walk, dim3(n), dim3(64), 0, s, data, streams, n, pass, walk,
                           pages);
    return hipGetLastError();
}

hipError_t launch_ogg_crc(const uint32_t *w, uint64_t nw, const OggPage *pages, uint64_t npages,
                          uint64_t nchunks, uint32_t *acc, hipStream_t s)
{
    if (nchunks)
        hipLaunchKernelGGL(k_ogg_crc, dim3((unsigned)((nchunks + 255) / 256)), dim3(256), 0, s, w,
                           nw, pages, npages, nchunks, acc);
    return hipGetLastError();
}

hipError_t launch_ogg_summary(const OggStream *streams, uint32_t n, const OggWalk *walk,
                              const OggPage *pages, const uint32_t *acc, OggSum *sum,
                              hipStream_t s)
{
    if (n)
        hipLaunchKernelGGL(k_ogg_summary, dim3(n), dim3(64), 0, s, streams, n, walk, pages, acc,
                           sum);
    return hipGetLastError();
}

hipError_t launch_ogg_packets(const uint8_t *data, const OggStream *streams, const OggSum *sum,
                              const OggPage *pages, uint64_t npages, uint64_t *pk_pos,
                              uint32_t *pk_len, uint32_t *pk_trk, hipStream_t s)
{
    if (npages)
        hipLaunchKernelGGL(k_ogg_packets, dim3((unsigned)((npages + 3) / 4)), dim3(256), 0, s, data,
                           streams, sum, pages, npages, pk_pos, pk_len, pk_trk);
    return hipGetLastError();
}

hipError_t launch_ogg_gather(const uint32_t *w, uint64_t nw, const OggStream *streams,
                             const OggSum *sum, const OggPage *pages, uint32_t n,
                             uint64_t max_out, uint32_t *out, hipStream_t s)
{
    if (n && max_out)
        hipLaunchKernelGGL(k_ogg_gather,
                           dim3((unsigned)((max_out + 16 * 256 - 1) / (16 * 256)),
                                (unsigned)(n < 65535u ? n : 65535u)),
                           dim3(256), 0, s, w, nw, streams, sum, pages, n, out);
    return hipGetLastError();
}
