// ogg_mux.hip — the Ogg container of the MI355X batch Ogg FLAC encoder: the
// page layout of DESIGN.md section 4k over a batch of finished FLAC frames.
//
// The FLAC encoder leaves every track's frames back to back (FrameDesc.bytes,
// FrameDesc.out_off) in a staging buffer.  A packet of n bytes is n / 255
// lacing values of 255 and then n % 255, and every lacing value takes one
// *slot*; page p of a track holds the slots [p S, (p + 1) S).  With a page
// per packet a packet's first slot is the next multiple of S (the slots
// between are empty and close the page), otherwise the slots are the running
// segment count -- one rule for both layouts.  Since the frames are
// contiguous in the staging buffer, so is every page's body.  The passes:
//
//   k_ogg_plan     block per track: a block scan over its frames gives each
//                  packet's first slot, the segments and PCM frames before
//                  it; a second sweep the byte of the page its packet begins
//                  on.  Track totals: audio pages and image bytes.
//   k_ogg_hdr_*    the header pages, the same bytes for every track but the
//                  serial number, STREAMINFO (copied from the staged native
//                  header, so MD5 and frame sizes are final) and the
//                  end-of-stream flag of a track without frames.
//   k_ogg_pages    wave per audio page: the owner packet of its first slot
//                  (binary search), four slots per lane, the 27 header bytes
//                  and the lacing table, one record per page.
//   k_ogg_split    wave per audio page: its body from the staging buffer
//                  (dword stores to aligned destinations).
//   k_ogg_mux_crc  wave per page, coalesced: lane l takes the aligned 16-byte
//                  blocks l, l + 64, ... -- each block's own CRC-32 by the
//                  slicing tables of ogg_demux.hip, folded with that file's
//                  "1024 zero bytes" matrix (as byte tables in LDS) between
//                  a lane's blocks -- then advances over the rest of the
//                  page with the 2^m-zero-byte matrices; xor-ed across the
//                  wave, written to bytes 22-25.
#include <hip/hip_runtime.h>

#include "crc_common.h"
#include "ogg_demux.h"
#include "ogg_mux.h"
#include "table_search.h"
#include "wave.h"

namespace {

// exclusive prefix of v over a 256-thread block; *total = the block's sum
__device__ __forceinline__ uint64_t block_excl_scan_u64(uint64_t v, uint64_t *wsum,
                                                        uint64_t *total)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const uint64_t x = wave_incl_scan_u64(v, lane);
    __syncthreads(); // the previous use of wsum is over
    if (lane == 63)
        wsum[wave] = x;
    __syncthreads();
    uint64_t below = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint64_t s = wsum[w];
        below += w < wave ? s : 0ull;
        all += s;
    }
    *total = all;
    return below + x - v;
}

// the last frame i of [0, n) with slot0 <= q (slot0 ascends, fr[0].slot0 = 0)
__device__ __forceinline__ uint32_t owner_of(const OggMuxFrame *fr, uint32_t n, uint64_t q)
{
    return last_le(fr, n, q, &OggMuxFrame::slot0);
}

__global__ __launch_bounds__(256) void k_ogg_plan(OggMuxParams mp,
                                                  const OggMuxTrack *__restrict__ tracks,
                                                  const uint32_t *__restrict__ order,
                                                  const FrameDesc *__restrict__ fd,
                                                  const FrameInfo *__restrict__ frames,
                                                  OggMuxFrame *__restrict__ fr_all,
                                                  uint64_t *__restrict__ pgoff,
                                                  OggMuxOut *__restrict__ outs)
{
    __shared__ uint64_t wsum[4];
    const uint32_t t = blockIdx.x;
    if (t >= mp.n_tracks)
        return;
    const OggMuxTrack tr = tracks[t];
    OggMuxFrame *fr = fr_all + tr.first_pos;
    const uint64_t S = mp.S;
    uint64_t c_seg = 0, c_slot = 0, c_pcm = 0, c_bytes = 0;
    for (uint32_t base = 0; base < tr.n_frames; base += 256u) {
        const uint32_t i = base + threadIdx.x;
        const bool on = i < tr.n_frames;
        uint32_t b = 0, off = 0, n_pcm = 0;
        if (on) {
            const uint32_t f = order[tr.first_pos + i];
            b = fd[f].bytes;
            off = fd[f].out_off;
            n_pcm = frames[f].n;
        }
        const uint64_t ns = on ? b / 255u + 1u : 0u;
        const uint64_t adv = mp.per_packet ? (ns + S - 1u) / S * S : ns;
        uint64_t t_seg, t_slot, t_pcm, t_bytes;
        const uint64_t e_seg = block_excl_scan_u64(ns, wsum, &t_seg);
        const uint64_t e_slot = block_excl_scan_u64(adv, wsum, &t_slot);
        const uint64_t e_pcm = block_excl_scan_u64(n_pcm, wsum, &t_pcm);
        (void)block_excl_scan_u64(b, wsum, &t_bytes);
        if (on) {
            OggMuxFrame o;
            o.slot0 = c_slot + e_slot;
            o.segpref = c_seg + e_seg;
            o.gran = c_pcm + e_pcm + n_pcm;
            o.bytepref = off;
            o.bytes = b;
            fr[i] = o;
        }
        c_seg += t_seg;
        c_slot += t_slot;
        c_pcm += t_pcm;
        c_bytes += t_bytes;
    }
    const uint64_t pages = (c_slot + S - 1u) / S;
    if (threadIdx.x == 0) {
        OggMuxOut o;
        o.bytes = mp.hdr_bytes + 27u * pages + c_seg + c_bytes;
        o.pages = (uint32_t)pages;
        o.pad = 0;
        outs[t] = o;
    }
    __syncthreads(); // the block's frame records are written
    for (uint32_t i = threadIdx.x; i < tr.n_frames; i += 256u) {
        const uint64_t pg = fr[i].slot0 / S, q0 = pg * S;
        const uint32_t j = owner_of(fr, i + 1u, q0);
        const uint64_t d = q0 - fr[j].slot0;
        pgoff[tr.first_pos + i] = mp.hdr_bytes + 27u * pg + fr[j].segpref + d +
                                  fr[j].bytepref + 255u * d;
    }
}

// the header pages' bytes to every track's image (a dword per thread)
__global__ __launch_bounds__(256) void k_ogg_hdr_copy(OggMuxParams mp,
                                                      const OggMuxTrack *__restrict__ tracks,
                                                      const uint8_t *__restrict__ tmpl,
                                                      uint8_t *__restrict__ out)
{
    const uint64_t b = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (b >= mp.hdr_bytes)
        return;
    for (uint32_t t = blockIdx.y; t < mp.n_tracks; t += gridDim.y) {
        uint8_t *dst = out + tracks[t].out_base + b; // (out_base is 16-byte aligned)
        if (b + 4u <= mp.hdr_bytes)
            *(uint32_t *)dst = *(const uint32_t *)(tmpl + b);
        else
            for (uint64_t k = 0; b + k < mp.hdr_bytes; ++k)
                dst[k] = tmpl[b + k];
    }
}

// what differs between the tracks' header pages, and their page records
__global__ __launch_bounds__(64) void k_ogg_hdr_patch(OggMuxParams mp,
                                                      const OggMuxTrack *__restrict__ tracks,
                                                      const uint32_t *__restrict__ hp, // off, size
                                                      const uint8_t *__restrict__ tmpl,
                                                      const uint8_t *__restrict__ stage,
                                                      uint8_t *__restrict__ out,
                                                      OggMuxPage *__restrict__ pages)
{
    const uint32_t t = blockIdx.x;
    if (t >= mp.n_tracks)
        return;
    const OggMuxTrack tr = tracks[t];
    const uint32_t lane = threadIdx.x;
    const uint32_t serial = mp.serial + t;
    uint8_t *img = out + tr.out_base;
    for (uint32_t k = lane; k < mp.hdr_pages; k += 64u) {
        const uint32_t off = hp[2u * k], size = hp[2u * k + 1u];
        for (uint32_t j = 0; j < 4u; ++j)
            img[off + 14u + j] = (uint8_t)(serial >> (8u * j));
        if (k + 1u == mp.hdr_pages && tr.n_frames == 0u)
            img[off + 5u] = (uint8_t)(tmpl[off + 5u] | 4u); // the stream ends here
        OggMuxPage p;
        p.off = tr.out_base + off;
        p.src = 0;
        p.size = size;
        p.nseg = tmpl[off + 26u];
        pages[tr.page_base + k] = p;
    }
    // STREAMINFO: 34 bytes after "fLaC" and the block header of the native
    // image, to byte 17 of the first packet (page 0: 27 + 1 lacing value)
    if (lane < 34u)
        img[28u + 17u + lane] = stage[tr.src_base + 8u + lane];
}

__global__ __launch_bounds__(256) void k_ogg_pages(OggMuxParams mp,
                                                   const OggMuxTrack *__restrict__ tracks,
                                                   const OggMuxFrame *__restrict__ fr_all,
                                                   const OggMuxOut *__restrict__ outs,
                                                   uint8_t *__restrict__ out,
                                                   OggMuxPage *__restrict__ pages)
{
    const uint64_t p = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t S = mp.S;
    for (uint32_t t = blockIdx.y; t < mp.n_tracks; t += gridDim.y) {
        const uint32_t np = outs[t].pages;
        if (p >= np)
            continue;
        const OggMuxTrack tr = tracks[t];
        const OggMuxFrame *fr = fr_all + tr.first_pos;
        const uint64_t q0 = p * S;
        const uint32_t own = owner_of(fr, tr.n_frames, q0);
        const OggMuxFrame fo = fr[own];
        const uint64_t d = q0 - fo.slot0;
        // four slots per lane: the lacing value, or none past the page's last
        uint32_t v[4], nseg = 0, body = 0, ends = 0; // ends: 1 + last packet ending here
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t j = 4u * lane + (uint32_t)k;
            v[k] = 0xFFFFFFFFu;
            if (j < S) {
                const uint64_t q = q0 + j;
                // the packet of slot q lies at most j packets after the owner
                const uint32_t hi = own + j + 1u < tr.n_frames ? own + j + 1u : tr.n_frames;
                const uint32_t i = own + owner_of(fr + own, hi - own, q);
                const uint64_t r = q - fr[i].slot0, ns = fr[i].bytes / 255u + 1u;
                if (r < ns) {
                    v[k] = r + 1u < ns ? 255u : fr[i].bytes % 255u;
                    ++nseg;
                    body += v[k];
                    ends = v[k] < 255u ? i + 1u : ends;
                }
            }
        }
        nseg = wave_sum_u32(nseg);
        body = wave_sum_u32(body);
        ends = wave_max_u32(ends);
        const int64_t gran = ends ? (int64_t)fr[ends - 1u].gran : -1;
        const uint64_t rel = mp.hdr_bytes + 27u * p + fo.segpref + d + fo.bytepref + 255u * d;
        uint8_t *pg = out + tr.out_base + rel;
        const uint32_t flags = (d ? 1u : 0u) | (p + 1u == np ? 4u : 0u);
        const uint32_t serial = mp.serial + t, seq = mp.hdr_pages + (uint32_t)p;
        if (lane < 27u) {
            uint32_t b = 0;
            if (lane < 4u)
                b = 0x5367674Fu >> (8u * lane); // "OggS"
            else if (lane == 5u)
                b = flags;
            else if (lane >= 6u && lane < 14u)
                b = (uint32_t)((uint64_t)gran >> (8u * (lane - 6u)));
            else if (lane >= 14u && lane < 18u)
                b = serial >> (8u * (lane - 14u));
            else if (lane >= 18u && lane < 22u)
                b = seq >> (8u * (lane - 18u));
            else if (lane == 26u)
                b = nseg;
            pg[lane] = (uint8_t)b; // (the checksum field stays 0 for k_ogg_crc)
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (v[k] != 0xFFFFFFFFu)
                pg[27u + 4u * lane + (uint32_t)k] = (uint8_t)v[k];
        if (lane == 0u) {
            OggMuxPage r;
            r.off = tr.out_base + rel;
            r.src = tr.src_base + mp.native_hdr + fo.bytepref + 255u * d;
            r.size = 27u + nseg + body;
            r.nseg = nseg;
            pages[tr.page_base + mp.hdr_pages + p] = r;
        }
    }
}

__device__ __forceinline__ uint32_t ld_u32(const uint8_t *p) // any alignment
{
    uint32_t x;
    __builtin_memcpy(&x, p, 4);
    return x;
}

__global__ __launch_bounds__(256) void k_ogg_split(OggMuxParams mp,
                                                   const OggMuxTrack *__restrict__ tracks,
                                                   const OggMuxOut *__restrict__ outs,
                                                   const OggMuxPage *__restrict__ pages,
                                                   const uint8_t *__restrict__ stage,
                                                   uint8_t *__restrict__ out)
{
    const uint64_t p = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t t = blockIdx.y; t < mp.n_tracks; t += gridDim.y) {
        if (p >= outs[t].pages)
            continue;
        const OggMuxPage r = pages[tracks[t].page_base + mp.hdr_pages + p];
        const uint32_t n = r.size - 27u - r.nseg;
        uint8_t *dst = out + r.off + 27u + r.nseg;
        const uint8_t *src = stage + r.src;
        // bytes up to the first aligned destination word, words, the rest
        uint32_t head = (uint32_t)((4u - ((uint64_t)dst & 3u)) & 3u);
        head = head < n ? head : n;
        const uint32_t words = (n - head) / 4u, tail = head + 4u * words;
        if (lane < head)
            dst[lane] = src[lane];
        for (uint32_t w = lane; w < words; w += 64u)
            *(uint32_t *)(dst + head + 4u * w) = ld_u32(src + head + 4u * w);
        if (lane < n - tail)
            dst[tail + lane] = src[tail + lane];
    }
}

__global__ __launch_bounds__(256) void k_ogg_mux_crc(OggMuxParams mp,
                                                     const OggMuxTrack *__restrict__ tracks,
                                                     const OggMuxOut *__restrict__ outs,
                                                     const OggMuxPage *__restrict__ pages,
                                                     const uint32_t *__restrict__ crc_tab,
                                                     const uint32_t *__restrict__ adv,
                                                     uint8_t *__restrict__ out)
{
    // T: the slicing tables.  A: a state advanced over 1024 zero bytes, by
    // its bytes (the 2^10 matrix as four 256-entry tables)
    __shared__ uint32_t T[4][256], A[4][256];
    for (uint32_t i = threadIdx.x; i < 1024u; i += 256u) {
        T[i >> 8][i & 255u] = crc_tab[i];
        uint32_t v = 0;
        for (uint32_t j = 0; j < 8u; ++j)
            v ^= ((i >> j) & 1u) ? adv[32u * 10u + 8u * (i >> 8) + j] : 0u;
        A[i >> 8][i & 255u] = v;
    }
    __syncthreads();
    const uint64_t p = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t t = blockIdx.y; t < mp.n_tracks; t += gridDim.y) {
        if (p >= (uint64_t)mp.hdr_pages + outs[t].pages)
            continue;
        const OggMuxPage r = pages[tracks[t].page_base + p];
        const uint8_t *pg = out + r.off;
        // (bytes 22-25 are zero in the image until this kernel writes them)
        // The CRC is linear: the page's is the xor of each aligned 16-byte
        // block's own CRC advanced over the bytes after it.  Lane l takes the
        // blocks l, l + 64, ... (the wave loads 1024 contiguous bytes at a
        // time) and folds them Horner-wise: the ends of two of its blocks
        // lie 1024 bytes apart.
        const uint32_t size = r.size;
        uint32_t head = (uint32_t)((16u - ((uint64_t)pg & 15u)) & 15u);
        head = head < size ? head : size;
        const uint32_t nblocks = (size - head) / 16u;
        const uint4 *w = (const uint4 *)(pg + head);
        uint32_t acc = 0, z = 0; // z: bytes of the page after the lane's last block
        if (lane < nblocks) {
            uint32_t k = lane;
            for (;; k += 64u) {
                const uint4 v = w[k];
                const uint32_t x4[4] = {v.x, v.y, v.z, v.w};
                uint32_t c = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t x = __builtin_bswap32(x4[i]) ^ c;
                    c = T[3][x >> 24] ^ T[2][(x >> 16) & 0xFFu] ^ T[1][(x >> 8) & 0xFFu] ^
                        T[0][x & 0xFFu];
                }
                acc ^= c;
                if (k + 64u >= nblocks)
                    break;
                acc = A[3][acc >> 24] ^ A[2][(acc >> 16) & 0xFFu] ^ A[1][(acc >> 8) & 0xFFu] ^
                      A[0][acc & 0xFFu];
            }
            z = size - head - 16u * (k + 1u);
        }
        for (int m = 0; z; ++m, z >>= 1)
            if (z & 1u)
                acc = crc_advance<32>(adv + 32 * m, acc);
        if (lane == 63u) { // the bytes before the first block
            uint32_t hc = 0;
            for (uint32_t q = 0; q < head; ++q)
                hc = (hc << 8) ^ T[0][(hc >> 24) ^ pg[q]];
            uint32_t zh = size - head;
            for (int m = 0; zh; ++m, zh >>= 1)
                if (zh & 1u)
                    hc = crc_advance<32>(adv + 32 * m, hc);
            acc ^= hc;
        }
        if (lane == 0u) { // the bytes after the last block: nothing follows them
            uint32_t tc = 0;
            for (uint32_t q = head + 16u * nblocks; q < size; ++q)
                tc = (tc << 8) ^ T[0][(tc >> 24) ^ pg[q]];
            acc ^= tc;
        }
        acc = wave_xor_u32(acc);
        if (lane < 4u)
            out[r.off + 22u + lane] = (uint8_t)(acc >> (8u * lane));
    }
}

unsigned grid_y(uint32_t n) { return n < 65535u ? n : 65535u; }

} // namespace

hipError_t launch_ogg_mux_plan(const OggMuxParams &mp, const OggMuxTrack *tracks,
                               const uint32_t *order, const FrameDesc *fd,
                               const FrameInfo *frames, OggMuxFrame *fr, uint64_t *pgoff,
                               OggMuxOut *outs, hipStream_t s)
{
    if (mp.n_tracks)
        hipLaunchKernelGGL(k_ogg_plan, dim3(mp.n_tracks), dim3(256), 0, s, mp, tracks, order, fd,
                           frames, fr, pgoff, outs);
    return hipGetLastError();
}

hipError_t launch_ogg_mux_headers(const OggMuxParams &mp, const OggMuxTrack *tracks,
                                  const uint32_t *hp, const uint8_t *tmpl, const uint8_t *stage,
                                  uint8_t *out, OggMuxPage *pages, hipStream_t s)
{
    if (!mp.n_tracks)
        return hipSuccess;
    hipLaunchKernelGGL(k_ogg_hdr_copy, dim3((unsigned)((mp.hdr_bytes + 1023u) / 1024u),
                                            grid_y(mp.n_tracks)),
                       dim3(256), 0, s, mp, tracks, tmpl, out);
    hipLaunchKernelGGL(k_ogg_hdr_patch, dim3(mp.n_tracks), dim3(64), 0, s, mp, tracks, hp, tmpl,
                       stage, out, pages);
    return hipGetLastError();
}

hipError_t launch_ogg_mux_pages(const OggMuxParams &mp, const OggMuxTrack *tracks,
                                const OggMuxFrame *fr, const OggMuxOut *outs, uint8_t *out,
                                OggMuxPage *pages, uint64_t max_audio_pages, hipStream_t s)
{
    if (mp.n_tracks && max_audio_pages)
        hipLaunchKernelGGL(k_ogg_pages, dim3((unsigned)((max_audio_pages + 3u) / 4u),
                                             grid_y(mp.n_tracks)),
                           dim3(256), 0, s, mp, tracks, fr, outs, out, pages);
    return hipGetLastError();
}

hipError_t launch_ogg_mux_split(const OggMuxParams &mp, const OggMuxTrack *tracks,
                                const OggMuxOut *outs, const OggMuxPage *pages,
                                const uint8_t *stage, uint8_t *out, uint64_t max_audio_pages,
                                hipStream_t s)
{
    if (mp.n_tracks && max_audio_pages)
        hipLaunchKernelGGL(k_ogg_split, dim3((unsigned)((max_audio_pages + 3u) / 4u),
                                             grid_y(mp.n_tracks)),
                           dim3(256), 0, s, mp, tracks, outs, pages, stage, out);
    return hipGetLastError();
}

hipError_t launch_ogg_mux_crc(const OggMuxParams &mp, const OggMuxTrack *tracks,
                              const OggMuxOut *outs, const OggMuxPage *pages,
                              const uint32_t *crc_tab, const uint32_t *adv, uint8_t *out,
                              uint64_t max_audio_pages, hipStream_t s)
{
    const uint64_t np = mp.hdr_pages + max_audio_pages;
    if (mp.n_tracks)
        hipLaunchKernelGGL(k_ogg_mux_crc, dim3((unsigned)((np + 3u) / 4u), grid_y(mp.n_tracks)),
                           dim3(256), 0, s, mp, tracks, outs, pages, crc_tab, adv, out);
    return hipGetLastError();
}
