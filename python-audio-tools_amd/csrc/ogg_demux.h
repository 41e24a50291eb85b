// ogg_demux.h — the Ogg container pass of the Ogg FLAC decoder
// (ogg_demux.hip): tables shared with flac_decode.hip and the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr uint32_t kOggNoPage = 0xFFFFFFFFu;
constexpr uint32_t kOggCrcChunk = 256; // bytes of a page one lane checksums

// one stream of the batch: its image, and (after the host's prefixes) where
// its pages, checksum chunks, packets and compacted bytes go
struct OggStream {
    uint64_t start, end;   // image bytes [start, end) of the batch buffer
    uint64_t page_base;    // first OggPage slot
    uint64_t chunk_base;   // first checksum chunk
    uint64_t pkt_base;     // first packet slot
    uint64_t out_base;     // byte of the compacted buffer (16-byte aligned)
};

// what the page walk found (magic, version and EOF checks only)
struct OggWalk {
    uint32_t pages;      // pages before the failure or through the end-of-stream page
    int32_t status;      // ATG_OGG_OK (ended by its flag), _MAGIC, _VERSION, _PREMATURE_EOF
    uint64_t fail_off;   // byte (from the image start) of the failing page
    uint32_t packets;    // lacing values below 255 in those pages
    uint32_t pad;
    uint64_t body_bytes; // body bytes of those pages
    uint64_t chunks;     // checksum chunks of those pages
};

struct OggPage {
    uint64_t off;        // absolute byte of the page
    uint64_t body_off;   // body bytes of the stream's pages before this one
    uint64_t chunk_base; // first checksum chunk (batch-wide)
    uint32_t nseg, body; // lacing values, body bytes
    uint32_t flags, crc; // header type byte, stored checksum
    uint32_t first_pkt;  // packets ended in the pages before (stream-relative)
    uint32_t carry;      // bytes of an unfinished packet carried into this page
    uint32_t stream;
    uint32_t pad;
};

// per stream, once the checksums are known: what is delivered
struct OggSum {
    uint32_t pages;     // pages before the first failure
    uint32_t packets;   // packets completed in them
    uint64_t bytes;     // their body bytes (the compacted stream)
    uint32_t fail_page; // kOggNoPage when the stream ended by its flag
    int32_t status;     // ATG_OGG_OK .. ATG_OGG_PREMATURE_EOF
    uint64_t fail_off;  // byte of the failing page from the image start
};

hipError_t ogg_upload_tables();
// the device addresses of the uploaded tables, for the muxer (ogg_mux.hip):
// crc[4][256] slicing tables, adv[17][32] "2^m zero bytes" matrices
hipError_t ogg_crc_tables(const uint32_t **crc, const uint32_t **adv);
// the page walk, one wave per stream; pass 1 counts (walk), pass 2 also fills
// the page records
hipError_t launch_ogg_walk(const uint8_t *data, const OggStream *streams, uint32_t n, int pass,
                           OggWalk *walk, OggPage *pages, hipStream_t s);
// CRC-32 of every walked page, a lane per kOggCrcChunk bytes, into acc[page]
// (zeroed by the caller)
hipError_t launch_ogg_crc(const uint32_t *w, uint64_t nw, const OggPage *pages, uint64_t npages,
                          uint64_t nchunks, uint32_t *acc, hipStream_t s);
// first failing page per stream and what is delivered before it
hipError_t launch_ogg_summary(const OggStream *streams, uint32_t n, const OggWalk *walk,
                              const OggPage *pages, const uint32_t *acc, OggSum *sum,
                              hipStream_t s);
// the packet table of the delivered pages: position in the compacted buffer,
// length and stream of every packet
hipError_t launch_ogg_packets(const uint8_t *data, const OggStream *streams, const OggSum *sum,
                              const OggPage *pages, uint64_t npages, uint64_t *pk_pos,
                              uint32_t *pk_len, uint32_t *pk_trk, hipStream_t s);
// page bodies to the compacted buffer (stream t at out_base, out_cap[t] bytes
// with the padding zeroed)
hipError_t launch_ogg_gather(const uint32_t *w, uint64_t nw, const OggStream *streams,
                             const OggSum *sum, const OggPage *pages, uint32_t n,
                             uint64_t max_out, uint32_t *out, hipStream_t s);
