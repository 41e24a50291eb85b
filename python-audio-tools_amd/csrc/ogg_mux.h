// ogg_mux.h — the Ogg container pass of the Ogg FLAC encoder (ogg_mux.hip):
// tables shared with engine.hip and the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flac_dev.h"

struct OggMuxParams {
    uint32_t n_tracks;
    uint32_t S;          // segments per page, 1..255
    uint32_t per_packet; // every audio packet ends its page
    uint32_t serial;     // track t: serial + t
    uint32_t hdr_pages;  // header pages of every track
    uint32_t native_hdr; // bytes before the first frame in the staged native image
    uint64_t hdr_bytes;  // bytes of the header pages
};

struct OggMuxTrack {
    uint64_t out_base;  // byte of the track's image in the output (16-byte aligned)
    uint64_t src_base;  // byte of the track's native image in the staging buffer
    uint64_t page_base; // first OggMuxPage slot
    uint32_t first_pos; // as TrackInfo
    uint32_t n_frames;
};

// one audio packet (a FLAC frame), indexed by track-order position
struct OggMuxFrame {
    uint64_t slot0;    // its first lacing slot (page = slot / S)
    uint64_t segpref;  // lacing values of the track's packets before it
    uint64_t gran;     // PCM frames up to and including it
    uint32_t bytepref; // frame bytes before it (FrameDesc.out_off)
    uint32_t bytes;
};

struct OggMuxOut {
    uint64_t bytes; // the track's whole image
    uint32_t pages; // audio pages
    uint32_t pad;
};

struct OggMuxPage {
    uint64_t off;  // byte of the page in the output
    uint64_t src;  // byte of its body in the staging buffer (audio pages)
    uint32_t size; // 27 + nseg + body
    uint32_t nseg;
};

hipError_t launch_ogg_mux_plan(const OggMuxParams &mp, const OggMuxTrack *tracks,
                               const uint32_t *order, const FrameDesc *fd,
                               const FrameInfo *frames, OggMuxFrame *fr, uint64_t *pgoff,
                               OggMuxOut *outs, hipStream_t s);
// hp: (offset, size) of every header page in the template `tmpl`
hipError_t launch_ogg_mux_headers(const OggMuxParams &mp, const OggMuxTrack *tracks,
                                  const uint32_t *hp, const uint8_t *tmpl, const uint8_t *stage,
                                  uint8_t *out, OggMuxPage *pages, hipStream_t s);
// max_audio_pages: an upper bound on any track's audio pages (sizes the grid)
hipError_t launch_ogg_mux_pages(const OggMuxParams &mp, const OggMuxTrack *tracks,
                                const OggMuxFrame *fr, const OggMuxOut *outs, uint8_t *out,
                                OggMuxPage *pages, uint64_t max_audio_pages, hipStream_t s);
hipError_t launch_ogg_mux_split(const OggMuxParams &mp, const OggMuxTrack *tracks,
                                const OggMuxOut *outs, const OggMuxPage *pages,
                                const uint8_t *stage, uint8_t *out, uint64_t max_audio_pages,
                                hipStream_t s);
// crc_tab / adv: ogg_crc_tables() of ogg_demux.hip
hipError_t launch_ogg_mux_crc(const OggMuxParams &mp, const OggMuxTrack *tracks,
                              const OggMuxOut *outs, const OggMuxPage *pages,
                              const uint32_t *crc_tab, const uint32_t *adv, uint8_t *out,
                              uint64_t max_audio_pages, hipStream_t s);
