/* atgpu_dvda.h — the DVD-Audio block of the libatgpu C ABI (included by
 * atgpu.h): AOB sector demux and the packed-PCM codec on the GPU
 * (csrc/aob_decode.hip).  Stateless like the packed-PCM block: no handle.
 *
 * An AOB file is a run of independent 2048-byte sectors.  A sector starts
 * with an MPEG pack header and is tiled exactly by PES packets; the
 * private-stream-1 packets (0xBD) carry the audio.  A title is a range of
 * sectors; its payload stream is the payloads of its sectors end to end, and
 * the PCM codec (codec id 0xA0) is a fixed byte permutation over chunks of
 * two frames of that stream.  MLP (0xA1) is recognised and not decoded; it
 * will read the per-sector payload table that atg_aob_scan_device returns.
 *
 * The rules are those of the reference's src/decoders/aob.c and aobpcm.c:
 * the sector's payload is that of its last 0xBD packet, the title's
 * attributes are those of its first sector alone, and a title runs until a
 * bad sector or the end of the sectors given.
 */
#ifndef ATGPU_DVDA_H
#define ATGPU_DVDA_H

#include "atgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATG_AOB_SECTOR_BYTES 2048u
/* limits, checked before any GPU call (ATG_ERR_UNSUPPORTED) */
#define ATG_AOB_MAX_TITLE_SECTORS (1u << 23) /* 16 GiB, above nine 1 GiB AOBs */
#define ATG_AOB_MAX_BATCH_BYTES (1ull << 38)
#define ATG_AOB_MAX_TITLES (1u << 20)

/* atg_aob_result.status */
enum {
    ATG_DVDA_OK = 0,            /* every sector walked; the title decoded      */
    ATG_DVDA_BAD_SECTOR = 1,    /* stopped at bad sector `stop_sector`         */
    ATG_DVDA_EOF = 2,           /* the sectors ended: a title of no sectors    */
    ATG_DVDA_UNKNOWN_CODEC = 3, /* first sector's codec id not 0xA0 / 0xA1     */
    ATG_DVDA_MLP = 4,           /* first sector is 0xA1: not decoded yet       */
    ATG_DVDA_UNSUPPORTED = 5    /* 20 bit, a bits or rate code that maps to 0, */
                                /* or a channel assignment above 20           */
};

/* atg_aob_sector.status: 0, or why the sector is bad */
enum {
    ATG_AOB_SECTOR_OK = 0,
    ATG_AOB_SECTOR_SYNC = 1,         /* pack header sync is not 0x000001BA     */
    ATG_AOB_SECTOR_MARKER = 2,       /* one of the six marker fields           */
    ATG_AOB_SECTOR_SHORT = 3,        /* fewer than 6 bytes left for a packet   */
    ATG_AOB_SECTOR_START_CODE = 4,   /* packet start code is not 0x000001      */
    ATG_AOB_SECTOR_PACKET_END = 5,   /* a packet passes the sector's end       */
    ATG_AOB_SECTOR_AUDIO_HEADER = 6, /* audio header passes the end, pad2 < 9  */
    ATG_AOB_SECTOR_NEGATIVE = 7,     /* packet shorter than its audio header   */
    ATG_AOB_SECTOR_NO_AUDIO = 8      /* no 0xBD packet                         */
};

/* One title: n_sectors sectors from byte `byte_offset` of the byte buffer.
   byte_offset must be a multiple of 16. */
typedef struct {
    uint64_t byte_offset;
    uint32_t n_sectors;
    uint32_t reserved;
} atg_aob_title;

/* One record per sector (the sector pass).  A bad sector's other fields are
   0.  codec_id is that of the sector's last 0xBD packet, whose payload is
   the sector's; the three PCM header fields are those of its last 0xA0
   packet (0 without one). */
typedef struct {
    uint16_t payload_offset; /* within the sector */
    uint16_t payload_length;
    uint8_t status;          /* ATG_AOB_SECTOR_* */
    uint8_t codec_id;
    uint8_t group_1_bps, group_1_rate, channel_assignment;
    uint8_t reserved[7];
} atg_aob_sector;

/* stop_sector: the first bad sector, or n_sectors when every sector walked.
   good_frames = 2 * floor(payload bytes before stop_sector / chunk), chunk =
   bits_per_sample / 8 * channels * 2.  sample_offset: where the title's
   good_frames * channels samples start in the output (a multiple of
   16 / sizeof(sample); filled by the decode calls, and by the scan for
   `format`).  A title whose status is neither OK nor BAD_SECTOR with
   stop_sector > 0 has no attributes and no frames. */
typedef struct {
    int32_t status; /* ATG_DVDA_* */
    uint32_t stop_sector;
    uint32_t sample_rate, bits_per_sample, channels, channel_mask, channel_assignment;
    uint32_t reserved;
    uint64_t good_frames;
    uint64_t sample_offset;
} atg_aob_result;

const char *atg_aob_last_error(void);

/* Sector and layout passes over d_bytes (device memory): fills results[i]
   for every title, sample_offset laid out for `format` from 0 upwards, and
   *total_samples (may be NULL) with the output capacity a decode needs.
   sectors (host memory, may be NULL) receives the sector table, the titles'
   sectors in order, sectors_cap records at the most (ATG_ERR_CAPACITY when
   it is too small).
   Memory contract: d_bytes must be 16-byte aligned; the kernels read bytes
   of a title's own sectors only, [byte_offset, byte_offset + 2048 *
   n_sectors), which must lie inside bytes_cap: the sector pass reads single
   bytes, the PCM pass whole aligned 16-byte units of a sector that hold
   payload.  Titles may overlap.
   Checked before any GPU call, ATG_ERR_INVALID: NULL arrays with n_titles >
   0, a misaligned buffer or byte_offset, an unknown format;
   ATG_ERR_CAPACITY: a title that passes bytes_cap; ATG_ERR_UNSUPPORTED: one
   of the limits above.  `stream` is a hipStream_t (NULL = default stream); it
   is synchronised before the call returns. */
atg_status atg_aob_scan_device(const void *d_bytes, uint64_t bytes_cap,
                               const atg_aob_title *titles, uint32_t n_titles,
                               atg_pcm_format format, atg_aob_result *results,
                               uint64_t *total_samples, atg_aob_sector *sectors,
                               uint64_t sectors_cap, void *stream);

/* All three passes: every title's PCM into d_pcm (device memory, 16-byte
   aligned), interleaved int16 (ATG_PCM_S16, 16-bit titles only) or int32,
   at results[i].sample_offset.  The kernel writes only the titles' own
   sample ranges, in 16-byte groups.  ATG_ERR_CAPACITY when pcm_cap_samples
   is too small (results are filled, so the caller can size the buffer);
   ATG_ERR_INVALID for ATG_PCM_S16 with a 24-bit title in the batch.  The
   other checks are those of atg_aob_scan_device. */
atg_status atg_aob_decode_device(const void *d_bytes, uint64_t bytes_cap,
                                 const atg_aob_title *titles, uint32_t n_titles, void *d_pcm,
                                 atg_pcm_format format, uint64_t pcm_cap_samples,
                                 atg_aob_result *results, void *stream);

/* The same for host buffers of any alignment, staged through `device`. */
atg_status atg_aob_decode_host(int device, const void *bytes, uint64_t n_bytes,
                               const atg_aob_title *titles, uint32_t n_titles, void *pcm,
                               atg_pcm_format format, uint64_t pcm_cap_samples,
                               atg_aob_result *results);

/* PCM frames per tile of the PCM pass (tests place title lengths round it). */
uint32_t atg_aob_tile_frames(void);

/* Names and milliseconds of the calling thread's last call's passes
   ("sectors", "layout", "pcm"); returns the number written, 0 before any. */
int atg_aob_kernel_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif
#endif
