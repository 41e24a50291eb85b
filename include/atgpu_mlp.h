/* atgpu_mlp.h — the MLP block of the libatgpu C ABI (included by atgpu.h):
 * DVD-Audio titles whose codec is MLP (Meridian Lossless Packing, codec id
 * 0xA1) decoded on the GPU (csrc/mlp_decode.hip).  Stateless like the AOB
 * block of atgpu_dvda.h, whose title table (atg_aob_title) and sector records
 * it shares.
 *
 * atg_aob_scan_device and atg_aob_decode_device answer ATG_DVDA_MLP for such
 * a title.  Since this block exists that status means "decode it with the MLP
 * calls below": they take the same titles and give PCM of the same layout.
 *
 * The rules are those of the reference's src/decoders/mlp.c, driven as its
 * src/decoders/aob.c drives it: the title's attributes come from the major
 * sync at byte 4 of the first sector's payload; the payloads of the sectors
 * before the first bad one are one stream of access units (a 4-byte header
 * `4p 12u 16p`, length in 16-bit words); the reference reads a sector, then
 * decodes every whole access unit it holds, and on an error drops what that
 * call decoded.  So a title that fails at access unit f delivers the frames
 * of the access units whose last byte lies in a sector before the one in
 * which unit f ends; a partial last unit is not decoded.
 *
 * Where the reference reads filter state it never wrote (a filter order above
 * the state's length: it indexes before its array) the missing state is 0.
 *
 * Limits, ATG_MLP_UNSUPPORTED, found on the device: the reference runs into
 * undefined behaviour or never returns on these.
 *   - an access unit length field below 2 words;
 *   - no complete major sync in the first access unit;
 *   - more than ATG_MLP_MAX_UNIT_FRAMES frames in one access unit;
 *   - a substream whose first block of the title has no restart header;
 *   - max_matrix_channel above 5, more than 6 matrices, a negative output
 *     shift, a matrix added in a later block of an access unit;
 *   - channel ranges of the restart headers that do not tile 0 ..
 *     max_matrix_channel (substream 0 from 0; the last substream up to its
 *     max_matrix_channel, starting where substream 0 ends), that leave
 *     max_matrix_channel + 1 below the title's channel count, or that change
 *     at a later restart header;
 *   - the two substreams of an access unit giving different frame counts;
 *   - 20 bit, a bits or rate code that maps to 0, an assignment above 20.
 */
#ifndef ATGPU_MLP_H
#define ATGPU_MLP_H

#include "atgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATG_MLP_MAX_UNIT_FRAMES 4096u

/* atg_mlp_result.status, atg_mlp_unit.status */
enum {
    ATG_MLP_OK = 0,
    ATG_MLP_NOT_MLP = 1,            /* first sector's codec id is not 0xA1     */
    ATG_MLP_NO_MAJOR_SYNC = 2,      /* no F8726F BB at byte 4 of the first      */
                                    /* payload, or fewer than 18 bytes in it    */
    ATG_MLP_BAD_SECTOR = 3,         /* stopped at bad sector `stop_sector`      */
    ATG_MLP_EOF = 4,                /* a title of no sectors                    */
    ATG_MLP_IO_ERROR = 5,           /* one per value of the reference's         */
    ATG_MLP_INVALID_MAJOR_SYNC = 6, /* mlp_status from here on                  */
    ATG_MLP_INVALID_EXTRAWORD = 7,
    ATG_MLP_INVALID_RESTART_HEADER = 8,
    ATG_MLP_INVALID_DECODING_PARAMETERS = 9,
    ATG_MLP_INVALID_MATRIX_PARAMETERS = 10,
    ATG_MLP_INVALID_CHANNEL_PARAMETERS = 11,
    ATG_MLP_INVALID_BLOCK_DATA = 12,
    ATG_MLP_INVALID_FILTER_PARAMETERS = 13,
    ATG_MLP_PARITY_MISMATCH = 14,
    ATG_MLP_CRC8_MISMATCH = 15,
    ATG_MLP_UNSUPPORTED = 16        /* one of the limits above                  */
};

/* stop_sector: the sector in which the failing access unit ends, the first
   bad sector for ATG_MLP_BAD_SECTOR, n_sectors for ATG_MLP_OK.  stop_unit:
   the access unit that failed, access_units when none did.  access_units:
   the whole access units of the stream.  good_frames and sample_offset as in
   atg_aob_result.  A title whose status is NOT_MLP, NO_MAJOR_SYNC, EOF,
   BAD_SECTOR with stop_sector 0, or UNSUPPORTED with no access_units has no
   frames. */
typedef struct {
    int32_t status; /* ATG_MLP_* */
    uint32_t stop_sector;
    uint32_t stop_unit;
    uint32_t access_units;
    uint32_t sample_rate, bits_per_sample, channels, channel_mask, channel_assignment;
    uint32_t substreams;
    uint64_t good_frames;
    uint64_t sample_offset;
} atg_mlp_result;

/* One record per whole access unit (the unit walk).  flags: bit 0 a major
   sync is present, bit 1 it equals the title's first.  substream_flags: bit 0
   extraword, bit 1 check data, bit 2 the substream's first block opens with a
   restart header.  substream_end: the info's value * 2, from data_start.
   status: what the unit's own header says (OK, IO_ERROR, INVALID_MAJOR_SYNC,
   INVALID_EXTRAWORD, UNSUPPORTED). */
typedef struct {
    uint64_t offset;      /* of the unit's header in the title's payload stream */
    uint32_t end_sector;  /* the title's sector that holds the unit's last byte */
    uint16_t size;        /* bytes, the 4-byte header included                  */
    uint16_t data_start;  /* of substream 0, from the unit's header             */
    uint16_t substream_end[2];
    uint8_t substream_flags[2];
    uint8_t flags;
    uint8_t status;
    uint8_t reserved[8];
} atg_mlp_unit;

const char *atg_mlp_last_error(void);

/* Every pass but the ones that write PCM, over d_bytes (device memory):
   fills results[i] for every title, sample_offset laid out for `format` from
   0 upwards, and *total_samples (may be NULL) with the output capacity a
   decode needs.  units (host memory, may be NULL) receives the access-unit
   table, the titles' units in order (results[i].access_units each),
   units_cap records at the most (ATG_ERR_CAPACITY when it is too small, with
   the results filled).  The memory contract and the checks before any GPU
   call are those of atg_aob_scan_device: the kernels read bytes of a title's
   own sectors only. */
atg_status atg_mlp_scan_device(const void *d_bytes, uint64_t bytes_cap,
                               const atg_aob_title *titles, uint32_t n_titles,
                               atg_pcm_format format, atg_mlp_result *results,
                               uint64_t *total_samples, atg_mlp_unit *units,
                               uint64_t units_cap, void *stream);

/* All passes: every title's PCM into d_pcm (device memory, 16-byte aligned),
   interleaved int16 (ATG_PCM_S16, 16-bit titles only) or int32, RIFF WAVE
   channel order, at results[i].sample_offset (a multiple of 16 /
   sizeof(sample)).  Only the titles' own sample ranges are written.
   ATG_ERR_CAPACITY when pcm_cap_samples is too small (results are filled, so
   the caller can size the buffer); ATG_ERR_INVALID for ATG_PCM_S16 with a
   24-bit title in the batch. */
atg_status atg_mlp_decode_device(const void *d_bytes, uint64_t bytes_cap,
                                 const atg_aob_title *titles, uint32_t n_titles, void *d_pcm,
                                 atg_pcm_format format, uint64_t pcm_cap_samples,
                                 atg_mlp_result *results, void *stream);

/* The same for host buffers of any alignment, staged through `device`. */
atg_status atg_mlp_decode_host(int device, const void *bytes, uint64_t n_bytes,
                               const atg_aob_title *titles, uint32_t n_titles, void *pcm,
                               atg_pcm_format format, uint64_t pcm_cap_samples,
                               atg_mlp_result *results);

/* Names and milliseconds of the calling thread's last call's passes
   ("sectors", "layout", "gather", "walk", "check", "parse", "resolve",
   "store", "filter", "output"); returns the number written, 0 before any. */
int atg_mlp_kernel_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif
#endif
