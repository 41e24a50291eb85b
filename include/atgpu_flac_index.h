/* atgpu_flac_index.h — the FLAC frame index block of the libatgpu C ABI
 * (included by atgpu.h): the frame starts inside byte ranges of FLAC frame
 * data, found on the device (csrc/flac_index.hip).  A FLAC stream carries no
 * per-frame table; this makes one, so a window of a long file can start at
 * the frame that holds it.  Stateless: no handle.
 *
 * Which starts are listed.  A position p of a range is listed when
 *   - a frame header parses at p, passes its CRC-8 and agrees with the
 *     range's STREAMINFO (sample rate, channels, bits per sample, block size
 *     <= max_block_size: the checks the decoder makes), header inside the
 *     range;
 *   - for some later such header q of the range, or q = the range's end,
 *     with 9 <= q - p <= the frame bound below, the bytes [p, q) leave a zero
 *     CRC-16 residue;
 *   - where q is a header, it has p's blocking strategy and its number
 *     follows p's: frame number + 1, or sample number + p's block size.
 * The frame bound is min(2^22, 64 + 2 * channels * (ceil(max_block_size *
 * (bits_per_sample + 1) / 8) + 8)) bytes, twice what a frame of verbatim
 * subframes takes.
 *
 * The index promises starts, never lengths: a frame cut by either end of its
 * range is not listed, a frame followed by junk may be.
 */
#ifndef ATGPU_FLAC_INDEX_H
#define ATGPU_FLAC_INDEX_H

#include "atgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint64_t data_offset, data_bytes; /* byte range in the buffer, any alignment */
    uint32_t sample_rate, channels, bits_per_sample, max_block_size; /* STREAMINFO */
    uint32_t min_block_size, reserved;
} atg_flac_index_range;

typedef struct {
    uint64_t byte_offset;  /* from the range's start */
    uint64_t first_sample; /* from the header: the sample number, or the frame
                              number x the STREAMINFO block size (min_block_size,
                              max_block_size where that is 0) for fixed blocking */
    uint32_t block_size, range;
} atg_flac_index_entry;

const char *atg_flac_index_last_error(void);

/* Every range in one call.  d_data holds len bytes (its allocation reaches
   the next multiple of 4); ranges may overlap.  The entries come back in host
   memory sorted by (range, byte_offset), *n_entries their number.  When
   entry_cap is less, the call returns ATG_ERR_CAPACITY with the number needed
   in *n_entries and writes no entry.
   Checked before any GPU call, ATG_ERR_INVALID: ranges NULL with n_ranges >
   0; n_entries NULL; entries NULL with entry_cap > 0; d_data NULL with bytes
   to scan; d_data off a 4-byte boundary; a range that passes len; channels
   outside 1..8; bits_per_sample outside 4..32; max_block_size outside
   1..65535; min_block_size above max_block_size; reserved != 0.
   ATG_ERR_UNSUPPORTED: 2^40 bytes of ranges or more.  Nothing is launched
   when no range holds 9 bytes.  The device is the one that holds d_data.
   `stream` is a hipStream_t (NULL = default stream); it is synchronised
   before the call returns. */
atg_status atg_flac_index_device(const void *d_data, uint64_t len,
                                 const atg_flac_index_range *ranges, uint32_t n_ranges,
                                 atg_flac_index_entry *entries, uint64_t entry_cap,
                                 uint64_t *n_entries, void *stream);

/* The same from host memory: the bytes the ranges cover are staged on
   `device` for the call. */
atg_status atg_flac_index_host(int device, const uint8_t *data, uint64_t len,
                               const atg_flac_index_range *ranges, uint32_t n_ranges,
                               atg_flac_index_entry *entries, uint64_t entry_cap,
                               uint64_t *n_entries);

/* Names ("sync", "header", "confirm") and milliseconds of the calling
   thread's last call (its last run, where a capacity overflow made it run
   twice); returns the number of entries written, 0 before any launch. */
int atg_flac_index_kernel_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif
#endif
