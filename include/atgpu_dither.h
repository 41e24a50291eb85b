/* atgpu_dither.h — the dither block of the libatgpu C ABI (included by
 * atgpu.h): the dither bits of a batch conversion made where they are used
 * (csrc/dither.hip).  Stateless like the converter chain: no handle.
 *
 * The source is counter based, so any byte of any stream stands alone:
 * Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2,
 * 3", SC11) with the multipliers 0xD2511F53 and 0xCD9E8D57 and the key
 * increments 0x9E3779B9 and 0xBB67AE85.  With b = j / 16, byte j of stream s
 * under the 64-bit seed is byte j % 16 of the four output words c0..c3, each
 * little endian, of
 *   Philox(counter = (lo32(b), hi32(b), lo32(s), hi32(s)),
 *          key     = (lo32(seed), hi32(seed))).
 * A block is the 16 bytes of one counter value.
 */
#ifndef ATGPU_DITHER_H
#define ATGPU_DITHER_H

#include "atgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One run: blocks first_block .. first_block + blocks - 1 of stream `stream`
   to the 16 * blocks bytes at d_out + byte_offset. */
typedef struct {
    uint64_t stream;
    uint64_t first_block;
    uint64_t blocks;
    uint64_t byte_offset; /* on a 16-byte boundary */
} atg_dither_run;

const char *atg_dither_last_error(void);

/* Every run in one launch; d_out holds out_cap bytes.  Each block is written
   by one lane in one 16-byte store, and nothing outside the runs is written.
   Checked before any GPU call, ATG_ERR_INVALID: runs NULL with n_runs > 0;
   d_out NULL with blocks to write; d_out or a byte_offset off a 16-byte
   boundary; first_block + blocks past 2^64; runs whose outputs overlap.
   ATG_ERR_CAPACITY: a run that passes out_cap.  ATG_ERR_UNSUPPORTED: more
   than 2^31 - 1 tiles (atg_dither_tile_blocks) in one call.  Nothing is
   launched for n_runs == 0 or when every run has blocks == 0.  The device is
   the one that holds d_out.  `stream` is a hipStream_t (NULL = default
   stream); it is synchronised before the call returns. */
atg_status atg_dither_fill_device(const atg_dither_run *runs, uint32_t n_runs, uint64_t seed,
                                  void *d_out, uint64_t out_cap, void *stream);

/* Blocks one workgroup writes (tests place run lengths around it). */
uint32_t atg_dither_tile_blocks(void);

/* Name ("fill") and milliseconds of the calling thread's last launch;
   returns the number of entries written, 0 before any launch. */
int atg_dither_kernel_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif
#endif
