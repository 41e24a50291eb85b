/* atgpu_tensor.h — the tensor block of the libatgpu C ABI (included by
 * atgpu.h): the library's PCM rows to and from what a tensor program holds
 * (csrc/pcm_tensor.hip).  Stateless like the converter chain: no handle.
 *
 * The PCM side is what the decoders, the chain and the encoders use: ragged
 * rows of channel-interleaved int16 or int32 samples.  The tensor side is a
 * buffer of one element type in which a row is `channels` runs of frames,
 * channel c's run starting channel_stride elements after channel c-1's: a
 * row of a padded, planar [batch, channels, frames] tensor, or of any slice
 * of one whose last stride is 1.
 *
 * The arithmetic is the reference's (src/pcm.c): FrameList.to_float() is
 * sample / 2^(bits-1) (:599-615), FloatFrameList.to_int(bits) is
 * (int)(x * 2^(bits-1)) clamped to the width (:1198-1227), with the cast an
 * x86-64 build performs (cvttsd2si).
 */
#ifndef ATGPU_TENSOR_H
#define ATGPU_TENSOR_H

#include "atgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* element type of the tensor side, one per call */
typedef enum {
    ATG_TENSOR_F16 = 0, /* IEEE binary16 */
    ATG_TENSOR_F32 = 1,
    ATG_TENSOR_F64 = 2,
    ATG_TENSOR_I32 = 3 /* the samples themselves, unscaled */
} atg_tensor_dtype;

/* PCM -> tensor, one row.  src is read as atg_pcm_view describes a source:
   src_frames frames of `channels` channels from sample_offset on
   (window_offset must be 0); src_frames is the row's length.  With E the
   element index out_offset + c * channel_stride, channel c's run receives
   value(frame i, channel c) at E + i for i < src_frames and exact zeros for
   src_frames <= i < pad_frames.  Nothing else is written.  The value of a
   sample s of bits_per_sample bits:
     ATG_TENSOR_F64  (double)s / 2^(bits-1)
     ATG_TENSOR_F32  that double rounded to nearest even
     ATG_TENSOR_F16  the float32 rounded to nearest even, subnormals kept
                     (16-bit sample 1 is the subnormal 2^-15)
     ATG_TENSOR_I32  s
   For samples inside the row's bits_per_sample range every float value is
   one exact-or-nearest-even step; samples outside it in an int32 container
   are outside the contract. */
typedef struct {
    atg_pcm_view src;
    uint32_t channels;        /* 1..8 */
    uint32_t bits_per_sample; /* 1..24 */
    uint64_t pad_frames;      /* >= src.src_frames */
    uint64_t out_offset;      /* element index of channel 0's run */
    uint64_t channel_stride;  /* >= pad_frames, elements between channel runs */
} atg_pcm_to_tensor_row;

/* tensor -> PCM, one row: `frames` frames of `channels` runs from element
   in_offset on, channel_stride elements apart, to the frames * channels
   interleaved samples from index out_offset of the call's PCM output.  A
   float element x is widened exactly to double, multiplied by 2^(bits-1) and
   converted as cvttsd2si converts: truncation toward zero, INT_MIN for NaN,
   +-inf and anything outside int32; the result is clamped to
   [-2^(bits-1), 2^(bits-1) - 1].  NaN and +inf so give the most negative
   sample, as the reference's cast does.  An int32 element is clamped only. */
typedef struct {
    uint64_t in_offset;
    uint64_t channel_stride;  /* >= frames */
    uint64_t frames;
    uint32_t channels;        /* 1..8 */
    uint32_t bits_per_sample; /* 1..24 */
    uint64_t out_offset;      /* on a 16-byte boundary of the PCM output */
} atg_pcm_from_tensor_row;

const char *atg_pcm_tensor_last_error(void);

/* Every row in one launch; d_out holds out_cap_elems elements of `dtype`.
   Memory contract: the PCM side is read only in aligned 16-byte units that
   hold at least one sample of some row, so sources need only be aligned to
   their sample size; d_out needs alignment to its element size only and a
   channel run may start at any element: its 16-byte-aligned interior is
   written in 16-byte stores, its two ends element by element.
   Checked before any GPU call, ATG_ERR_INVALID: rows NULL with n_rows > 0;
   d_out NULL with elements to write; a source pointer NULL with frames or
   off its sample size; an unknown source format or dtype; window_offset !=
   0; channels outside 1..8; bits_per_sample outside 1..24; pad_frames <
   src_frames; channel_stride < pad_frames; d_out off its element size; a
   size or offset at or above 2^59; channel runs that overlap, of one row or
   of two.  ATG_ERR_CAPACITY: a run that passes out_cap_elems.  Nothing is
   launched for n_rows == 0 or when every row has pad_frames == 0; a row of
   src_frames == 0 and pad_frames > 0 is zero-filled.  The device is the one
   that holds d_out.  `stream` is a hipStream_t (NULL = default stream); it
   is synchronised before the call returns. */
atg_status atg_pcm_to_tensor_device(const atg_pcm_to_tensor_row *rows, uint32_t n_rows,
                                    void *d_out, atg_tensor_dtype dtype, uint64_t out_cap_elems,
                                    void *stream);

/* The way back; d_in holds in_cap_elems elements of `dtype`, d_out is
   interleaved int16 (ATG_PCM_S16, rows of at most 16 bits) or int32.
   Memory contract: d_in is read in 16-byte loads over a run's aligned
   interior and element by element at its ends, never outside a run; d_out is
   written as atg_pcm_chain_device writes it, so it must be 16-byte aligned
   and every out_offset a multiple of 16 / sizeof(sample).
   ATG_ERR_INVALID, before any GPU call: rows, d_in or d_out NULL with
   samples to convert; an unknown dtype or output format; channels outside
   1..8; bits_per_sample outside 1..24; channel_stride < frames; ATG_PCM_S16
   for a row of more than 16 bits; d_in off its element size; a misaligned
   d_out or out_offset; a size or offset at or above 2^59; output rows that
   overlap.  ATG_ERR_CAPACITY: an input run that passes in_cap_elems or an
   output range that passes out_cap_samples.  Nothing is launched for n_rows
   == 0 or when every row has frames == 0. */
atg_status atg_pcm_from_tensor_device(const atg_pcm_from_tensor_row *rows, uint32_t n_rows,
                                      const void *d_in, atg_tensor_dtype dtype,
                                      uint64_t in_cap_elems, void *d_out,
                                      atg_pcm_format out_format, uint64_t out_cap_samples,
                                      void *stream);

/* Frames per tile, whatever the channel count (tests place lengths around
   it). */
uint32_t atg_pcm_tensor_tile_frames(void);

/* Name ("to_tensor" or "from_tensor") and milliseconds of the calling
   thread's last launch; returns the number of entries written, 0 before any
   launch. */
int atg_pcm_tensor_kernel_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif
#endif
