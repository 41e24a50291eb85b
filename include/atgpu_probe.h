/* atgpu_probe.h — test probes of the libatgpu C ABI (included by atgpu.h):
 * entries that run one production kernel of the FLAC encoder alone and hand
 * back an intermediate result the encoder itself never exposes, so a test can
 * check it directly.  They are for tests; nothing in the product calls them.
 */
#ifndef ATGPU_PROBE_H
#define ATGPU_PROBE_H

#include "atgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Run the encoder's LPC analysis kernel alone (the production kernel with its
   probe pointer set, not a copy) on a batch of host PCM and return its raw
   autocorrelation sums, before Levinson-Durbin.  Tracks, options, channels
   and bits_per_sample as atg_flac_encode_host; the engine must be idle.
   sums: (max_lpc_order + 1) doubles per (frame, candidate), frames in track
   order (all of track 0's, then track 1's, ...), candidates as the encoder
   numbers them (channel c; with mid/side: left, right, mid, side);
   sums_cap counts doubles.  Frames too short for LPC (n <= max_lpc_order + 1)
   give zeros.  window (may be NULL): receives the window_n doubles of the
   window table the kernel read for frames of window_n samples, copied back
   from device memory; ATG_ERR_INVALID when no frame of that length has been
   analysed on this engine.  Errors are reported by atg_last_error. */
atg_status atg_flac_lpc_probe_host(atg_engine *eng, const atg_flac_options *opts,
                                   const void *pcm, atg_pcm_format format,
                                   const atg_track *tracks, uint32_t n_tracks,
                                   uint32_t channels, uint32_t bits_per_sample,
                                   double *sums, uint64_t sums_cap, uint32_t window_n,
                                   double *window);

#ifdef __cplusplus
}
#endif
#endif
