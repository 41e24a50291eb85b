/*
 * atgpu.h — C ABI of libatgpu, the MI355X (gfx950) batch FLAC encoder.
 *
 * This is the drop-in boundary for python-audio-tools' FLAC encode hot path.
 * The reference binds the encoder through its CPython-2 extension
 * `audiotools.encoders.encode_flac` (reference src/encoders/flac.c:44-121,
 * registered at src/encoders.h:65-67); that function pulls PCM from a
 * PCMReader (src/pcmconv.c:207-329), encodes frame by frame
 * (src/encoders/flac.c:240-274) and returns [(byte_offset, pcm_frames)].
 * The entry points below replace the body of that function (and of the
 * frame loop) for a whole batch of tracks at once; the Python-visible
 * `encode_flac` in python-audio-tools_amd/audiotools/encoders.py keeps the
 * reference's signature and error behaviour and calls into this ABI.
 *
 * Plain C types only.  No exceptions cross the ABI: every entry point
 * returns an atg_status; atg_last_error() describes the most recent failure
 * on the calling thread.
 */
#ifndef ATGPU_H
#define ATGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ATG_ABI_VERSION 11

typedef enum {
    ATG_OK = 0,
    ATG_ERR_INVALID = -1,     /* bad argument (maps to ValueError) */
    ATG_ERR_UNSUPPORTED = -2, /* option combination not supported on GPU */
    ATG_ERR_DEVICE = -3,      /* HIP runtime failure */
    ATG_ERR_NOMEM = -4,       /* device or host allocation failed */
    ATG_ERR_CAPACITY = -5     /* caller output buffer too small */
} atg_status;

/* Encoder options: the keyword arguments of encode_flac
   (reference src/encoders/flac.c:52-67; struct flac_encoding_options,
   src/encoders/flac.h:30-55).  Derived options (QLP precision, maximum Rice
   parameter) are computed inside, as the reference does (flac.c:164-184). */
typedef struct {
    uint32_t block_size;
    uint32_t max_lpc_order;
    uint32_t min_residual_partition_order; /* accepted; unused, as reference */
    uint32_t max_residual_partition_order;
    int32_t mid_side;
    int32_t adaptive_mid_side;
    int32_t exhaustive_model_search;
    int32_t disable_verbatim_subframes;
    int32_t disable_constant_subframes;
    int32_t disable_fixed_subframes;
    int32_t disable_lpc_subframes;
    uint32_t padding_size;
} atg_flac_options;

/* PCM sample containers the engine reads. */
typedef enum {
    ATG_PCM_S16 = 0, /* interleaved int16 (bits_per_sample <= 16) */
    ATG_PCM_S32 = 1  /* interleaved int32 (any bits_per_sample <= 24), the
                        reference FrameList layout (src/pcm.h:40-54) */
} atg_pcm_format;

/* One track of a batch: a contiguous run of interleaved PCM frames.
   By default the track is cut into block_size frames plus a shorter last
   one (what BufferedPCMReader feeds the reference encoder,
   audiotools/__init__.py:2561-2606).  When frame_sizes is non-NULL the
   track is cut exactly as listed instead (the reference encodes whatever
   each pcmreader.read(block_size) call returns as one frame,
   src/encoders/flac.c:244-274); sizes must sum to pcm_frames and each be
   1..65535 (frames above 4096 samples take the large-frame kernels). */
typedef struct {
    uint64_t pcm_offset; /* index of the track's first PCM frame */
    uint64_t pcm_frames; /* number of PCM frames (samples per channel) */
    const uint32_t *frame_sizes; /* optional explicit frame lengths */
    uint64_t n_frame_sizes;
} atg_track;

/* Per-track result.  `bytes` is the length of the complete .flac image
   (stream marker, STREAMINFO, VORBIS_COMMENT, PADDING, frames) written at
   out + out_offset.  frame_offsets[] (caller array indexed by
   first_frame .. first_frame+n_frames-1) hold each frame's byte offset from
   the first frame, as encode_flac's return list does (flac.c:249-253). */
typedef struct {
    uint64_t out_offset;
    uint64_t bytes;
    uint32_t first_frame;
    uint32_t n_frames;
    uint32_t min_frame_bytes;
    uint32_t max_frame_bytes;
    uint8_t md5[16];
    int32_t status;
    uint32_t reserved;
} atg_track_result;

typedef struct atg_engine atg_engine;

/* Library / device management */
int atg_abi_version(void);
const char *atg_last_error(void);
atg_status atg_engine_create(int device, atg_engine **out);
/* flags for atg_engine_create_ex */
#define ATG_ENGINE_STREAMING 1u /* streams on first use: a process that only
                                   encodes one track at a time through
                                   atg_flac_encode_frames (encode_flac, one
                                   process per track under track2track -j N)
                                   then holds two HIP streams, so many such
                                   processes fit the device's hardware queues */
/* Where a device batch's STREAMINFO MD5 is computed.  By default the engine
   picks per batch: one GPU hash chain per track (md5.hip) unless the tracks
   are few and long enough that host cores hash the PCM sooner than the
   longest serial chain ends (config 5: 64 tracks x 8.6 MB of 24-bit 5.1 PCM
   -- the PCM goes to pinned host memory and host threads hash it beside the
   next batch's GPU work).  These flags force one side (the images are the
   same bytes either way). */
#define ATG_ENGINE_MD5_GPU 2u
#define ATG_ENGINE_MD5_HOST 4u
/* atg_engine_create with flags.  Without ATG_ENGINE_STREAMING every stream
   is created at once in a fixed order (the batch APIs' queue layout). */
atg_status atg_engine_create_ex(int device, uint32_t flags, atg_engine **out);
void atg_engine_destroy(atg_engine *eng);

/* Device choice for callers that do not name one (the drop-in entry points:
   encode_flac, FlacDecoder, the process-wide engines), host code only, no
   HIP call.  atg_pick_device: ATG_DEVICE, else LOCAL_RANK, else the next
   visible device of a node-wide round robin (a flock'ed counter in
   /dev/shm, per user; ATG_RR_FILE names another file), so the reference's
   one-process-per-track conversions (audiotools/__init__.py:5263-5529)
   spread over the node's GPUs.  Decided once per process (again after a
   fork).  atg_visible_devices: the entries of HIP_VISIBLE_DEVICES /
   CUDA_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES, else the GPU nodes of the KFD
   topology (ATG_DEVICE_COUNT overrides, for tests); at least 1. */
int atg_pick_device(void);
int atg_visible_devices(void);

/* Number of FLAC frames and worst-case output bytes of a batch, so callers
   can size outputs (the reference's recorders grow on demand; a batch
   engine needs bounds up front). */
atg_status atg_flac_batch_bounds(const atg_flac_options *opts,
                                 const atg_track *tracks, uint32_t n_tracks,
                                 uint32_t channels, uint32_t bits_per_sample,
                                 uint64_t *total_frames, uint64_t *out_bytes);

/* Encode a batch whose PCM and output live in host memory.
   pcm: interleaved samples in `format`; out: out_cap bytes (>= the
   atg_flac_batch_bounds size); results: n_tracks entries; frame_offsets /
   frame_pcm_frames: total_frames entries each (may be NULL).  Each track's
   image starts at results[t].out_offset; the images are packed back to back
   (16-byte aligned) from out on.  The batch runs as a pipeline of chunks of
   consecutive tracks (atg_engine_set_host_chunk_bytes), three in flight:
   chunk c+1's upload, chunk c's encode and chunk c-1's download overlap.
   Page-locked buffers (atg_host_alloc, hipHostMalloc, hipHostRegister) are
   copied by DMA directly; pageable ones through pinned staging. */
atg_status atg_flac_encode_host(atg_engine *eng, const atg_flac_options *opts,
                                const void *pcm, atg_pcm_format format,
                                const atg_track *tracks, uint32_t n_tracks,
                                uint32_t channels, uint32_t bits_per_sample,
                                uint32_t sample_rate, uint8_t *out,
                                uint64_t out_cap, atg_track_result *results,
                                uint64_t *frame_offsets,
                                uint32_t *frame_pcm_frames);

/* Asynchronous form of atg_flac_encode_host: plans the job, queues its
   chunks on the pipeline (collecting older chunks, of this or earlier jobs,
   as stages free up) and returns a ticket; pcm, out, results and the frame
   arrays must stay valid until atg_flac_encode_host_wait(ticket).  Jobs
   share the pipeline in submission order, so job k+1's uploads overlap job
   k's last chunks: back to back, the PCIe link stays busy.  Fails with
   ATG_ERR_INVALID while an atg_flac_encode_device_async batch is unwaited
   (and that call fails while a host job is in flight). */
atg_status atg_flac_encode_host_async(atg_engine *eng, const atg_flac_options *opts,
                                      const void *pcm, atg_pcm_format format,
                                      const atg_track *tracks, uint32_t n_tracks,
                                      uint32_t channels, uint32_t bits_per_sample,
                                      uint32_t sample_rate, uint8_t *out, uint64_t out_cap,
                                      atg_track_result *results, uint64_t *frame_offsets,
                                      uint32_t *frame_pcm_frames, uint64_t *ticket);
/* Wait for host job `ticket` (and the jobs before it); its results and
   images are then complete.  A job's ticket can be waited once. */
atg_status atg_flac_encode_host_wait(atg_engine *eng, uint64_t ticket);

/* Streaming form for ONE track (the reference's frame loop,
   src/encoders/flac.c:244-274, run over bounded segments of a long track):
   encodes pcm_frames PCM frames (host memory, cut into block_size frames or
   the explicit frame_sizes, as atg_track) as FLAC frames only -- no stream
   header, no MD5 -- numbered from first_frame_number (the frame header's
   UTF-8 frame number, flac.c:1531-1566).  The frames land back to back at
   out (*out_bytes in total, frame_bytes[i] each; out_cap >=
   atg_flac_max_frames_bytes).  The caller hashes the PCM (a serial MD5
   chain per track runs faster on a host core than on one GPU lane) and
   writes the stream header with atg_flac_stream_header before the first
   segment and again, with the final STREAMINFO, at the end (the reference
   rewrites STREAMINFO once the frames are written, flac.c:276-279). */
atg_status atg_flac_encode_frames(atg_engine *eng, const atg_flac_options *opts,
                                  const void *pcm, atg_pcm_format format, uint64_t pcm_frames,
                                  const uint32_t *frame_sizes, uint64_t n_frame_sizes,
                                  uint32_t channels, uint32_t bits_per_sample,
                                  uint32_t sample_rate, uint64_t first_frame_number,
                                  uint8_t *out, uint64_t out_cap, uint64_t *out_bytes,
                                  uint32_t *frame_bytes);
/* One segment of atg_flac_encode_frames_batch: PCM frames
   [pcm_offset, pcm_offset + pcm_frames) of the batch buffer, cut as
   atg_track, numbered from first_frame_number. */
typedef struct {
    uint64_t pcm_offset;
    uint64_t pcm_frames;
    const uint32_t *frame_sizes; /* NULL: block_size frames + a short last one */
    uint64_t n_frame_sizes;
    uint64_t first_frame_number;
} atg_segment;

/* atg_flac_encode_frames for many segments (of many tracks, from many
   callers) in one GPU pass: what the encoder service (atgpu-encoderd)
   runs for the encode_flac calls of concurrent processes.  Segments share
   the options and the PCM format.  Segment k's frames land at
   out + seg_offsets[k] (seg_bytes[k] bytes; offsets 16-byte aligned, packed
   in segment order; out_cap >= the sum of atg_flac_max_frames_bytes rounded
   up to 16 each); frame_bytes (may be NULL) receives every frame's size in
   segment order.  The engine's results of earlier batches are gone. */
atg_status atg_flac_encode_frames_batch(atg_engine *eng, const atg_flac_options *opts,
                                        const void *pcm, atg_pcm_format format,
                                        const atg_segment *segs, uint32_t n_segs,
                                        uint32_t channels, uint32_t bits_per_sample,
                                        uint32_t sample_rate, uint8_t *out, uint64_t out_cap,
                                        uint64_t *seg_offsets, uint64_t *seg_bytes,
                                        uint32_t *frame_bytes);
/* worst-case bytes of atg_flac_encode_frames' output (0: invalid options) */
uint64_t atg_flac_max_frames_bytes(const atg_flac_options *opts, uint64_t pcm_frames,
                                   const uint32_t *frame_sizes, uint64_t n_frame_sizes,
                                   uint32_t channels, uint32_t bits_per_sample);
/* fLaC + STREAMINFO (fields clamped as flacenc_write_streaminfo,
   flac.c:376-409) + VORBIS_COMMENT (vendor string) + PADDING of
   opts->padding_size bytes (flac.c:208-238), host-side; returns the header
   size, or 0 when cap is too small or an argument is invalid. */
uint64_t atg_flac_stream_header(const atg_flac_options *opts, uint32_t channels,
                                uint32_t bits_per_sample, uint32_t sample_rate,
                                uint64_t total_samples, uint32_t min_frame_bytes,
                                uint32_t max_frame_bytes, const uint8_t *md5, uint8_t *out,
                                uint64_t cap);

/* ------------------------------------------------------------------ */
/* Encoder service.  track2track converts every track in a fresh process */
/* (reference audiotools/__init__.py:5494-5521), and a process that      */
/* brings up its own HIP context, engine and code objects pays ~0.3-0.5 s */
/* for it.  atgpu-encoderd (beside libatgpu.so) owns one engine per GPU  */
/* and encodes the segments of every client process, batching concurrent */
/* clients' segments that share options and format into one GPU pass     */
/* (atg_flac_encode_frames_batch).  The streaming encode_flac uses it.   */
/* ------------------------------------------------------------------ */
typedef struct atg_service atg_service;
/* Connect to `device`'s service; with spawn != 0 start atgpu-encoderd when
   none listens (never from a process that has opened the GPU itself: it may
   not exec another program).  The service exits after an idle period. */
atg_status atg_service_connect(int device, int spawn, atg_service **out);
void atg_service_close(atg_service *svc);
const char *atg_service_last_error(void);
/* atg_flac_encode_frames' contract, encoded by the service */
atg_status atg_service_encode_frames(atg_service *svc, const atg_flac_options *opts,
                                     const void *pcm, atg_pcm_format format,
                                     uint64_t pcm_frames, const uint32_t *frame_sizes,
                                     uint64_t n_frame_sizes, uint32_t channels,
                                     uint32_t bits_per_sample, uint32_t sample_rate,
                                     uint64_t first_frame_number, uint8_t *out,
                                     uint64_t out_cap, uint64_t *out_bytes,
                                     uint32_t *frame_bytes);

/* PCM bytes per chunk of atg_flac_encode_host's pipeline (default 512 MiB):
   consecutive tracks are grouped into chunks of about this much PCM, and
   chunk c+1's upload, chunk c's encode and chunk c-1's download overlap. */
atg_status atg_engine_set_host_chunk_bytes(atg_engine *eng, uint64_t bytes);

/* Batches atg_flac_encode_device_async keeps in flight (slots in rotation,
   each its own device workspace, ~2 KB of tables per frame of the batch):
   3 .. 32, or 0 = automatic (the default).  Every track's MD5 is one serial
   hash (~12.5 ms per MiB of track on the GPU, whatever the batch width), so
   a narrow batch -- a rank's share of a strong-scaling job -- needs more
   batches in flight to keep the chains off its step.  From 4 on, the chains
   of all batches in flight advance together, one launch per enqueue on one
   stream, each batch's chain in n - 2 slices.  Automatic: the first device
   batch enqueued while nothing is in flight sets the depth from the ratio of
   its longest track's MD5 chain to its kernel time (12, 24 or 32; 3 when
   the chains are short or hashed on the host), and a host job sets it back
   to 3.  Lowering the depth frees the workspaces of the slots beyond it.
   Fails with ATG_ERR_INVALID while any batch or host job is unwaited. */
atg_status atg_engine_set_inflight(atg_engine *eng, uint32_t n);
/* The current depth D (the slots in rotation): a pipelined caller keeps up
   to D batches in flight and waits the oldest before enqueueing the next.
   With the automatic depth, read it after the pipeline's first enqueue. */
uint32_t atg_engine_inflight(atg_engine *eng);

/* Device-memory entry points run on the library's own non-blocking HIP
   streams: device inputs must be complete (e.g. the producing stream
   synchronized) when the call is made. */

/* Encode a batch whose PCM already lives in device memory (HBM) and leave
   the .flac images in device memory at d_out (out_cap bytes).  Results are
   copied back to host `results` (small).  Runs on the engine's streams and
   returns when the images are complete. */
atg_status atg_flac_encode_device(atg_engine *eng, const atg_flac_options *opts,
                                  const void *d_pcm, atg_pcm_format format,
                                  const atg_track *tracks, uint32_t n_tracks,
                                  uint32_t channels, uint32_t bits_per_sample,
                                  uint32_t sample_rate, void *d_out,
                                  uint64_t out_cap, atg_track_result *results);

/* The same batch encode, enqueued: returns once the work is queued, with a
   ticket for atg_flac_encode_wait.  The engine keeps D batches in flight
   (atg_engine_inflight: automatic unless atg_engine_set_inflight fixed it;
   each its own device workspace): batch k's MD5 chains and stream headers run on their own
   stream while batches k+1 .. k+D-1 are analysed, so a caller that waits
   for ticket k after enqueueing k+D-1 overlaps them.  d_pcm and d_out must
   stay untouched until the ticket is waited.  Enqueue number D+1 while D
   tickets are unwaited fails with ATG_ERR_INVALID (wait the oldest first);
   atg_flac_encode_device takes a slot too and fails the same way, and
   atg_flac_encode_host fails while any ticket is unwaited.  A waited
   ticket's results stay readable until its slot is reused D enqueues later, or
   until a streaming call (atg_flac_encode_frames[_batch]), which always
   takes slot 0. */
atg_status atg_flac_encode_device_async(atg_engine *eng, const atg_flac_options *opts,
                                        const void *d_pcm, atg_pcm_format format,
                                        const atg_track *tracks, uint32_t n_tracks,
                                        uint32_t channels, uint32_t bits_per_sample,
                                        uint32_t sample_rate, void *d_out, uint64_t out_cap,
                                        uint64_t *ticket);
/* wait for the batch of `ticket`; results as atg_flac_encode_device's */
atg_status atg_flac_encode_wait(atg_engine *eng, uint64_t ticket, atg_track_result *results);

/* Per-kernel device time of the engine's most recent encode, measured with
   HIP events recorded on the stream each kernel ran on.  names/ms arrays of
   capacity `cap`; returns the number of entries written. */
int atg_engine_kernel_times(atg_engine *eng, const char **names, float *ms, int cap);

/* Page-locked host memory: PCM and output buffers the host pipeline moves
   by DMA without staging (SURVEY 8(d)'s timer starts from pinned PCM). */
atg_status atg_host_alloc(uint64_t bytes, void **ptr);
void atg_host_free(void *ptr);

/* Device-memory helpers so callers without a GPU framework can stage data. */
atg_status atg_device_alloc(atg_engine *eng, uint64_t bytes, void **d_ptr);
atg_status atg_device_free(atg_engine *eng, void *d_ptr);
atg_status atg_copy_to_device(atg_engine *eng, void *d_dst, const void *src,
                              uint64_t bytes);
atg_status atg_copy_device(atg_engine *eng, void *d_dst, const void *d_src, uint64_t bytes);
/* Host-side gather: n host buffers (srcs[i], bytes[i]) copied back to back
   into dst on `threads` host threads (0 = the library's default, at most
   16) -- the reads of a batch of PCMReaders laid out in a (pinned) staging
   buffer in one call at memory bandwidth. */
atg_status atg_host_gather(void *dst, const void *const *srcs, const uint64_t *bytes,
                           uint64_t n, uint32_t threads);
atg_status atg_copy_to_host(atg_engine *eng, void *dst, const void *d_src,
                            uint64_t bytes);

/* ------------------------------------------------------------------ */
/* FLAC decoder (trackverify / FlacDecoder path).                     */
/* Replaces the body of the reference's audiotools.decoders.FlacDecoder */
/* (src/decoders/flac.c:28-98 init + flacdec_read_metadata :568-707,   */
/* read() :174-285 with its frame/subframe/residual readers :710-1269, */
/* offsets() :365-443, MD5 verify :446-493) for a batch of images.      */
/* ------------------------------------------------------------------ */

/* Decode status per track: the reference's flac_status values
   (src/decoders/flac.h:68-81) plus what read() raises itself. */
enum {
    ATG_FD_OK = 0, ATG_FD_ERROR = 1, ATG_FD_SYNC = 2, ATG_FD_RESERVED = 3,
    ATG_FD_BPS = 4, ATG_FD_RATE = 5, ATG_FD_HDR_CRC = 6,
    ATG_FD_RATE_MISMATCH = 7, ATG_FD_CH_MISMATCH = 8, ATG_FD_BPS_MISMATCH = 9,
    ATG_FD_MAXBS = 10, ATG_FD_CODING = 11, ATG_FD_FIXED_ORDER = 12,
    ATG_FD_SUBFRAME_TYPE = 13,
    ATG_FD_FRAME_CRC = 14, /* "invalid checksum in frame" (flac.c:251-255) */
    ATG_FD_EOF = 15,       /* IOError "EOF reading frame" (flac.c:259-264) */
    ATG_FD_MD5 = 16        /* "MD5 mismatch at end of stream" (:199-207) */
};

/* STREAMINFO and the parts of the other metadata blocks the reference
   decoder keeps (struct flac_STREAMINFO, src/decoders/flac.h:37-48). */
typedef struct {
    uint32_t min_block_size, max_block_size, min_frame_size, max_frame_size;
    uint32_t sample_rate, channels, bits_per_sample, channel_mask;
    uint64_t total_samples;
    uint8_t md5[16];
    uint64_t frames_offset; /* bytes from the image start to the first frame */
    uint32_t n_seekpoints;
    uint32_t reserved;
} atg_flac_streaminfo;

typedef struct {
    uint64_t sample_number, byte_offset;
    uint32_t samples, reserved;
} atg_flac_seekpoint;

/* flacdec_read_metadata (src/decoders/flac.c:568-707) over an in-memory
   image.  Returns 0 ok, 1 not a FLAC stream (ValueError), 2 EOF (IOError).
   Up to sp_cap SEEKTABLE points are stored into sp (may be NULL). */
int atg_flac_read_metadata(const uint8_t *data, uint64_t len, atg_flac_streaminfo *si,
                           atg_flac_seekpoint *sp, uint32_t sp_cap);

/* One stream of a decode batch: its frames occupy
   data[data_offset, data_offset + data_bytes) (data_offset = image start +
   frames_offset); the remaining fields are its STREAMINFO. */
typedef struct {
    uint64_t data_offset;
    uint64_t data_bytes;
    uint64_t total_samples;
    uint32_t sample_rate, channels, bits_per_sample, max_block_size;
    uint8_t md5[16];
} atg_flac_dec_track;

/* Per-track decode result.
   read() view (src/decoders/flac.c:174-285): the stream hands out n_frames
   FLAC frames = pcm_frames PCM frames (interleaved int32, FrameList layout,
   at PCM-frame index pcm_offset of the batch output) and then raises
   `status` (0 = end of stream with the MD5 verified); md5 = MD5 of those
   frames' little-endian PCM bytes.
   offsets() view (flac.c:365-443, which never checks CRC-16): walk_frames
   frames are walked (frame arrays first_frame .. first_frame+walk_frames-1,
   decoded PCM continuing after pcm_frames) before walk_status stops it.
   The two differ only when a frame fails its CRC-16.  walk_end = the byte
   (from the track's first frame) where the walk stopped: the frame that
   stopped it, or the end of the last frame once remaining reached 0 -- a
   streaming caller resumes a window there. */
typedef struct {
    uint64_t pcm_offset;
    uint64_t pcm_frames;
    uint32_t first_frame;
    uint32_t n_frames;
    int32_t status;
    uint32_t walk_frames;
    uint8_t md5[16];
    int32_t walk_status;
    uint32_t reserved;
    uint64_t walk_end;
} atg_flac_dec_result;

typedef struct atg_decoder atg_decoder;

atg_status atg_decoder_create(int device, atg_decoder **out);
void atg_decoder_destroy(atg_decoder *dec);
const char *atg_decoder_last_error(void);

/* Decode a batch held in host memory; the PCM stays in the decoder until
   atg_flac_decode_fetch.  total_samples = interleaved samples of the batch
   output, total_frames = FLAC frames decoded. */
atg_status atg_flac_decode_host(atg_decoder *dec, const uint8_t *data, uint64_t len,
                                const atg_flac_dec_track *tracks, uint32_t n_tracks,
                                atg_flac_dec_result *results, uint64_t *total_samples,
                                uint64_t *total_frames);

/* Copy the last decode's PCM (pcm_cap int32 samples) and, per FLAC frame,
   its byte offset from the track's first frame and its header block size
   (what FlacDecoder.offsets() reports, flac.c:365-443).  Any may be NULL. */
atg_status atg_flac_decode_fetch(atg_decoder *dec, int32_t *pcm, uint64_t pcm_cap,
                                 uint64_t *frame_offsets, uint32_t *frame_block_sizes,
                                 uint64_t frame_cap);

/* Decode a batch already in device memory (4-byte aligned, readable up to
   len rounded up to 4).  *d_pcm receives the decoder-owned device PCM
   (valid until the call after next). */
atg_status atg_flac_decode_device(atg_decoder *dec, const void *d_data, uint64_t len,
                                  const atg_flac_dec_track *tracks, uint32_t n_tracks,
                                  atg_flac_dec_result *results, const int32_t **d_pcm,
                                  uint64_t *total_samples);

/* Decode batches atg_flac_decode_device_async keeps in flight: 3 (default)
   .. 16.  A batch's STREAMINFO MD5 checks are serial hashes (~12 ms per 1 MB
   of decoded PCM whatever the batch width); from 4 on, the hashes of every
   batch in flight advance together, one launch per enqueue on one stream,
   each batch's in n - 2 slices.  Each slot holds its batch's PCM, restore
   scratch and MD5 byte image (~5 GB for a 1024-track config-2 batch);
   lowering the depth frees the slots past it.  Fails while a batch is
   unwaited; the last waited batch's buffers are no longer fetchable
   afterwards. */
atg_status atg_decoder_set_inflight(atg_decoder *dec, uint32_t n);

/* The parse's frame-end hypothesis (flac_decode.hip k_dec_spec): 1 (default)
   takes a frame's end from the next frame-header candidate whose bytes give
   a zero CRC-16 residue, so the parse does not walk the frame's last
   subframe; the restore checks every such frame on the subframe it walks
   anyway, and a batch with a failed check is redone with every subframe
   walked inside atg_flac_decode_wait -- results are those of the full parse
   (src/decoders/flac.c:174-285) either way; after four redone batches in a
   row the decoder switches itself to 0 (a stream of input the hypothesis
   keeps failing on would pay two decodes per batch) until the mode is set
   again.  0: every subframe walked by the parse.  2: as 1, and every batch
   redone (self-check of the redo path). */
atg_status atg_decoder_set_frame_hypothesis(atg_decoder *dec, int mode);

/* Batches this decoder redid with the full parse (mode 1: failed checks). */
uint64_t atg_decoder_frame_hypothesis_redos(atg_decoder *dec);

/* Asynchronous form of atg_flac_decode_device, D batches in flight (D = 3
   unless atg_decoder_set_inflight says otherwise, each slot with its own
   buffers): the scan, parse and frame walk run on the decoder's stream
   (two host round trips for the counts), then the restore, emit and
   per-track MD5 on the batch's slot stream, so batch k's back half runs
   under batch k+1's scan and parse.  Returns once everything is queued.
   d_data must stay valid and unchanged until the batch is waited: when a
   frame-end hypothesis fails its check, atg_flac_decode_wait re-reads
   d_data to redo the batch with the full parse.  The PCM pointer the wait
   returns stays valid until the slot is reused, D enqueues later.  An
   enqueue while D batches are unwaited fails with ATG_ERR_INVALID; an
   enqueue that fails leaves nothing of its batch queued. */
atg_status atg_flac_decode_device_async(atg_decoder *dec, const void *d_data, uint64_t len,
                                        const atg_flac_dec_track *tracks, uint32_t n_tracks,
                                        uint64_t *ticket);
atg_status atg_flac_decode_wait(atg_decoder *dec, uint64_t ticket,
                                atg_flac_dec_result *results, const int32_t **d_pcm,
                                uint64_t *total_samples);

/* Per-kernel device time of the decoder's most recently waited batch.  After
   an Ogg FLAC batch the container pass's phases follow the seven of the
   FLAC decode: ogg_walk, ogg_crc, ogg_gather. */
int atg_decoder_kernel_times(atg_decoder *dec, const char **names, float *ms, int cap);

/* ------------------------------------------------------------------ */
/* Ogg FLAC decoder (.oga; trackverify / track2track through           */
/* OggFlacAudio.to_pcm).  Replaces the reference's                      */
/* audiotools.decoders.OggFlacDecoder: the page reader and packet       */
/* iterator (src/ogg.c:24-119, 203-254), the first packet               */
/* (src/decoders/oggflac.c:324-394) and the frame loop (:471-559), for  */
/* a batch of images, on the atg_decoder handle.                        */
/*                                                                      */
/* Pages are read in file order; only the magic, the version, the       */
/* end-of-stream flag, the lacing table and the checksum are used.  A   */
/* page fails with the first of: invalid magic, invalid version,        */
/* premature EOF (a read past the image anywhere in the page, a file    */
/* that ends without an end-of-stream page included), checksum          */
/* mismatch.  A page is checked whole before any of its segments is     */
/* handed out; nothing is read after the end-of-stream page.  A packet  */
/* is the segments up to the first lacing value below 255; one left     */
/* unfinished at the end of the stream is dropped.  The first packet    */
/* carries STREAMINFO and the number of header packets, which are       */
/* skipped unparsed; every packet after them is decoded as one FLAC     */
/* frame from its first byte, its reads bounded by the packet (bytes    */
/* after the frame are ignored, total_samples is never consulted).      */
/* Where the reference aborts -- a frame whose subframes end within the  */
/* last two bytes of its packet -- the status is ATG_FD_EOF.             */
/* ------------------------------------------------------------------ */

/* Limits, refused with ATG_ERR_UNSUPPORTED before any launch: one image
   (which bounds its pages, its packets and its largest packet) and the
   batch buffer. */
#define ATG_OGG_MAX_IMAGE_BYTES (1ull << 28)
#define ATG_OGG_MAX_BATCH_BYTES (1ull << 32)
/* which follow from the image size: a page is at least 27 bytes, a packet
   takes at least one lacing byte */
#define ATG_OGG_MAX_PAGES (ATG_OGG_MAX_IMAGE_BYTES / 27)
#define ATG_OGG_MAX_PACKETS ATG_OGG_MAX_IMAGE_BYTES
#define ATG_OGG_MAX_PACKET_BYTES ATG_OGG_MAX_IMAGE_BYTES

/* What ended the container side of a stream: the reference's ogg_status
   (src/ogg.h) and the first packet's errors (oggflac.c:324-394). */
enum {
    ATG_OGG_OK = 0,
    ATG_OGG_MAGIC = 1,           /* ValueError "invalid magic number" */
    ATG_OGG_VERSION = 2,         /* ValueError "invalid stream version" */
    ATG_OGG_CHECKSUM = 3,        /* ValueError "checksum mismatch" */
    ATG_OGG_PREMATURE_EOF = 4,   /* IOError "premature EOF reading Ogg stream" */
    ATG_OGG_STREAM_FINISHED = 5, /* IOError "stream finished": no first packet,
                                    or fewer header packets than stated */
    ATG_OGG_PACKET_BYTE = 6,     /* ValueError "invalid packet byte" */
    ATG_OGG_SIGNATURE = 7,       /* ValueError "invalid Ogg signature" */
    ATG_OGG_MAJOR_VERSION = 8,   /* ValueError "invalid major version" */
    ATG_OGG_MINOR_VERSION = 9,   /* ValueError "invalid minor version" */
    ATG_OGG_FLAC_SIGNATURE = 10, /* ValueError "invalid fLaC signature" */
    ATG_OGG_BLOCK_TYPE = 11,     /* ValueError "invalid block type" */
    ATG_OGG_STREAMINFO_EOF = 12  /* IOError "EOF while reading STREAMINFO block" */
};

/* The first packet of an image in host memory (oggflac_read_streaminfo), read
   through pages checked as above: STREAMINFO, the header-packet count, the
   first page's serial number, and the channel mask a VORBIS_COMMENT header
   packet's WAVEFORMATEXTENSIBLE_CHANNEL_MASK gives (else the default for the
   channel count).  si.frames_offset = byte of the image where the page after
   the first packet's last page starts. */
typedef struct {
    atg_flac_streaminfo si;
    uint32_t header_packets;
    uint32_t serial_number;
    uint32_t has_channel_mask; /* the tag was present and matched the channels */
    uint32_t reserved;
} atg_oggflac_info;

/* Returns ATG_OGG_OK or the ATG_OGG_* value of the failure; host code only. */
int atg_oggflac_read_info(const uint8_t *data, uint64_t len, atg_oggflac_info *info);

/* One stream of a batch: its whole image data[data_offset, +data_bytes). */
typedef struct {
    uint64_t data_offset;
    uint64_t data_bytes;
} atg_oggflac_dec_track;

/* Per-stream result: the stream hands out n_frames FLAC frames = pcm_frames
   PCM frames (interleaved int32 at PCM-frame index pcm_offset of the batch
   output; sample_offset is the same place as an index of interleaved
   samples, exact also in a batch of streams with different channel counts,
   which the caller of this entry cannot sort beforehand) and then ends with
   the first failure in stream order: `status` when
   a frame failed (ATG_FD_*), else `ogg_status` when the container ran out or
   failed, else status ATG_FD_MD5 or, with both 0, success.  md5 = MD5 of the
   frames' little-endian PCM bytes.  pages = pages that passed every check
   before the first failing one; packets = packets completed in them;
   fail_page / fail_offset = index and image byte of the failing page
   (0xFFFFFFFF / 0 when the stream ended by its flag).  The STREAMINFO fields
   are zero unless the first packet parsed. */
typedef struct {
    uint64_t pcm_offset;
    uint64_t pcm_frames;
    uint32_t n_frames;
    int32_t status;
    int32_t ogg_status;
    uint32_t header_packets;
    uint8_t md5[16];
    uint32_t pages;
    uint32_t packets;
    uint32_t fail_page;
    uint32_t reserved;
    uint64_t fail_offset;
    uint32_t sample_rate, channels, bits_per_sample, max_block_size;
    uint64_t total_samples;
    uint8_t streaminfo_md5[16];
    uint64_t sample_offset;
} atg_oggflac_dec_result;

/* As atg_flac_decode_host / _device / _fetch.  The container pass (page walk,
   page CRC-32, packet table, gather into per-stream contiguous buffers) and
   the frame decode run on the GPU; three host round trips for the counts.
   frame_offsets of the fetch are relative to the stream's first audio packet
   in the compacted stream.  Fails with ATG_ERR_INVALID while an
   atg_flac_decode_device_async batch is unwaited. */
atg_status atg_oggflac_decode_host(atg_decoder *dec, const uint8_t *data, uint64_t len,
                                   const atg_oggflac_dec_track *tracks, uint32_t n_tracks,
                                   atg_oggflac_dec_result *results, uint64_t *total_samples,
                                   uint64_t *total_frames);
atg_status atg_oggflac_decode_device(atg_decoder *dec, const void *d_data, uint64_t len,
                                     const atg_oggflac_dec_track *tracks, uint32_t n_tracks,
                                     atg_oggflac_dec_result *results, const int32_t **d_pcm,
                                     uint64_t *total_samples);
atg_status atg_oggflac_decode_fetch(atg_decoder *dec, int32_t *pcm, uint64_t pcm_cap,
                                    uint64_t *frame_offsets, uint32_t *frame_block_sizes,
                                    uint64_t frame_cap);

/* ------------------------------------------------------------------ */
/* Ogg FLAC (.oga) batch encode: the FLAC frames of atg_flac_encode_*   */
/* in an Ogg container (csrc/ogg_mux.hip).  The reference pipes PCM to  */
/* the external `flac --ogg` program (audiotools/flac.py:3249-3367);    */
/* the page layout here is this library's own,   */
/* and what the reference's decoder (src/ogg.c, src/decoders/oggflac.c) */
/* accepts.  Packets: the mapping's first packet with STREAMINFO, one   */
/* per further metadata block (VORBIS_COMMENT, PADDING when             */
/* padding_size > 0), one per FLAC frame.  A page closes when it holds  */
/* page_segments lacing values, when a header packet ends on it, and    */
/* with ATG_OGG_PAGE_PER_PACKET when any packet ends on it.             */
/* ------------------------------------------------------------------ */
#define ATG_OGG_PAGE_PER_PACKET 1u
typedef struct {
    uint32_t serial_number; /* track t gets serial_number + t (mod 2^32) */
    uint32_t page_segments; /* 1..255; 0 = 255 */
    uint32_t flags;         /* ATG_OGG_PAGE_PER_PACKET */
    uint32_t channel_mask;  /* nonzero: VORBIS_COMMENT carries
                               WAVEFORMATEXTENSIBLE_CHANNEL_MASK=0x%.4X */
} atg_oggflac_enc_options;

/* As atg_track_result (bytes = the whole .oga image at out + out_offset),
   plus the image's pages, its header pages and its serial number. */
typedef struct {
    uint64_t out_offset;
    uint64_t bytes;
    uint32_t first_frame;
    uint32_t n_frames;
    uint32_t min_frame_bytes;
    uint32_t max_frame_bytes;
    uint8_t md5[16];
    int32_t status;
    uint32_t pages;
    uint32_t header_pages;
    uint32_t serial_number;
} atg_oggflac_track_result;

/* Frames and worst-case output bytes of a batch (host code, no HIP call):
   an upper bound on the layout for any frame sizes up to
   atg_flac_batch_bounds' worst case.  ATG_ERR_INVALID for page_segments >
   255, unknown flags and whatever the FLAC options are refused for. */
atg_status atg_oggflac_batch_bounds(const atg_flac_options *opts,
                                    const atg_oggflac_enc_options *ogg_opts,
                                    const atg_track *tracks, uint32_t n_tracks,
                                    uint32_t channels, uint32_t bits_per_sample,
                                    uint64_t *total_frames, uint64_t *out_bytes);

/* Encode a batch to .oga images.  As atg_flac_encode_device / _host; the
   device entry leaves track t's image at results[t].out_offset of d_out
   (16-byte aligned slots sized by the bounds), the host entry packs the
   images back to back, 16-byte aligned.  frame_page_offsets[first_frame + i]
   = byte, from the image's start, of the page on which frame i's packet
   begins; frame_pcm_frames as the FLAC entries (both host arrays of
   total_frames entries, may be NULL).  ATG_ERR_INVALID while an asynchronous
   FLAC batch or host job of the engine is unwaited. */
atg_status atg_oggflac_encode_device(atg_engine *eng, const atg_flac_options *opts,
                                     const atg_oggflac_enc_options *ogg_opts,
                                     const void *d_pcm, atg_pcm_format format,
                                     const atg_track *tracks, uint32_t n_tracks,
                                     uint32_t channels, uint32_t bits_per_sample,
                                     uint32_t sample_rate, void *d_out, uint64_t out_cap,
                                     atg_oggflac_track_result *results,
                                     uint64_t *frame_page_offsets,
                                     uint32_t *frame_pcm_frames);
atg_status atg_oggflac_encode_host(atg_engine *eng, const atg_flac_options *opts,
                                   const atg_oggflac_enc_options *ogg_opts,
                                   const void *pcm, atg_pcm_format format,
                                   const atg_track *tracks, uint32_t n_tracks,
                                   uint32_t channels, uint32_t bits_per_sample,
                                   uint32_t sample_rate, uint8_t *out, uint64_t out_cap,
                                   atg_oggflac_track_result *results,
                                   uint64_t *frame_page_offsets,
                                   uint32_t *frame_pcm_frames);

/* ------------------------------------------------------------------ */
/* Integer PCM converters (track2track --bits-per-sample / --channels). */
/* Replace the read() bodies of the reference's pcmconverter types:     */
/* BPSConverter (src/pcmconverter.c:667-747, dither src/dither.c:73-89),*/
/* Downmixer (:220-342) and Averager (:64-97), over whole tracks.       */
/* PCM is interleaved int32 (FrameList layout) in and out.              */
/* ------------------------------------------------------------------ */
enum {
    ATG_CONV_BPS = 0,     /* in_bps -> out_bps; dither bits when reducing */
    ATG_CONV_DOWNMIX = 1, /* -> 2 channels (channel_mask 0 = invented mask) */
    ATG_CONV_AVERAGE = 2  /* -> 1 channel */
};

const char *atg_pcm_convert_last_error(void);
uint32_t atg_pcm_convert_out_channels(int kind, uint32_t in_channels);

/* Device buffers; `stream` is a hipStream_t (NULL = default stream); the
   call returns after the launch.  Reducing bits reads one dither bit per
   sample from d_dither, starting at bit dither_bit0, MSB first, in the
   reference's order: per 4096-frame read(), channel by channel. */
atg_status atg_pcm_convert_device(int kind, const int32_t *d_in, int32_t *d_out,
                                  uint64_t frames, uint32_t channels, uint32_t channel_mask,
                                  uint32_t in_bps, uint32_t out_bps, const uint8_t *d_dither,
                                  uint64_t dither_bit0, void *stream);

/* Host buffers (staged through the device); out holds
   frames x atg_pcm_convert_out_channels() samples. */
atg_status atg_pcm_convert_host(int device, int kind, const int32_t *in, int32_t *out,
                                uint64_t frames, uint32_t channels, uint32_t channel_mask,
                                uint32_t in_bps, uint32_t out_bps, const uint8_t *dither,
                                uint64_t dither_bytes, uint64_t dither_bit0);

/* ------------------------------------------------------------------ */
/* AccurateRip checksums (trackverify -R, cd2track).                    */
/* Replaces audiotools._accuraterip.ChecksumV1 / ChecksumV2             */
/* (src/accuraterip.c:121-326) for every track of a batch, and gives v1 */
/* at every drive read offset in [-max_offset, max_offset].  Tracks are */
/* stereo, 16 bits per sample, interleaved, in ATG_PCM_S16 or           */
/* ATG_PCM_S32.  Stateless: no handle.                                  */
/* ------------------------------------------------------------------ */
#define ATG_AR_FIRST 1u /* atg_ar_track.flags: first track of the disc */
#define ATG_AR_LAST 2u  /* last track of the disc */

/* One track, or one piece of a track fed in pieces.  Frame i (from 1) has
   the index index0 + i and the value (uint16(right) << 16) | uint16(left);
   it counts when start <= index <= end, start = (sample_rate / 75) * 5 for
   a first track (else 0), end = (uint32_t)(total_pcm_frames - that skip)
   for a last track (else total_pcm_frames).  The cast wraps, as the
   reference's does: a last track shorter than the skip has nothing cut.
   At offset k frame i is read from frame position pcm_offset + k + i - 1 of
   the buffer; positions outside [lo_frame, hi_frame) read as silence (the
   track itself for separate files, the whole image for a disc image). */
typedef struct {
    int64_t pcm_offset;   /* buffer position of the track's first frame */
    uint64_t pcm_frames;
    uint64_t lo_frame, hi_frame;
    uint32_t index0;           /* index of the first frame, minus 1 */
    uint32_t total_pcm_frames; /* the range rule's length; pcm_frames unless
                                  this is a piece of a longer track */
    uint32_t sample_rate;
    uint32_t flags;            /* ATG_AR_FIRST | ATG_AR_LAST */
} atg_ar_track;

typedef struct {
    uint32_t v1, v2; /* at offset 0 */
    int32_t status;  /* 0 */
    uint32_t reserved;
} atg_ar_result;

const char *atg_accuraterip_last_error(void);

/* Checksums of n_tracks tracks whose PCM is in device memory (16-byte
   aligned, readable over every track's [lo_frame, hi_frame)).  offset_v1 is
   a host array of n_tracks x (2 * max_offset + 1) values, v1 at offset k of
   track t at [t * (2 * max_offset + 1) + max_offset + k]; it may be NULL
   when max_offset is 0.  v2 is not linear in the offset and is given at
   offset 0 only: submit the track again with pcm_offset + k for v2 there.
   Checked before any GPU call, ATG_ERR_INVALID: NULL arrays with n_tracks
   > 0, an unknown format, sample_rate 0, pcm_frames or total_pcm_frames 0,
   lo_frame > hi_frame, index0 + pcm_frames >= 2^32; ATG_ERR_UNSUPPORTED:
   max_offset above 65535.  Synchronises `stream` before it returns. */
atg_status atg_accuraterip_device(const void *d_pcm, int format, const atg_ar_track *tracks,
                                  uint32_t n_tracks, uint32_t max_offset,
                                  atg_ar_result *results, uint32_t *offset_v1, void *stream);

/* The same for PCM in host memory (pcm_frames_total frames), staged through
   `device`; also ATG_ERR_INVALID for a hi_frame above pcm_frames_total. */
atg_status atg_accuraterip_host(int device, const void *pcm, int format,
                                uint64_t pcm_frames_total, const atg_ar_track *tracks,
                                uint32_t n_tracks, uint32_t max_offset,
                                atg_ar_result *results, uint32_t *offset_v1);

/* PCM frames per tile of the streaming pass (tests place track lengths
   around it). */
uint32_t atg_accuraterip_tile_frames(void);

/* ------------------------------------------------------------------ */
/* Packed PCM bytes <-> integer PCM, and the AIFF / Sun AU containers.  */
/* The ten byte layouts of the reference's FrameList(bytes, ...) and    */
/* FrameList.to_bytes (src/pcm.c, converters src/pcmconv.c): 1, 2 or 3  */
/* bytes per sample, little or big endian, signed or unsigned (an       */
/* unsigned sample's value is raw - 2^(bits-1)).  Stateless: no handle. */
/* ------------------------------------------------------------------ */
typedef struct {
    uint8_t bytes_per_sample; /* 1, 2 or 3 */
    uint8_t big_endian;       /* ignored for 1 byte per sample */
    uint8_t is_signed;
    uint8_t reserved;
} atg_pcm_layout;

/* `samples` packed samples from byte `byte_offset` of the packed buffer
   (any offset) <-> the samples from index `sample_offset` of the integer
   buffer.  Runs of one call must not overlap on the side written. */
typedef struct {
    uint64_t byte_offset, samples, sample_offset;
} atg_pcm_run;

const char *atg_pcm_bytes_last_error(void);

/* Unpack every run of d_bytes (device memory) into d_pcm, interleaved int16
   (ATG_PCM_S16, layouts of at most 2 bytes) or int32.  One launch for the
   whole table.  Memory contract: the kernel reads only aligned 16-byte
   units of d_bytes that hold at least one byte of some run, so d_bytes must
   be 16-byte aligned and bytes_cap a multiple of 16; it writes d_pcm in
   16-byte groups inside the runs' sample ranges, so d_pcm must be 16-byte
   aligned and every sample_offset a multiple of 16 / sizeof(sample).
   Checked before any GPU call, ATG_ERR_INVALID: NULL arrays with n_runs >
   0, bytes_per_sample outside 1..3, ATG_PCM_S16 with 3 bytes per sample, an
   unknown format, a misaligned buffer, capacity or sample_offset;
   ATG_ERR_CAPACITY: a run whose packed range passes bytes_cap or whose
   sample range passes pcm_cap_samples.  Nothing is launched for n_runs ==
   0 or when every run is empty.  `stream` is a hipStream_t (NULL = default
   stream); it is synchronised before the call returns. */
atg_status atg_pcm_unpack_device(const void *d_bytes, uint64_t bytes_cap, atg_pcm_layout layout,
                                 const atg_pcm_run *runs, uint32_t n_runs, void *d_pcm,
                                 atg_pcm_format format, uint64_t pcm_cap_samples, void *stream);

/* The inverse: d_pcm's runs packed into d_bytes, each value (plus 2^(bits-1)
   when unsigned) masked to the layout's width as FrameList.to_bytes masks
   it.  The kernel writes only bytes inside a run's packed range and never
   reads the packed buffer, so runs may sit back to back at odd offsets; it
   reads only the runs' own samples.  d_bytes must be 16-byte aligned and
   d_pcm aligned to its sample size; sample_offset may be any.  The other
   checks are those of atg_pcm_unpack_device. */
atg_status atg_pcm_pack_device(const void *d_pcm, atg_pcm_format format, uint64_t pcm_cap_samples,
                               atg_pcm_layout layout, const atg_pcm_run *runs, uint32_t n_runs,
                               void *d_bytes, uint64_t bytes_cap, void *stream);

/* The same for host buffers of any alignment, staged through `device`: only
   the runs' ranges of the output buffer are written. */
atg_status atg_pcm_unpack_host(int device, const void *bytes, uint64_t n_bytes,
                               atg_pcm_layout layout, const atg_pcm_run *runs, uint32_t n_runs,
                               void *pcm, atg_pcm_format format, uint64_t pcm_cap_samples);
atg_status atg_pcm_pack_host(int device, const void *pcm, atg_pcm_format format,
                             uint64_t pcm_cap_samples, atg_pcm_layout layout,
                             const atg_pcm_run *runs, uint32_t n_runs, void *bytes,
                             uint64_t n_bytes);

/* Samples per tile of both kernels (tests place run lengths around it). */
uint32_t atg_pcm_bytes_tile_samples(void);

/* Name and milliseconds of the calling thread's last launch ("unpack" or
   "pack"); returns the number of entries written, 0 before any launch. */
int atg_pcm_bytes_kernel_times(const char **names, float *ms, int cap);

/* Status bit of a file decoded by the batch PCM reader: the file holds fewer
   data bytes than its header says; the PCM is the whole frames present. */
#define ATG_PCMF_TRUNCATED 1

/* atg_aiff_read_info: 0, or one of these for the reference's errors
   (audiotools/text.py:530-545, those AiffReader.__init__ can raise), or
   ATG_ERR_UNSUPPORTED for a bits_per_sample other than 8, 16 or 24 or a
   sample rate outside [0, 2^32), ATG_ERR_INVALID for a NULL argument. */
enum {
    ATG_AIFF_OK = 0,
    ATG_AIFF_NOT_AIFF = 1,         /* "not an AIFF file" */
    ATG_AIFF_INVALID_AIFF = 2,     /* "invalid AIFF file" */
    ATG_AIFF_INVALID_CHUNK_ID = 3, /* "invalid AIFF chunk ID" */
    ATG_AIFF_INVALID_CHUNK = 4,    /* "invalid AIFF chunk": pad byte missing */
    ATG_AIFF_PREMATURE_SSND = 5,   /* "SSND chunk found before fmt", and no
                                      COMM chunk after it */
    ATG_AIFF_NO_SSND = 6,          /* "SSND chunk not found" */
    ATG_AIFF_IOERROR = 7           /* the file ends inside the COMM fields */
};

typedef struct {
    uint32_t channels;
    uint32_t bits_per_sample;
    uint32_t sample_rate;  /* the 80-bit extended field, truncated */
    uint32_t channel_mask; /* 0x4 for 1 channel, 0x3 for 2, otherwise 0 */
    uint64_t total_pcm_frames;
    uint64_t ssnd_data_offset; /* first sound byte: after SSND's two words */
    uint64_t ssnd_data_bytes;  /* the chunk's sound bytes present in the image */
} atg_aiff_info;

/* Walks the chunks of a whole file image up to SSND, as the reference's
   AiffReader does; an SSND chunk met before COMM is kept and the walk goes on
   to COMM (the reference refuses such a file).  ssnd_data_offset +
   ssnd_data_bytes <= len always. */
int atg_aiff_read_info(const uint8_t *data, uint64_t len, atg_aiff_info *info);

/* atg_au_read_info: 0, one of these (text.py:547-548), ATG_ERR_UNSUPPORTED
   for a header with no channels, ATG_ERR_INVALID for a NULL argument. */
enum {
    ATG_AU_OK = 0,
    ATG_AU_INVALID_HEADER = 1,     /* "invalid Sun AU header" */
    ATG_AU_UNSUPPORTED_FORMAT = 2, /* "unsupported Sun AU format" */
    ATG_AU_IOERROR = 3             /* fewer than the header's 24 bytes */
};

typedef struct {
    uint32_t channels;
    uint32_t bits_per_sample; /* encodings 2, 3, 4 -> 8, 16, 24 */
    uint32_t sample_rate;
    uint32_t channel_mask;
    uint64_t total_pcm_frames; /* data_size / bytes per frame */
    uint64_t data_offset, data_size; /* as the header states them */
    uint64_t data_bytes; /* of data_size, those present in the image */
} atg_au_info;

int atg_au_read_info(const uint8_t *data, uint64_t len, atg_au_info *info);

/* ------------------------------------------------------------------ */
/* PCM comparison (trackcmp) and offset search.                         */
/* Replaces pcm_frame_cmp over two decoded streams (trackcmp's          */
/* cmp_files) and over PCMReaderWindow views of a CD image (its         */
/* image_compare) for every pair of a batch, and finds the frame shift  */
/* at which two streams hold the same audio.  Stateless: no handle.     */
/* ------------------------------------------------------------------ */
#define ATG_PCM_NO_MISMATCH UINT64_MAX

/* A view: an infinite sequence of PCM frames over a finite source.  View
   frame i is source frame window_offset + i; source frames outside
   [0, src_frames) are silence (every channel 0).  The source's samples are
   d_pcm[sample_offset .. sample_offset + src_frames * channels), channel-
   interleaved int16 or int32. */
typedef struct {
    const void *d_pcm;      /* device memory, aligned to its sample size */
    uint64_t sample_offset; /* index in d_pcm of the source's first sample */
    uint64_t src_frames;    /* PCM frames the source holds */
    int64_t window_offset;  /* source frame of view frame 0; may be negative */
    uint32_t format;        /* ATG_PCM_S16 / ATG_PCM_S32 */
    uint32_t reserved;
} atg_pcm_view;

/* `frames` frames of view a against view b, both of `channels` channels;
   the two formats are independent and an int16 sample is compared by its
   sign-extended value. */
typedef struct {
    atg_pcm_view a, b;
    uint64_t frames;
    uint32_t channels, reserved;
} atg_pcm_pair;

typedef struct {
    uint64_t first_mismatch; /* smallest i in [0, frames) at which any channel
                                differs, or ATG_PCM_NO_MISMATCH */
    int32_t offset;          /* the search's shift k: a(i) == b(i + k) */
    uint32_t offset_found;
} atg_pcm_cmp_result;

const char *atg_pcm_compare_last_error(void);

/* first_mismatch of every pair, one launch for the whole table; offset and
   offset_found are set to 0.  Memory contract: the kernel reads only
   aligned 16-byte units that hold at least one sample of a view's source
   range [sample_offset, sample_offset + src_frames * channels); buffers
   need only be aligned to their sample size, and a and b may share one.
   Checked before any GPU call, ATG_ERR_INVALID: NULL arrays with n_pairs >
   0, an unknown format, d_pcm NULL with src_frames > 0, a pointer off its
   sample size, channels == 0, frames * channels or src_frames * channels at
   or above 2^62, a source that ends at or beyond sample 2^62,
   |window_offset| at or above 2^62; ATG_ERR_UNSUPPORTED: channels > 8.
   Nothing is launched for n_pairs == 0 or when every pair has frames == 0
   (an empty pair has no mismatch).  `stream` is a hipStream_t (NULL =
   default stream); it is synchronised before the call returns. */
atg_status atg_pcm_compare_device(const atg_pcm_pair *pairs, uint32_t n_pairs,
                                  atg_pcm_cmp_result *results, void *stream);

/* With S = { k in [-max_offset, max_offset] : a(i) == b(i + k) for every i in
   [0, frames) }, b read at any index with silence outside its source:
   offset is the k in S of smallest |k| (of +k and -k the positive one) and
   offset_found says whether S has any; first_mismatch is the one at shift
   0.  An empty pair gives offset_found = 1, offset = 0.  The checks are
   those of atg_pcm_compare_device, and ATG_ERR_UNSUPPORTED for max_offset
   above 65535.  At most 2 * max_offset + 1 shifts are verified per pair. */
atg_status atg_pcm_offset_search_device(const atg_pcm_pair *pairs, uint32_t n_pairs,
                                        uint32_t max_offset, atg_pcm_cmp_result *results,
                                        void *stream);

/* PCM frames per tile of the compare pass (tests place lengths around it). */
uint32_t atg_pcm_compare_tile_frames(void);

/* Milliseconds the calling thread's last call spent in its kernels:
   "compare" (every compare launch of the call) and "probe" (the search's
   shift probe); returns the number of entries written, 0 before any call
   that launched. */
int atg_pcm_compare_kernel_times(const char **names, float *ms, int cap);

/* ------------------------------------------------------------------ */
/* The PCM converter chain of a batch conversion (track2track with      */
/* another channel count or bits per sample).  One launch does, for     */
/* every track of a ragged table, what the reference's PCMConverter     */
/* stacks as readers (audiotools/__init__.py:2729-2802) on either side  */
/* of its resampler: a channel operation (ReorderedPCMReader /          */
/* RemaskedPCMReader / Downmixer / Averager), then BPSConverter.        */
/* Stateless: no handle.                                                */
/* ------------------------------------------------------------------ */
enum {
    ATG_CHAIN_MAP = 0,             /* output k = input map[k], or silence */
    ATG_CHAIN_DOWNMIX = 1,         /* ATG_CONV_DOWNMIX's arithmetic, -> 2 channels */
    ATG_CHAIN_AVERAGE = 2,         /* ATG_CONV_AVERAGE's, -> 1 channel */
    ATG_CHAIN_DOWNMIX_AVERAGE = 3  /* Averager(Downmixer(x)), -> 1 channel */
};
#define ATG_CHAIN_SILENT 0xFFu /* a map entry: the output channel is silence */

/* One track.  src is read as atg_pcm_view describes a source (src_frames
   frames of in_channels channels from sample_offset on; window_offset must
   be 0).  The channel operation gives out_channels channels at in_bps bits,
   the bits-per-sample operation then out_bps: up is x << s, down is
   (x >> s) ^ dither bit, identity when the two are equal.  A row that
   reduces takes src_frames * out_channels bits of the call's dither stream
   from bit dither_bit0 on, MSB first, in atg_pcm_convert_device's order:
   per 4096-frame read of the stage's input (the last read short), channel
   by channel within a read.  The output is the src_frames * out_channels
   samples from index out_offset of the call's output buffer. */
typedef struct {
    atg_pcm_view src;
    uint32_t in_channels, out_channels; /* 1..8; 2 for DOWNMIX, 1 for the averages */
    uint32_t channel_op;                /* ATG_CHAIN_* */
    uint32_t channel_mask;              /* the downmixes: the input's mask, 0 =
                                           the invented mask of its channel count */
    uint8_t map[8];                     /* MAP: per output channel an input
                                           channel or ATG_CHAIN_SILENT */
    uint32_t in_bps, out_bps;           /* 1..24 */
    uint64_t out_offset;
    uint64_t dither_bit0;
} atg_pcm_chain_row;

const char *atg_pcm_chain_last_error(void);

/* Convert every row in one launch; d_out is interleaved int16 (ATG_PCM_S16,
   rows of at most 16 output bits) or int32.  Memory contract: the kernel
   reads only aligned 16-byte units that hold at least one sample of some
   row's source range, so sources need only be aligned to their sample size
   and may lie at any sample offset; it reads only the dither bytes that hold
   a row's bits; it writes only samples inside the rows' output ranges, in
   16-byte groups, so d_out must be 16-byte aligned and every out_offset a
   multiple of 16 / sizeof(sample).
   Checked before any GPU call, ATG_ERR_INVALID: rows NULL with n_rows > 0;
   d_out NULL with output to write; d_dither NULL with a row that reduces; a
   channel count outside 1..8 or one that does not fit the operation; an
   unknown operation or format; a map entry at or above in_channels; a
   downmix mask that names more channels than present; bits per sample
   outside 1..24; ATG_PCM_S16 output for a row of more than 16 bits; a source
   pointer off its sample size or NULL with frames; window_offset != 0; a
   misaligned d_out or out_offset; output rows that overlap; a dither range
   that passes dither_bytes.  ATG_ERR_CAPACITY: an output range that passes
   out_cap_samples.  Nothing is launched for n_rows == 0 or when every row is
   empty.  `stream` is a hipStream_t (NULL = default stream); it is
   synchronised before the call returns. */
atg_status atg_pcm_chain_device(const atg_pcm_chain_row *rows, uint32_t n_rows, void *d_out,
                                atg_pcm_format out_format, uint64_t out_cap_samples,
                                const uint8_t *d_dither, uint64_t dither_bytes, void *stream);

/* The same for host memory, staged through `device`: src.d_pcm, out and
   dither are host pointers.  Every source goes up at its own address modulo
   16 and `out` goes up whole before the launch and comes back whole after
   it, so only the rows' ranges of it change. */
atg_status atg_pcm_chain_host(int device, const atg_pcm_chain_row *rows, uint32_t n_rows,
                              void *out, atg_pcm_format out_format, uint64_t out_cap_samples,
                              const uint8_t *dither, uint64_t dither_bytes);

/* Samples per tile on a row's wider side: a tile is 8 * (tile_samples / (8 *
   max(in_channels, out_channels))) frames (tests place lengths around it). */
uint32_t atg_pcm_chain_tile_samples(void);

/* Name ("chain") and milliseconds of the calling thread's last launch;
   returns the number of entries written, 0 before any launch. */
int atg_pcm_chain_kernel_times(const char **names, float *ms, int cap);

/* ------------------------------------------------------------------ */
/* ReplayGain analysis (tracktag/track2track --replay-gain).           */
/* Replaces ReplayGain(rate).title_gain(pcmreader) for every track of a */
/* batch and album_gain() per album (src/replaygain.c:115-322,         */
/* :566-807).  PCM is interleaved int32 (FrameList layout), 1 or 2      */
/* channels, 8/16/24 bits, one of the 20 supported sample rates.        */
/* ------------------------------------------------------------------ */
typedef struct {
    uint64_t pcm_offset; /* first PCM frame of the track in d_pcm */
    uint64_t pcm_frames;
    uint32_t channels, bits_per_sample, sample_rate;
    uint32_t album;      /* album index (tracks grouped by album) */
    /* host array: the frame counts pcmreader.read(4096) returned, one
       ReplayGain_analyze_samples call each (replaygain.c:210-305); they
       decide the fp64 summation order.  NULL = 4096-frame reads. */
    const uint32_t *chunk_frames;
    uint64_t n_chunks;
} atg_rg_track;

typedef struct {
    double title_gain;   /* dB; 0.0 when no 50 ms window completed */
    double title_peak;   /* max |x| / 2^(bps-1) */
    int32_t status;      /* 0 ok, 1 not enough samples */
    uint32_t reserved;
} atg_rg_result;

const char *atg_replaygain_last_error(void);

/* Title gains/peaks of all tracks; when n_albums > 0 also each album's
   12000-bin window histogram (the reference's B array) into d_album_hist
   (device, n_albums x 12000 uint32; NULL = internal) and album peaks into
   album_peaks (host, may be NULL).  Album gains follow from
   atg_replaygain_hist_gain -- after an RCCL all-reduce of the histograms
   when an album spans several GPUs. */
atg_status atg_replaygain_device(const int32_t *d_pcm, const atg_rg_track *tracks,
                                 uint32_t n_tracks, uint32_t n_albums, atg_rg_result *results,
                                 uint32_t *d_album_hist, double *album_peaks, void *stream);

/* The certification bound of the time-split title analysis for one sample
   rate (host computation, no GPU), out[6]: out[0] G = max over lags of the
   Butterworth output's l1 response to a unit error state, out[1] R_s and
   out[2] R_b the rounding sums into the state and the output, out[3]
   1 / (1 - ||A^L||_inf), out[4] L the segment length in frames, out[5] G_L
   = max over lags >= L (see replaygain.hip k_rg_seg).  A warm segment's
   outputs err by at most G m + G_L (m + R_s) out[3] + 1.5 R_b for the
   largest measured seam state difference m. */
atg_status atg_replaygain_bound(uint32_t sample_rate, double *out);
/* The multiple of R_b the kernels use in that bound: 1.5 -- R_b is two
   trajectories' rounding, and the bound counts three trajectories once
   each (warm, predecessor, and the serial one at disjoint times; the
   derivation is in replaygain.hip). */
double atg_replaygain_rb_factor(void);
/* windows whose histogram bin the host's log10 moved (lifetime count; a
   window within 1e-9 of a bin edge is binned with the C library's log10) */
uint64_t atg_replaygain_rebinned_windows(void);
/* Test hooks of the time-split analysis (replaygain.hip): the warm-up
   frames of every segment after a track's first (-1 = the rate-scaled
   default; 0 = none, so every track fails certification and is analysed
   again serially), and how many tracks the last atg_replaygain_device call
   analysed again serially. */
void atg_replaygain_set_warmup(int frames);
uint32_t atg_replaygain_fallback_tracks(void);

/* analyzeResult (replaygain.c:754-776) of n device histograms -> gains
   (host); NaN = not enough samples (album_gain raises ValueError). */
atg_status atg_replaygain_hist_gain(const uint32_t *d_hist, uint32_t n, double *gains,
                                    void *stream);

/* ReplayGainReader (src/replaygain.c:820-925): multiplier from (gain, peak)
   as ReplayGainReader_init computes it (long double pow; 1/peak when the
   gain would amplify), then per sample lround(x * multiplier), clamp to
   bits_per_sample, XOR one dither bit (consumed per read(chunk_frames)
   call, channel by channel, MSB first, starting at dither_bit0). */
double atg_replaygain_multiplier(double replaygain, double peak);
atg_status atg_pcm_apply_gain_device(const int32_t *d_in, int32_t *d_out, uint64_t frames,
                                     uint32_t channels, uint32_t bits_per_sample,
                                     double multiplier, uint32_t chunk_frames,
                                     const uint8_t *d_dither, uint64_t dither_bit0,
                                     void *stream);
atg_status atg_pcm_apply_gain_host(int device, const int32_t *in, int32_t *out,
                                   uint64_t frames, uint32_t channels,
                                   uint32_t bits_per_sample, double multiplier,
                                   uint32_t chunk_frames, const uint8_t *dither,
                                   uint64_t dither_bytes, uint64_t dither_bit0);

/* ------------------------------------------------------------------ */
/* ALAC encoder (E1-E7).  Replaces the body of the reference's          */
/* audiotools.encoders.encode_alac (src/encoders/alac.c:30-206:         */
/* ALACEncoder_encode_alac -> write_frameset / write_frame /            */
/* compute_coefficients / calculate_residuals / encode_residuals) for a */
/* batch of tracks; audiotools.m4a.ALACAudio.from_pcm wraps the mdat in */
/* the M4A atoms on the host.  Interlacing shift 2; leftweights        */
/* minimum..maximum_interlacing_leftweight (0..4 by default,            */
/* alac.c:57-72; 0 <= min <= max <= 255, others ATG_ERR_INVALID).       */
/* ------------------------------------------------------------------ */
typedef struct {
    uint32_t block_size;         /* PCM frames per frameset, 1..65535 */
    uint32_t initial_history;    /* encode_alac keyword arguments     */
    uint32_t history_multiplier;
    uint32_t maximum_k;
    uint32_t minimum_interlacing_leftweight;
    uint32_t maximum_interlacing_leftweight;
} atg_alac_options;

/* Per-track result: the mdat atom (32-bit size, "mdat", framesets) is
   `bytes` long at out + out_offset; frameset_bytes[first_frameset ..
   first_frameset + n_framesets) is the frame-size log encode_alac returns
   (alac.c:150-151, 1255-1290). */
typedef struct {
    uint64_t out_offset;
    uint64_t bytes;
    uint64_t pcm_frames;
    uint32_t first_frameset;
    uint32_t n_framesets;
    int32_t status;
    uint32_t reserved;
} atg_alac_track_result;

typedef struct atg_alac_encoder atg_alac_encoder;

const char *atg_alac_last_error(void);
atg_status atg_alac_encoder_create(int device, atg_alac_encoder **out);
void atg_alac_encoder_destroy(atg_alac_encoder *enc);
/* framesets and worst-case output bytes of a batch (tracks as for FLAC:
   block_size frames + a short last one, or explicit frame_sizes) */
atg_status atg_alac_batch_bounds(atg_alac_encoder *enc, const atg_alac_options *opts,
                                 const atg_track *tracks, uint32_t n_tracks, uint32_t channels,
                                 uint32_t bits_per_sample, uint64_t *total_framesets,
                                 uint64_t *out_bytes);
/* PCM and output in device memory (d_out 4-byte aligned, out_cap >= the
   bound); frameset_bytes (host, total_framesets entries) may be NULL */
atg_status atg_alac_encode_device(atg_alac_encoder *enc, const atg_alac_options *opts,
                                  const void *d_pcm, atg_pcm_format format,
                                  const atg_track *tracks, uint32_t n_tracks,
                                  uint32_t channels, uint32_t bits_per_sample, void *d_out,
                                  uint64_t out_cap, atg_alac_track_result *results,
                                  uint32_t *frameset_bytes);
/* the same for host buffers (staged through the device) */
atg_status atg_alac_encode_host(atg_alac_encoder *enc, const atg_alac_options *opts,
                                const void *pcm, atg_pcm_format format, const atg_track *tracks,
                                uint32_t n_tracks, uint32_t channels, uint32_t bits_per_sample,
                                uint8_t *out, uint64_t out_cap, atg_alac_track_result *results,
                                uint32_t *frameset_bytes);
int atg_alac_encoder_kernel_times(atg_alac_encoder *enc, const char **names, float *ms, int cap);

/* ------------------------------------------------------------------ */
/* ALAC decoder (D6).  Replaces the reference's                        */
/* audiotools.decoders.ALACDecoder (src/decoders/alac.c: init          */
/* :25-98 with parse_decoding_parameters :439-672 and seek_mdat        */
/* :953-971, read() :183-254, read_frame :818-951, read_residuals       */
/* :1017-1085, decode_subframe :1147-1235, decorrelate_channels         */
/* :1237-1259, alac_order_to_wave_order :709-816) for a batch of M4A    */
/* images.                                                             */
/* ------------------------------------------------------------------ */
/* status values: the reference's decoder status enum (decoders/alac.h)
   plus the conditions its Python methods raise */
enum {
    ATG_AD_OK = 0,
    ATG_AD_IO_ERROR = 1,           /* IOError ("I/O Errror" at init,
                                      "EOF during frame reading" in read) */
    ATG_AD_INVALID_UNUSED_BITS = 2,/* ValueError "invalid unused bits" */
    ATG_AD_INVALID_ALAC_ATOM = 3,
    ATG_AD_INVALID_MDHD_ATOM = 4,
    ATG_AD_MDIA_NOT_FOUND = 5,
    ATG_AD_STSD_NOT_FOUND = 6,
    ATG_AD_MDHD_NOT_FOUND = 7,
    ATG_AD_INVALID_SEEKTABLE = 8,
    ATG_AD_NO_MDAT = 9,            /* IOError "Unable to locate 'mdat' atom" */
    ATG_AD_CHANNEL_MISMATCH = 10   /* ValueError "channel length mismatch" */
};

/* the "alac" / "mdhd" fields the decoder keeps, and where "mdat" starts */
typedef struct {
    uint32_t max_samples_per_frame, bits_per_sample, history_multiplier, initial_history;
    uint32_t maximum_k, channels, sample_rate, total_frames;
    uint64_t mdat_offset;   /* byte (from the image start) of the first frameset */
    uint32_t n_seekpoints;  /* entries of the stts/stsc/stco seektable */
    uint32_t reserved;
} atg_alac_info;

typedef struct {
    uint64_t pcm_frames_offset, file_offset;
} atg_alac_seekpoint;

/* parse_decoding_parameters + seek_mdat over an in-memory image (host):
   returns an ATG_AD_* status.  Seekpoints (sp_cap) and the stsz frameset
   sizes (fs_cap, a decoding hint the reference does not read) are copied
   when the buffers are non-NULL. */
int atg_alac_read_info(const uint8_t *data, uint64_t len, atg_alac_info *info,
                       atg_alac_seekpoint *sp, uint32_t sp_cap, uint32_t *frame_sizes,
                       uint32_t fs_cap, uint32_t *n_frame_sizes);

/* One stream of a decode batch: the image at data[data_offset,
   data_offset + data_bytes) (4-byte aligned); reading starts at byte
   `start` of the image (the mdat offset, or a seekpoint's file offset) with
   remaining_frames = `remaining`.  frameset_bytes: the stsz sizes from
   `start` on (may be NULL: framesets are then found by the serial walk). */
typedef struct {
    uint64_t data_offset, data_bytes, start, remaining;
    uint32_t max_samples_per_frame, bits_per_sample, history_multiplier, initial_history;
    uint32_t maximum_k, channels;
    const uint32_t *frameset_bytes;
    uint64_t n_frameset_bytes;
} atg_alac_dec_track;

/* read() view: n_framesets framesets = pcm_frames PCM frames (interleaved
   int32 in wave channel order at sample index sample_offset of the batch
   output) are returned, then `status` ends the stream (0 = remaining_frames
   reached 0). */
typedef struct {
    uint64_t sample_offset;
    uint64_t pcm_frames;
    uint32_t first_frameset;
    uint32_t n_framesets;
    int32_t status;
    uint32_t channels;
} atg_alac_dec_result;

typedef struct atg_alac_decoder atg_alac_decoder;

const char *atg_alac_decoder_last_error(void);
atg_status atg_alac_decoder_create(int device, atg_alac_decoder **out);
void atg_alac_decoder_destroy(atg_alac_decoder *dec);
atg_status atg_alac_decode_host(atg_alac_decoder *dec, const uint8_t *data, uint64_t len,
                                const atg_alac_dec_track *tracks, uint32_t n_tracks,
                                atg_alac_dec_result *results, uint64_t *total_samples,
                                uint64_t *total_framesets);
/* the last decode's PCM and, per frameset, its PCM frames and its byte
   offset from the image start */
atg_status atg_alac_decode_fetch(atg_alac_decoder *dec, int32_t *pcm, uint64_t pcm_cap,
                                 uint32_t *frameset_frames, uint64_t *frameset_offsets,
                                 uint64_t fs_cap);
atg_status atg_alac_decode_device(atg_alac_decoder *dec, const void *d_data, uint64_t len,
                                  const atg_alac_dec_track *tracks, uint32_t n_tracks,
                                  atg_alac_dec_result *results, const int32_t **d_pcm,
                                  uint64_t *total_samples);
int atg_alac_decoder_kernel_times(atg_alac_decoder *dec, const char **names, float *ms,
                                  int cap);

/* ------------------------------------------------------------------ */
/* True Audio (TTA1) encoder.  Replaces the body of the reference's     */
/* audiotools.encoders.encode_tta (src/encoders/tta.c:31-114 ->         */
/* encode_frame :144-259) for a batch of tracks of one format.  Every   */
/* block of sample_rate * 256 / 245 PCM frames (or every explicit       */
/* atg_track frame size) becomes one TTA frame: the Rice payload and    */
/* its CRC-32.  The output holds frames only; the 22-byte header and    */
/* the seektable are host work (audiotools/tta.py).  bits_per_sample    */
/* 8, 16 or 24.  There are no encoder options.                          */
/* ------------------------------------------------------------------ */
/* Per-track result: the track's frames are `bytes` long at out +
   out_offset; frame_bytes[first_frame .. first_frame + n_frames) are the
   frame sizes including each frame's CRC: the seektable body and the list
   encode_tta returns. */
typedef struct {
    uint64_t out_offset;
    uint64_t bytes;
    uint64_t pcm_frames;
    uint32_t first_frame;
    uint32_t n_frames;
    int32_t status;
    uint32_t reserved;
} atg_tta_track_result;

typedef struct atg_tta_encoder atg_tta_encoder;

const char *atg_tta_last_error(void);
atg_status atg_tta_encoder_create(int device, atg_tta_encoder **out);
void atg_tta_encoder_destroy(atg_tta_encoder *enc);
/* PCM and output in device memory (d_out 4-byte aligned).  A TTA frame has
   no useful size bound before it is encoded (a loud sample after a quiet
   passage costs a unary run as long as its value), so there is no
   batch_bounds call: the code lengths are computed first, *needed (may be
   NULL) receives the bytes the batch takes, and when that exceeds out_cap
   the call returns ATG_ERR_CAPACITY with nothing written to d_out: call
   again with a buffer of *needed bytes.  *needed counts output bytes
   only.  frame_bytes (host, frame_bytes_cap entries, may be NULL)
   receives the frame sizes; fewer entries than the batch has frames
   (ceil(pcm_frames / block) per track, or its explicit frame sizes) is
   ATG_ERR_INVALID. */
atg_status atg_tta_encode_device(atg_tta_encoder *enc, const void *d_pcm, atg_pcm_format format,
                                 const atg_track *tracks, uint32_t n_tracks, uint32_t channels,
                                 uint32_t bits_per_sample, uint32_t sample_rate, void *d_out,
                                 uint64_t out_cap, atg_tta_track_result *results,
                                 uint32_t *frame_bytes, uint64_t frame_bytes_cap,
                                 uint64_t *needed);
/* the same for host buffers (staged through the device) */
atg_status atg_tta_encode_host(atg_tta_encoder *enc, const void *pcm, atg_pcm_format format,
                               const atg_track *tracks, uint32_t n_tracks, uint32_t channels,
                               uint32_t bits_per_sample, uint32_t sample_rate, uint8_t *out,
                               uint64_t out_cap, atg_tta_track_result *results,
                               uint32_t *frame_bytes, uint64_t frame_bytes_cap,
                               uint64_t *needed);
/* the last encode: "tta_chain", "tta_size" (from the chain's end to the
   pack's start: the totals copied to the host, the extents, the clearing of
   the output), "tta_pack", "tta_crc" and "tta_total", first kernel to last */
int atg_tta_encoder_kernel_times(atg_tta_encoder *enc, const char **names, float *ms, int cap);

/* ------------------------------------------------------------------ */
/* True Audio decoder.  Replaces the reference's                        */
/* audiotools.decoders.TTADecoder (src/decoders/tta.c) for a batch of   */
/* images.                                                             */
/* ------------------------------------------------------------------ */
/* status values: the reference's decoder status enum (decoders/tta.h),
   plus the frame-read failure TTADecoder_read reports on its own */
enum {
    ATG_TD_OK = 0,
    ATG_TD_IO_ERROR = 1,           /* IOError "I/O error reading header" /
                                      "... seektable" / "... frame" */
    ATG_TD_CRC_MISMATCH = 2,       /* ValueError "CRC error reading header" /
                                      "... seektable", "CRC mismatch reading frame" */
    ATG_TD_INVALID_SIGNATURE = 3,  /* ValueError "invalid header signature" */
    ATG_TD_UNSUPPORTED_FORMAT = 4, /* ValueError "unsupported TTA format" */
    ATG_TD_FRAME_READ = 5          /* ValueError "I/O error during frame read":
                                      the Rice stream ran past its payload */
};

typedef struct {
    uint32_t channels, bits_per_sample, sample_rate, total_pcm_frames;
    uint32_t block_size;       /* sample_rate * 256 / 245 */
    uint32_t total_tta_frames; /* ceil(total_pcm_frames / block_size) */
    uint64_t id3_bytes;        /* ID3v2 comments skipped in front of "TTA1" */
    uint64_t frames_offset;    /* byte (from the image start) of the first frame */
    uint32_t stage;            /* how far parsing got: 0 header, 1 seektable, 2 done */
    uint32_t reserved;
} atg_tta_info;

/* read_header + read_seektable over an in-memory image (host): returns an
   ATG_TD_* status, info->stage telling a header failure from a seektable
   failure.  Both CRCs are checked; ID3v2 comments in front are skipped.
   The seektable's frame sizes are copied to frame_bytes (cap entries, may
   be NULL); *n_frame_bytes receives their number. */
int atg_tta_read_info(const uint8_t *data, uint64_t len, atg_tta_info *info,
                      uint32_t *frame_bytes, uint32_t cap, uint32_t *n_frame_bytes);

/* One stream of a decode batch: the image at data[data_offset, data_offset +
   data_bytes) (4-byte aligned); reading starts at byte `start` of the image
   (frames_offset, or a later frame's offset) with `remaining` PCM frames
   left; frame_bytes are the seektable entries from that frame on. */
typedef struct {
    uint64_t data_offset, data_bytes, start, remaining;
    uint32_t channels, bits_per_sample, block_size, reserved;
    const uint32_t *frame_bytes;
    uint64_t n_frame_bytes;
} atg_tta_dec_track;

/* n_frames frames = pcm_frames PCM frames (interleaved int32 at sample
   index sample_offset of the batch output) decoded, then `status` ends the
   stream: 0 when `remaining` was reached, else the status of the track's
   frame number n_frames (the first bad one). */
typedef struct {
    uint64_t sample_offset;
    uint64_t pcm_frames;
    uint32_t first_frame;
    uint32_t n_frames;
    int32_t status;
    uint32_t channels;
} atg_tta_dec_result;

typedef struct atg_tta_decoder atg_tta_decoder;

const char *atg_tta_decoder_last_error(void);
atg_status atg_tta_decoder_create(int device, atg_tta_decoder **out);
void atg_tta_decoder_destroy(atg_tta_decoder *dec);
atg_status atg_tta_decode_host(atg_tta_decoder *dec, const uint8_t *data, uint64_t len,
                               const atg_tta_dec_track *tracks, uint32_t n_tracks,
                               atg_tta_dec_result *results, uint64_t *total_samples);
/* the last decode's PCM (total_samples int32) */
atg_status atg_tta_decode_fetch(atg_tta_decoder *dec, int32_t *pcm, uint64_t pcm_cap);
/* image in device memory (4-byte aligned); *d_pcm is the decoder's own
   buffer, valid until its next call */
atg_status atg_tta_decode_device(atg_tta_decoder *dec, const void *d_data, uint64_t len,
                                 const atg_tta_dec_track *tracks, uint32_t n_tracks,
                                 atg_tta_dec_result *results, const int32_t **d_pcm,
                                 uint64_t *total_samples);
/* "ttad_crc", "ttad_parse", "ttad_chain", "ttad_out", "ttad_total" */
int atg_tta_decoder_kernel_times(atg_tta_decoder *dec, const char **names, float *ms,
                                 int cap);

/* ------------------------------------------------------------------ */
/* WavPack decoder.  Replaces the reference's                           */
/* audiotools.decoders.WavPackDecoder (src/decoders/wavpack.c) for a    */
/* batch of images.  Lossless integer streams (no hybrid, no float).   */
/* ------------------------------------------------------------------ */
/* status values: the reference's status enum (decoders/wavpack.h) with its
   message strings (wavpack_strerror), then what its callers report on their
   own, then the layout check the reference does not make */
enum {
    ATG_WVD_OK = 0,
    ATG_WVD_IO_ERROR = 1,                        /* IOError "I/O error" */
    ATG_WVD_SUB_BLOCK_NOT_FOUND = 2,             /* internal */
    ATG_WVD_INVALID_BLOCK_ID = 3,                /* "invalid block header ID" */
    ATG_WVD_INVALID_RESERVED_BIT = 4,            /* "invalid reserved bit" */
    ATG_WVD_EXCESSIVE_DECORRELATION_PASSES = 5,  /* "excessive decorrelation passes" */
    ATG_WVD_INVALID_DECORRELATION_TERM = 6,      /* "invalid decorrelation term" */
    ATG_WVD_DECORRELATION_TERMS_MISSING = 7,     /* "missing decorrelation terms sub block" */
    ATG_WVD_DECORRELATION_WEIGHTS_MISSING = 8,   /* "missing decorrelation weights sub block" */
    ATG_WVD_DECORRELATION_SAMPLES_MISSING = 9,   /* "missing decorrelation samples sub block" */
    ATG_WVD_ENTROPY_VARIABLES_MISSING = 10,      /* "missing entropy variables sub block" */
    ATG_WVD_RESIDUALS_MISSING = 11,              /* "missing bitstream sub block" */
    ATG_WVD_EXTENDED_INTEGERS_MISSING = 12,      /* "missing extended integers sub block" */
    ATG_WVD_EXCESSIVE_DECORRELATION_WEIGHTS = 13, /* "excessive decorrelation weight values" */
    ATG_WVD_INVALID_ENTROPY_VARIABLE_COUNT = 14, /* "invalid entropy variable count" */
    ATG_WVD_BLOCK_DATA_CRC_MISMATCH = 15,        /* "block data CRC mismatch" */
    ATG_WVD_BLOCK_DATA_IO = 16,      /* IOError "I/O error reading block data": the file
                                        ends inside a block */
    ATG_WVD_INCONSISTENT_BLOCK = 17, /* ValueError "inconsistent block header": a set's
                                        blocks do not add up to the channel count, disagree
                                        on block_samples, do not continue the set before,
                                        claim more than the stream has left or more
                                        than 2^31 - 1 frames (the reference trusts
                                        the headers here) */
    ATG_WVD_MD5_MISMATCH = 18,       /* ValueError "MD5 mismatch at end of stream" */
    ATG_WVD_SAMPLE_RATE_UNDEFINED = 19, /* ValueError "sample rate undefined" */
    ATG_WVD_CHANNELS_UNDEFINED = 20     /* ValueError "channel count/mask undefined":
                                           no channel-info sub-block, or one that
                                           declares 0 channels */
};

typedef struct {
    uint32_t sample_rate, bits_per_sample, channels, channel_mask;
    uint32_t total_pcm_frames;
    uint32_t n_sets;      /* complete, consistent block sets in the table */
    uint32_t n_blocks;    /* blocks in the table: those of the sets, then tail_blocks */
    uint32_t tail_blocks; /* readable blocks of the set a bad header or the end of the
                             file stopped in: decoded for their status only */
    int32_t end_status;   /* what ends the stream after the sets (0: the declared total) */
    uint32_t has_md5;     /* a 16-byte MD5 sub-block follows the audio */
    uint8_t md5[16];
    uint64_t end_offset;  /* byte after the last set */
} atg_wv_info;

/* one audio block: the 32-byte header is at `offset` of the image, `size`
   bytes of sub-blocks follow it */
typedef struct {
    uint64_t offset;
    uint32_t size;
    uint32_t block_index, block_samples;
    uint32_t flags; /* the header's flag word: mono 1<<2, joint stereo 1<<4, extended
                       integers 1<<8, initial 1<<11, final 1<<12, false stereo 1<<30 */
    uint32_t crc;
    uint32_t set;           /* the set (PCM frame range over all channels) it belongs to */
    uint32_t first_channel; /* its first channel within the set */
    uint32_t reserved;
} atg_wv_block;

/* WavPackDecoder_init and the header walk of the read loop over an
   in-memory image (host).  Returns an ATG_WVD_* status: non-zero where the
   reference fails to initialise.  The table ends before the first set that
   a header error, the end of the file or a layout check stops
   (info->end_status).  Up to cap blocks are written (blocks may be NULL);
   *n_blocks receives their number. */
int atg_wv_read_info(const uint8_t *data, uint64_t len, atg_wv_info *info,
                     atg_wv_block *blocks, uint32_t cap, uint32_t *n_blocks);

/* One stream of a decode batch: the image at data[data_offset, data_offset +
   data_bytes) (4-byte aligned) and its table from atg_wv_read_info, or the
   part of it from a later set on.  The table is checked again: a table that
   contradicts itself is ATG_ERR_INVALID. */
typedef struct {
    uint64_t data_offset, data_bytes;
    const atg_wv_block *blocks;
    uint32_t n_blocks, tail_blocks;
    uint32_t channels, bits_per_sample;
    int32_t end_status;
    /* compare the MD5 of the PCM's file byte form (clamped to the width, little
       endian) with md5 when every set decoded: 1 signed at every width, as the
       reference's standalone decoder hashes; 2 with 8-bit samples unsigned, as
       WavPackDecoder_update_md5sum and the reference's encoder do; 0 no check */
    uint32_t check_md5;
    uint8_t md5[16];
} atg_wv_dec_track;

/* n_sets sets = pcm_frames PCM frames (interleaved int32 at sample index
   sample_offset of the batch output) decoded, then `status` ends the
   stream: 0, or the status of the track's set number n_sets (the first bad
   one), or ATG_WVD_MD5_MISMATCH with all PCM delivered. */
typedef struct {
    uint64_t sample_offset;
    uint64_t pcm_frames;
    uint32_t n_sets;
    int32_t status;
    uint32_t channels;
    uint32_t reserved;
} atg_wv_dec_result;

typedef struct atg_wv_decoder atg_wv_decoder;

const char *atg_wv_decoder_last_error(void);
atg_status atg_wv_decoder_create(int device, atg_wv_decoder **out);
void atg_wv_decoder_destroy(atg_wv_decoder *dec);
atg_status atg_wv_decode_host(atg_wv_decoder *dec, const uint8_t *data, uint64_t len,
                              const atg_wv_dec_track *tracks, uint32_t n_tracks,
                              atg_wv_dec_result *results, uint64_t *total_samples);
/* the last decode's PCM (total_samples int32) */
atg_status atg_wv_decode_fetch(atg_wv_decoder *dec, int32_t *pcm, uint64_t pcm_cap);
/* images in device memory (4-byte aligned); *d_pcm is the decoder's own
   buffer, valid until its next call */
atg_status atg_wv_decode_device(atg_wv_decoder *dec, const void *d_data, uint64_t len,
                                const atg_wv_dec_track *tracks, uint32_t n_tracks,
                                atg_wv_dec_result *results, const int32_t **d_pcm,
                                uint64_t *total_samples);
/* "wvd_parse", "wvd_decorr", "wvd_out", "wvd_total" */
int atg_wv_decoder_kernel_times(atg_wv_decoder *dec, const char **names, float *ms, int cap);

/* ------------------------------------------------------------------ */
/* WavPack encoder.  Replaces the body of the reference's               */
/* audiotools.encoders.encode_wavpack (src/encoders/wavpack.c) for a    */
/* batch of tracks of one format.  Every block_size PCM frames become   */
/* one block per channel group (mono and stereo: one; more channels are */
/* split by channel_mask as init_context does: 0x7 2+1, 0x33 2+2, 0x107 */
/* 2+1+1, 0x37 2+1+2, 0x3F 2+1+1+2, anything else channel by channel).  */
/* A track's output is the complete .wv image: the blocks, the RIFF     */
/* header sub-block in the first of them, the footer block with the MD5 */
/* of the PCM, total_samples set in every header.  bits_per_sample 8,   */
/* 16 or 24.  No foreign RIFF chunks, tags, hybrid or float modes.      */
/* ------------------------------------------------------------------ */
typedef struct {
    uint32_t block_size;         /* PCM frames per block, at least 1 */
    uint32_t correlation_passes; /* 0, 1, 2, 5, 10 or 16 */
    uint32_t false_stereo;       /* code a stereo block whose channels are equal as one */
    uint32_t wasted_bits;        /* shift out low bits that are zero throughout a block */
    uint32_t joint_stereo;       /* mid/side for two-channel blocks */
} atg_wv_enc_options;

/* Per-track result: the image is `bytes` long at out + out_offset;
   block_bytes[first_block .. first_block + n_blocks) are the sizes of its
   audio blocks, headers included, in file order (the footer block of 50
   bytes follows them).  md5 is the digest of the PCM as the file's footer
   holds it: little endian at the sample width, 8-bit samples unsigned. */
typedef struct {
    uint64_t out_offset;
    uint64_t bytes;
    uint64_t pcm_frames;
    uint32_t first_block;
    uint32_t n_blocks;
    int32_t status;
    uint32_t reserved;
    uint8_t md5[16];
} atg_wv_track_result;

typedef struct atg_wv_encoder atg_wv_encoder;

const char *atg_wv_encoder_last_error(void);
atg_status atg_wv_encoder_create(int device, atg_wv_encoder **out);
void atg_wv_encoder_destroy(atg_wv_encoder *enc);
/* PCM and output in device memory.  A block has no useful size bound before
   it is encoded, so, as for TTA, the lengths are computed first: *needed
   (may be NULL) receives the bytes the batch takes, and when that exceeds
   out_cap the call returns ATG_ERR_CAPACITY with nothing written to d_out.
   block_bytes (host, block_bytes_cap entries, may be NULL) receives the
   block sizes; fewer entries than the batch has blocks is ATG_ERR_INVALID.
   ATG_ERR_INVALID: bits other than 8, 16, 24; 0 channels; passes outside
   {0, 1, 2, 5, 10, 16}; block_size 0; with passes, a block_size below the
   history depth of any stream's pass table (stereo 16: 8, 10: 5, 5: 3; mono
   5, 10, 16: 3; 1 and 2: 2), where the reference aborts on any block but
   the last once it is shorter than a term 1..8 -- a track no longer than
   such a block is refused too, which the reference would encode; a track
   of 2^32 - 1 frames or more.
   ATG_ERR_UNSUPPORTED: tracks with explicit frame_sizes; more than 255
   channels. */
atg_status atg_wv_encode_device(atg_wv_encoder *enc, const void *d_pcm, atg_pcm_format format,
                                const atg_track *tracks, uint32_t n_tracks, uint32_t channels,
                                uint32_t channel_mask, uint32_t bits_per_sample,
                                uint32_t sample_rate, const atg_wv_enc_options *options,
                                void *d_out, uint64_t out_cap, atg_wv_track_result *results,
                                uint32_t *block_bytes, uint64_t block_bytes_cap,
                                uint64_t *needed);
/* the same for host buffers (staged through the device) */
atg_status atg_wv_encode_host(atg_wv_encoder *enc, const void *pcm, atg_pcm_format format,
                              const atg_track *tracks, uint32_t n_tracks, uint32_t channels,
                              uint32_t channel_mask, uint32_t bits_per_sample,
                              uint32_t sample_rate, const atg_wv_enc_options *options,
                              uint8_t *out, uint64_t out_cap, atg_wv_track_result *results,
                              uint32_t *block_bytes, uint64_t block_bytes_cap, uint64_t *needed);
/* the last encode: "wv_prep", "wv_chain", "wv_md5", "wv_size" (from the
   digests' end to the pack's start: the block table copied to the host, the
   extents, their upload), "wv_pack" (with the footers) and "wv_total", first
   kernel to last */
int atg_wv_encoder_kernel_times(atg_wv_encoder *enc, const char **names, float *ms, int cap);

/* ------------------------------------------------------------------ */
/* Sinc resampler (R1-R3, track2track --sample-rate).  Replaces the     */
/* reference's audiotools.pcmconverter.Resampler (src/pcmconverter.c    */
/* :370-495: src_new(SRC_SINC_BEST_QUALITY) + src_process per 4096-frame */
/* read, libsamplerate 0.1.8 src/samplerate/src_sinc.c) for whole       */
/* tracks.  Coefficients: the MEDIUM table (BEST's table is absent from */
/* the reference tree; parity is against oracle/resample_port.c).      */
/* PCM is interleaved int32 (FrameList layout), 1..8 channels, 1..24    */
/* bits, in and out (the output keeps bits_per_sample).                 */
/* ------------------------------------------------------------------ */
typedef struct {
    uint64_t pcm_offset;  /* first frame of the track in the input buffer */
    uint64_t pcm_frames;
    uint32_t in_rate, out_rate;
    /* frame counts the wrapped PCMReader's read(4096) calls returned (they
       sum to pcm_frames; NULL = 4096-frame reads).  They can move the end
       of the stream by one frame in rare ties (atg_resample_read_sizes). */
    const uint32_t *reads;
    uint64_t n_reads;
} atg_rs_track;

const char *atg_resample_last_error(void);
/* output frames of one track read in 4096-frame reads (the converter's
   termination rule) */
uint64_t atg_resample_output_frames(uint64_t in_frames, uint32_t channels, uint32_t in_rate,
                                    uint32_t out_rate);
/* Device buffers.  Track t's output is written at frame out_offsets[t]
   (host array, filled) of d_out, out_frames[t] frames; out_cap_samples
   >= the sum of atg_resample_output_frames() x channels.  Returns after
   the stream has drained. */
atg_status atg_resample_device(const atg_rs_track *tracks, uint32_t n, uint32_t channels,
                               uint32_t bits_per_sample, const int32_t *d_in, int32_t *d_out,
                               uint64_t out_cap_samples, uint64_t *out_offsets,
                               uint64_t *out_frames, void *stream);
/* Host buffers (staged through the device). */
atg_status atg_resample_host(int device, const atg_rs_track *tracks, uint32_t n,
                             uint32_t channels, uint32_t bits_per_sample, const int32_t *in,
                             uint64_t in_samples, int32_t *out, uint64_t out_cap_samples,
                             uint64_t *out_offsets, uint64_t *out_frames);
/* The frame counts successive Resampler.read() calls return (the last is
   the 0 that ends the stream), given the frame counts the wrapped reader's
   read(4096) calls returned (`reads`, its terminating 0 excluded).
   Returns the number of counts (written up to cap), or -1. */
int64_t atg_resample_read_sizes(uint64_t in_frames, uint32_t channels, uint32_t in_rate,
                                uint32_t out_rate, const uint32_t *reads, uint64_t n_reads,
                                uint32_t *sizes, uint64_t cap);
/* durations (ms) of the last atg_resample_device call's kernels on the
   calling thread's device: "rs_positions" (0 when every track had a closed
   form) and "rs_filter" */
int atg_resample_kernel_times(const char **names, float *ms, int cap);

/* -------------------------------------------------------------------- */
/* Shorten (.shn).  Replaces the reference's audiotools.encoders.       */
/* encode_shn (src/encoders/shn.c) and audiotools.decoders.SHNDecoder   */
/* (src/decoders/shn.c) for a batch of tracks.  A .shn file is one      */
/* MSB-first bit stream with no frame table, block sizes, CRC or sample */
/* count.                                                               */
/* -------------------------------------------------------------------- */
/* The limits.  The encoder takes block sizes (and explicit frame sizes) up
   to ATG_SHN_MAX_ENCODE_BLOCK, where the reference's unsigned delta sums
   cannot wrap (|delta3| < 2^19, 2^19 x 4096 = 2^31).  The decoder ends a
   stream with ATG_SHN_UNSUPPORTED where the reference's behaviour is
   undefined or unbounded: channels 0 or above ATG_SHN_MAX_CHANNELS, a mean
   count above ATG_SHN_MAX_MEAN_COUNT, an audio command with block length 0
   (shnmean divides by it), DIFF0 or QLPC with mean count 0 (the same
   division), a block length that changes inside a set of channels, a shift
   or an energy above 31, a "long" wider than 32 bits, an LPC count above
   ATG_SHN_MAX_LPC_COUNT, or more than ATG_SHN_MAX_TRACK_SAMPLES decoded
   samples (a ZERO command is 5 bits and can claim 2^32 of them). */
#define ATG_SHN_MAX_ENCODE_BLOCK 4096u
#define ATG_SHN_MAX_CHANNELS 256u
#define ATG_SHN_MAX_LPC_COUNT 32u
#define ATG_SHN_MAX_MEAN_COUNT 64u
#define ATG_SHN_MAX_TRACK_SAMPLES (1ull << 28)

/* the reference's decoder status enum (decoders/shn.h) with the messages
   SHNDecoder raises, plus one of this library's own */
typedef enum {
    ATG_SHN_OK = 0,
    ATG_SHN_END_OF_STREAM = 1,           /* the stream ended with QUIT */
    ATG_SHN_IOERROR = 2,                 /* IOError "I/O error reading Shorten file"
                                            (header: "I/O error reading Shorten header") */
    ATG_SHN_UNKNOWN_COMMAND = 3,         /* ValueError "unknown command in Shorten stream" */
    ATG_SHN_INVALID_MAGIC_NUMBER = 4,    /* ValueError "invalid magic number" */
    ATG_SHN_INVALID_SHORTEN_VERSION = 5, /* ValueError "invalid Shorten version" */
    ATG_SHN_UNSUPPORTED_FILE_TYPE = 6,   /* ValueError "unsupported Shorten file type" */
    ATG_SHN_UNSUPPORTED = 7              /* outside the limits above */
} atg_shn_status;

typedef struct {
    uint32_t block_size;     /* 1..ATG_SHN_MAX_ENCODE_BLOCK; the reference's default is 256 */
    int32_t is_big_endian;   /* recorded in the file type only */
    int32_t signed_samples;  /* 0: 1 << (bits - 1) is added to every sample */
    uint32_t reserved;
} atg_shn_options;

/* the bytes of a track's VERBATIM commands: the header one is always
   written, the footer one when footer_bytes > 0 */
typedef struct {
    const uint8_t *header;
    uint64_t header_bytes;
    const uint8_t *footer;
    uint64_t footer_bytes;
} atg_shn_track_data;

typedef struct {
    uint64_t out_offset; /* 4-byte aligned */
    uint64_t bytes;      /* the whole .shn image; always 1 mod 4 */
    uint64_t pcm_frames;
    uint32_t n_blocks;
    uint32_t reserved;
} atg_shn_track_result;

typedef struct atg_shn_encoder atg_shn_encoder;

const char *atg_shn_encoder_last_error(void);
atg_status atg_shn_encoder_create(int device, atg_shn_encoder **out);
void atg_shn_encoder_destroy(atg_shn_encoder *enc);
/* PCM and output in device memory (d_out 4-byte aligned).  Every track
   becomes a whole .shn image at results[t].out_offset; a track's atg_track
   frame sizes are the lengths of the reader's short reads (a BLOCKSIZE
   command where the length changes).  `extra` holds n_tracks entries or is
   NULL.  Sizes are known only after a length pass: *needed (may be NULL)
   receives the bytes the batch takes, rounded up to 4, and ATG_ERR_CAPACITY
   is returned, with nothing written, when out_cap is less.  bits_per_sample
   other than 8 or 16 is ATG_ERR_INVALID (the reference's ValueError
   "unsupported bits per sample"), a block size above
   ATG_SHN_MAX_ENCODE_BLOCK ATG_ERR_UNSUPPORTED. */
atg_status atg_shn_encode_device(atg_shn_encoder *enc, const void *d_pcm, atg_pcm_format format,
                                 const atg_track *tracks, const atg_shn_track_data *extra,
                                 uint32_t n_tracks, uint32_t channels, uint32_t bits_per_sample,
                                 const atg_shn_options *options, void *d_out, uint64_t out_cap,
                                 atg_shn_track_result *results, uint64_t *needed);
/* Host buffers (staged through the device). */
atg_status atg_shn_encode_host(atg_shn_encoder *enc, const void *pcm, atg_pcm_format format,
                               const atg_track *tracks, const atg_shn_track_data *extra,
                               uint32_t n_tracks, uint32_t channels, uint32_t bits_per_sample,
                               const atg_shn_options *options, uint8_t *out, uint64_t out_cap,
                               atg_shn_track_result *results, uint64_t *needed);
/* the last encode: "shn_size", "shn_scan", "shn_layout" (the host between
   the scan and the pack), "shn_pack", "shn_edges" and "shn_total" */
int atg_shn_encoder_kernel_times(atg_shn_encoder *enc, const char **names, float *ms, int cap);

typedef struct {
    uint32_t file_type, channels, block_length, max_lpc, mean_count, bytes_to_skip;
    uint32_t bits_per_sample;
    uint32_t signed_samples;
    uint32_t sample_rate;  /* from a RIFF/WAVE fmt or AIFF COMM chunk in a leading
                              VERBATIM, else 44100 */
    uint32_t channel_mask; /* likewise, else 0 */
    uint64_t total_pcm_frames;  /* from that VERBATIM's data / SSND chunk size, as the
                                   reference's audiotools/shn.py computes it; else 0 */
    uint64_t first_command_bit; /* where the commands start */
} atg_shn_info;

/* read_shn_header on the host: returns an atg_shn_status (ATG_SHN_OK with
   *info filled, or the header's error). */
int atg_shn_read_info(const uint8_t *data, uint64_t len, atg_shn_info *info);

/* one stream of a decode batch: its image in the data (4-byte aligned
   offset) and the header fields atg_shn_read_info returned */
typedef struct {
    uint64_t data_offset;
    uint64_t data_bytes;
    uint64_t first_command_bit;
    uint32_t file_type, channels, block_length, max_lpc, mean_count;
    uint32_t reserved;
} atg_shn_dec_track;

/* status: ATG_SHN_END_OF_STREAM for a stream that ended with QUIT, else why
   it stopped; its PCM then ends before the first incomplete set of channels.
   The VERBATIM bytes (what pcm_split returns) are those in front of and
   after the first audio command, header first, at verbatim_offset of the
   bytes atg_shn_decode_fetch_verbatim copies. */
typedef struct {
    uint64_t pcm_offset; /* in samples, of the batch's int32 PCM */
    uint64_t pcm_frames;
    uint64_t verbatim_offset;
    uint32_t header_bytes, footer_bytes;
    int32_t status;
    uint32_t reserved;
} atg_shn_dec_result;

typedef struct atg_shn_decoder atg_shn_decoder;

const char *atg_shn_decoder_last_error(void);
atg_status atg_shn_decoder_create(int device, atg_shn_decoder **out);
void atg_shn_decoder_destroy(atg_shn_decoder *dec);
/* the index pass walks a stream's residual codes with the whole wave
   (cooperative != 0, the default) or with the lane-serial walker */
atg_status atg_shn_decoder_set_index_walk(atg_shn_decoder *dec, int cooperative);
atg_status atg_shn_decode_host(atg_shn_decoder *dec, const uint8_t *data, uint64_t len,
                               const atg_shn_dec_track *tracks, uint32_t n_tracks,
                               atg_shn_dec_result *results, uint64_t *total_samples);
/* the last decode's interleaved int32 PCM / VERBATIM bytes to host memory */
atg_status atg_shn_decode_fetch(atg_shn_decoder *dec, int32_t *pcm, uint64_t pcm_cap);
atg_status atg_shn_decode_fetch_verbatim(atg_shn_decoder *dec, uint8_t *bytes, uint64_t cap);
/* the frame counts of the sets of channels stream `track` of the last decode
   gave, in order (what successive SHNDecoder.read() calls return);
   *n_blocks receives their number, ATG_ERR_CAPACITY when cap is less */
atg_status atg_shn_decode_fetch_blocks(atg_shn_decoder *dec, uint32_t track, uint32_t *lengths,
                                       uint64_t cap, uint64_t *n_blocks);
/* data in device memory (4-byte aligned); *d_pcm stays valid until the
   decoder's next call */
atg_status atg_shn_decode_device(atg_shn_decoder *dec, const void *d_data, uint64_t len,
                                 const atg_shn_dec_track *tracks, uint32_t n_tracks,
                                 atg_shn_dec_result *results, const int32_t **d_pcm,
                                 uint64_t *total_samples);
/* "shnd_index", "shnd_layout", "shnd_parse", "shnd_recon", "shnd_total" */
int atg_shn_decoder_kernel_times(atg_shn_decoder *dec, const char **names, float *ms,
                                 int cap);

#ifdef __cplusplus
}
#endif

/* DVD-Audio: AOB sector demux and its packed-PCM codec, a block of its own */
#include "atgpu_dvda.h"
/* MLP titles of DVD-Audio discs, on the same title table */
#include "atgpu_mlp.h"
/* PCM rows to and from planar float tensors */
#include "atgpu_tensor.h"
/* the dither bits of a batch conversion, made on the device */
#include "atgpu_dither.h"
/* the frame starts inside ranges of FLAC frame data */
#include "atgpu_flac_index.h"
/* test probes into the encoder's kernels */
#include "atgpu_probe.h"
#endif
