"""audiotools.encoders — FLAC / ALAC encoding on the MI355X engine.

`encode_flac` IS the compiled C-API entry point `audiotools._encoders_c.
encode_flac` (csrc/ext/encoders_c.c over libatgpu's C ABI), as the
reference's module function is its C extension (src/encoders/flac.c:44-121,
registered src/encoders.h:65-67):

    encode_flac(filename, pcmreader, block_size, max_lpc_order,
                min_residual_partition_order, max_residual_partition_order,
                mid_side=0, adaptive_mid_side=0, exhaustive_model_search=0,
                disable_verbatim_subframes=0, disable_constant_subframes=0,
                disable_fixed_subframes=0, disable_lpc_subframes=0,
                padding_size=4096) -> [(byte_offset, pcm_frames), ...]

* the output file is opened first; failure raises OSError/IOError carrying
  errno and filename (flac.c:114-116);
* PCM is pulled with pcmreader.read(block_size) until an empty FrameList,
  and every read becomes one FLAC frame, exactly as the reference frame loop
  does (flac.c:244-274) — with a BufferedPCMReader that is block_size
  frames plus a shorter final frame;
* read() must return pcm.FrameList objects (TypeError otherwise,
  pcmconv.c:244-248); exceptions raised by read() propagate;
* on success the reader is closed (flac.c:282) and the list of
  (offset of the frame from the first frame, pcm frames) is returned.

It streams: up to 256 FLAC frames per GPU call (atg_flac_encode_frames) with
the GIL released, the MD5 of each segment's PCM bytes on a host thread
beside the GPU call, STREAMINFO rewritten at the end (flac.c:276-279), on a
streaming engine (two HIP streams per process, for one process per track
under track2track).

`encode_flac_batch` is the batch form the engine is built for: many tracks
in one GPU pass (what track2track -j N achieves with N processes), MD5
chains on the GPU, the tracks sharded over the node's GPUs.

`encode_oggflac` / `encode_oggflac_batch` write the same frames into an Ogg
container (.oga; GPU kernels ogg_mux.hip), where the reference calls the
external `flac --ogg` (audiotools/flac.py:3249-3367).

`encode_alac` / `encode_alac_batch` do the same for ALAC (reference
src/encoders/alac.c:30-189; GPU kernels alac_encode.hip).

`encode_tta` / `encode_tta_batch` do the same for True Audio (reference
src/encoders/tta.c:31-114; GPU kernels tta_encode.hip), `encode_shn` /
`encode_shn_batch` for Shorten (src/encoders/shn.c; shn_encode.hip).

`encode_wavpack` / `encode_wavpack_batch` do the same for WavPack (reference
src/encoders/wavpack.c; GPU kernels wavpack_encode.hip): complete .wv files.

`encode_aiff_batch` / `encode_au_batch` write AIFF / Sun AU files whose
big-endian samples are packed on the GPU (pcm_bytes.hip), the files of
AiffAudio.from_pcm / AuAudio.from_pcm; `encode_flac_files_batch` encodes
WAV / AIFF / AU files to FLAC with their data chunks uploaded as they lie on
disk and unpacked on the device.
"""

import numpy as np

from . import pcm as _pcm
from . import _atgpu
from ._encoders_c import encode_flac  # noqa: F401  (the drop-in entry point)


def pcm_le_bytes(samples, bits_per_sample):
    """little-endian signed PCM bytes of interleaved samples: what the
    reference's MD5 callback hashes (FrameList.to_bytes(False, True),
    flac.c:187-188 -> pcmconv.c:266-291)"""
    a = np.asarray(samples)
    if bits_per_sample <= 8:
        return a.astype(np.int8).tobytes()
    if bits_per_sample <= 16:
        return a.astype("<i2").tobytes()
    w = (bits_per_sample + 7) // 8
    return np.ascontiguousarray(a.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :w]).tobytes()


def _collect(pcmreader, block_size):
    """drain a PCMReader the way the reference frame loop does"""
    chunks, sizes = [], []
    while True:
        fl = pcmreader.read(block_size)
        if not isinstance(fl, _pcm.FrameList):
            raise TypeError("results from pcmreader.read() must be FrameLists")
        if fl.frames == 0:
            break
        if fl.channels != pcmreader.channels:
            raise ValueError("FrameList channel count does not match pcmreader")
        chunks.append(fl.samples)
        sizes.append(fl.frames)
    samples = (np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.int32))
    return samples, sizes


def _frame_sizes_or_none(sizes, block_size):
    """None when the chunks are plain block_size blocking (+ short tail)"""
    if all(s == block_size for s in sizes[:-1]) and (not sizes or sizes[-1] <= block_size):
        return None
    return np.asarray(sizes, dtype=np.uint32)


_SHARED_NAMES = {"channels": "channels", "channel_mask": "channel mask",
                 "bits_per_sample": "bits-per-sample", "sample_rate": "sample rate"}


def _shared_format(pcmreaders, attrs):
    """the values of `attrs` that every reader of a batch must share, as ints
    (a channel mask may be an object); ValueError where one differs"""
    fmt = tuple(int(getattr(pcmreaders[0], a)) for a in attrs)
    for r in pcmreaders:
        if tuple(int(getattr(r, a)) for a in attrs) != fmt:
            names = [_SHARED_NAMES[a] for a in attrs]
            raise ValueError("all pcmreaders of a batch must share %s and %s" %
                             (", ".join(names[:-1]), names[-1]))
    return fmt


def _drain(pcmreaders, block_size, channels, bits_per_sample, irregular=None):
    """every reader drained as _collect drains it, in order -> (one PCM array,
    int16 up to 16 bits per sample and int32 above, [(first frame, frames,
    read sizes or None for plain blocking)]).  With `irregular`, that
    exception is raised after a reader whose reads were not plain blocking."""
    parts, tracks, start = [], [], 0
    for r in pcmreaders:
        samples, sizes = _collect(r, block_size)
        sizes = _frame_sizes_or_none(sizes, block_size)
        if sizes is not None and irregular is not None:
            raise irregular
        frames = len(samples) // channels
        tracks.append((start, frames, sizes))
        parts.append(samples)
        start += frames
    pcm = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
    return pcm.astype(np.int16 if bits_per_sample <= 16 else np.int32, copy=False), tracks


def _write_images(files, out, results):
    """image k of `out` (results[k].out_offset, .bytes) to files[k]: an open
    file object, or a name, opened when its turn comes"""
    for f, res in zip(files, results):
        image = memoryview(out[res.out_offset:res.out_offset + res.bytes])
        if isinstance(f, str):
            with open(f, "wb") as g:
                g.write(image)
        else:
            f.write(image)


def _flac_batch(filenames, pcmreaders, block_size, flac_args, encode):
    """what encode_flac_batch and encode_oggflac_batch share: the readers
    drained to one PCM array, the tracks sharded over the node's GPUs,
    encode(engine, options, pcm, tracks, channels, bps, rate, first track) ->
    (out, results, per-frame offsets, per-frame pcm frames) per shard, the
    images written to the files; returns one offsets list per file"""
    filenames = list(filenames)
    pcmreaders = list(pcmreaders)
    if len(filenames) != len(pcmreaders):
        raise ValueError("filenames and pcmreaders differ in length")
    if not pcmreaders:
        return []
    channels, bps, rate = _shared_format(pcmreaders,
                                         ("channels", "bits_per_sample", "sample_rate"))
    files = [open(fn, "wb") for fn in filenames]
    try:
        opts = _atgpu.make_options(block_size, *flac_args)
        pcm, tracks = _drain(pcmreaders, block_size, channels, bps)
        # the tracks sharded over the node's GPUs (contiguous groups balanced
        # by frames, one engine per device, _atgpu.batch_devices)
        devs = _atgpu.batch_devices()
        ranges = (_atgpu.shard_ranges([t[1] for t in tracks], len(devs))
                  if len(devs) > 1 else [(0, len(tracks))])

        def shard(i):
            t0, t1 = ranges[i]
            s0 = tracks[t0][0]
            s1 = tracks[t1 - 1][0] + tracks[t1 - 1][1]
            eng = (_atgpu.engine() if len(ranges) == 1
                   else _atgpu.shard_object("engine", i, devs[i]))
            return encode(eng, opts, pcm[s0 * channels:s1 * channels],
                          [(a - s0, n, fs) for a, n, fs in tracks[t0:t1]],
                          channels, bps, rate, t0)

        lists = []
        for (t0, t1), (out, results, offsets, pcm_frames) in zip(
                ranges, _atgpu.run_shards(shard, len(ranges))):
            _write_images(files[t0:t1], out, results)
            for res in results:
                lo, n = res.first_frame, res.n_frames
                lists.append([(int(offsets[lo + i]), int(pcm_frames[lo + i]))
                              for i in range(n)])
        for r in pcmreaders:
            r.close()
        return lists
    finally:
        for f in files:
            f.close()


def encode_flac_batch(filenames, pcmreaders, block_size, max_lpc_order,
                      min_residual_partition_order, max_residual_partition_order,
                      mid_side=0, adaptive_mid_side=0, exhaustive_model_search=0,
                      disable_verbatim_subframes=0, disable_constant_subframes=0,
                      disable_fixed_subframes=0, disable_lpc_subframes=0,
                      padding_size=4096):
    """encode several PCMReaders (same channels / bits / rate) to several
    .flac files in one GPU batch; returns one offsets list per file"""
    def encode(eng, opts, pcm, tracks, channels, bps, rate, t0):
        return eng.encode(opts, pcm, tracks, channels, bps, rate)

    return _flac_batch(filenames, pcmreaders, block_size,
                       (max_lpc_order, min_residual_partition_order,
                        max_residual_partition_order, mid_side, adaptive_mid_side,
                        exhaustive_model_search, disable_verbatim_subframes,
                        disable_constant_subframes, disable_fixed_subframes,
                        disable_lpc_subframes, padding_size), encode)


def encode_oggflac_batch(filenames, pcmreaders, block_size, max_lpc_order,
                         min_residual_partition_order, max_residual_partition_order,
                         mid_side=0, adaptive_mid_side=0, exhaustive_model_search=0,
                         disable_verbatim_subframes=0, disable_constant_subframes=0,
                         disable_fixed_subframes=0, disable_lpc_subframes=0,
                         padding_size=4096, serial_number=None, page_segments=255,
                         page_per_packet=True, channel_mask=0):
    """encode several PCMReaders (same channels / bits / rate) to several
    Ogg FLAC (.oga) files in one GPU batch (ogg_mux.hip; the reference pipes
    each to `flac --ogg`, audiotools/flac.py:3249-3367).  File k of the call
    gets the serial number serial_number + k (None: 32 random bits per call);
    a page holds page_segments lacing values at most and, with
    page_per_packet, no more than one FLAC frame; a nonzero channel_mask is
    written as WAVEFORMATEXTENSIBLE_CHANNEL_MASK.  Returns one list of
    (offset of the page the frame's packet begins on, pcm frames) per file."""
    if serial_number is None:
        import random
        serial_number = random.getrandbits(32)

    def encode(eng, opts, pcm, tracks, channels, bps, rate, t0):
        ogg = _atgpu.oggflac_enc_options(serial_number + t0, page_segments, page_per_packet,
                                         channel_mask)
        return eng.encode_oggflac(opts, ogg, pcm, tracks, channels, bps, rate)

    return _flac_batch(filenames, pcmreaders, block_size,
                       (max_lpc_order, min_residual_partition_order,
                        max_residual_partition_order, mid_side, adaptive_mid_side,
                        exhaustive_model_search, disable_verbatim_subframes,
                        disable_constant_subframes, disable_fixed_subframes,
                        disable_lpc_subframes, padding_size), encode)


def encode_oggflac(filename, pcmreader, block_size, max_lpc_order,
                   min_residual_partition_order, max_residual_partition_order, **options):
    """one PCMReader to one Ogg FLAC file: encode_oggflac_batch of one"""
    return encode_oggflac_batch([filename], [pcmreader], block_size, max_lpc_order,
                                min_residual_partition_order, max_residual_partition_order,
                                **options)[0]


def encode_alac_batch(files, pcmreaders, block_size, initial_history, history_multiplier,
                      maximum_k, minimum_interlacing_leftweight=0,
                      maximum_interlacing_leftweight=4):
    """several PCMReaders (same channels / bits) -> one mdat atom written to
    each file object in one GPU batch; one (frame_byte_sizes,
    total_pcm_frames) tuple per file"""
    files = list(files)
    pcmreaders = list(pcmreaders)
    if len(files) != len(pcmreaders):
        raise ValueError("files and pcmreaders differ in length")
    if not pcmreaders:
        return []
    # the leftweights tried per stereo frame (alac.c:57-72, 459-481); the
    # reference writes them in 8 bits and, with min > max, emits a stale
    # frame: both refused here
    if not (0 <= minimum_interlacing_leftweight <= maximum_interlacing_leftweight <= 255):
        raise ValueError("interlacing leftweights must satisfy 0 <= minimum <= maximum <= 255")
    if pcmreaders[0].bits_per_sample not in (16, 24):
        raise ValueError("bits per sample must be 16 or 24")
    channels, bps = _shared_format(pcmreaders, ("channels", "bits_per_sample"))
    pcm, tracks = _drain(pcmreaders, block_size, channels, bps)
    enc = _atgpu.alac_encoder()
    opts = enc.options(block_size, initial_history, history_multiplier, maximum_k,
                       minimum_interlacing_leftweight, maximum_interlacing_leftweight)
    out, results, fsb = enc.encode(opts, pcm, tracks, channels, bps)
    _write_images(files, out, results)
    logs = []
    for res in results:
        lo = res.first_frameset
        logs.append(([int(x) for x in fsb[lo:lo + res.n_framesets]], int(res.pcm_frames)))
    for r in pcmreaders:
        r.close()
    return logs


def encode_alac(file, pcmreader, block_size, initial_history, history_multiplier, maximum_k,
                minimum_interlacing_leftweight=0, maximum_interlacing_leftweight=4):
    """encode_alac(file, pcmreader, block_size, initial_history,
    history_multiplier, maximum_k) -> ([frameset byte sizes], total PCM frames)

    writes the mdat atom (size, "mdat", framesets) to the file object at
    its position, as the reference does (src/encoders/alac.c:30-189)"""
    if not hasattr(file, "write"):
        raise TypeError("file must by a concrete file object")
    return encode_alac_batch([file], [pcmreader], block_size, initial_history,
                             history_multiplier, maximum_k, minimum_interlacing_leftweight,
                             maximum_interlacing_leftweight)[0]


def tta_block_size(sample_rate):
    """PCM frames per TTA frame (src/encoders/tta.c:62)"""
    return (int(sample_rate) * 256) // 245


def encode_tta_batch(files, pcmreaders):
    """several PCMReaders (same channels / bits / rate) -> the TTA frames of
    each written to its file object in one GPU batch (no header, no
    seektable); one list of frame byte sizes per file"""
    files = list(files)
    pcmreaders = list(pcmreaders)
    if len(files) != len(pcmreaders):
        raise ValueError("files and pcmreaders differ in length")
    if not pcmreaders:
        return []
    if pcmreaders[0].bits_per_sample not in (8, 16, 24):
        raise ValueError("bits per sample must be 8, 16 or 24")
    channels, bps, rate = _shared_format(pcmreaders,
                                         ("channels", "bits_per_sample", "sample_rate"))
    block_size = tta_block_size(rate)
    if block_size < 1:
        raise ValueError("sample rate too low for a TTA frame")
    # every read is one TTA frame, a short read a short frame (tta.c:70-82)
    pcm, tracks = _drain(pcmreaders, block_size, channels, bps)
    out, results, fsb = _atgpu.tta_encoder().encode(pcm, tracks, channels, bps, rate)
    _write_images(files, out, results)
    logs = [[int(x) for x in fsb[res.first_frame:res.first_frame + res.n_frames]]
            for res in results]
    for r in pcmreaders:
        r.close()
    return logs


def encode_tta(file, pcmreader):
    """encode_tta(file, pcmreader) -> [frame byte sizes]

    writes the TTA frames to the file object at its position, as the
    reference does (src/encoders/tta.c:31-114); header and seektable are
    the caller's (audiotools.tta.TrueAudio.from_pcm)"""
    if not hasattr(file, "write"):
        raise TypeError("file must by a concrete file object")
    return encode_tta_batch([file], [pcmreader])[0]


def encode_shn_batch(filenames, pcmreaders, is_big_endian, signed_samples, header_data,
                     footer_data=None, block_size=256):
    """several PCMReaders (same channels / bits) -> one .shn file each in one
    GPU batch; header_data / footer_data are one bytes object per file (or
    None for no footers)"""
    filenames = list(filenames)
    pcmreaders = list(pcmreaders)
    if len(filenames) != len(pcmreaders):
        raise ValueError("filenames and pcmreaders differ in length")
    if not pcmreaders:
        return
    if pcmreaders[0].bits_per_sample not in (8, 16):
        raise ValueError("unsupported bits per sample")
    channels, bps = _shared_format(pcmreaders, ("channels", "bits_per_sample"))
    block_size = int(block_size)
    # a read that returns another length than the last becomes a BLOCKSIZE
    # command (shn.c:213-218)
    pcm, tracks = _drain(pcmreaders, block_size, channels, bps)
    out, results = _atgpu.shn_encoder().encode(
        pcm, tracks, channels, bps, block_size, is_big_endian, signed_samples,
        headers=list(header_data), footers=None if footer_data is None else list(footer_data))
    _write_images(filenames, out, results)
    for r in pcmreaders:
        r.close()


def encode_shn(filename, pcmreader, is_big_endian, signed_samples, header_data,
               footer_data=None, block_size=256):
    """encode_shn(filename, pcmreader, is_big_endian, signed_samples,
    header_data, footer_data=None, block_size=256)

    writes the whole Shorten file, as the reference does
    (src/encoders/shn.c:26-145): header_data goes into a leading VERBATIM
    command, footer_data, if any, into one after the audio"""
    encode_shn_batch([filename], [pcmreader], is_big_endian, signed_samples, [header_data],
                     None if not footer_data else [footer_data], block_size)


def encode_wavpack_batch(filenames, pcmreaders, block_size, total_pcm_frames=0,
                         false_stereo=False, wasted_bits=False, joint_stereo=False,
                         correlation_passes=0, wave_header=None, wave_footer=None):
    """several PCMReaders (same channels / mask / bits / rate) -> one complete
    .wv file each, in one GPU batch.  total_pcm_frames: 0, one value for every
    file, or a list of one per file (see encode_wavpack)"""
    filenames = list(filenames)
    pcmreaders = list(pcmreaders)
    if len(filenames) != len(pcmreaders):
        raise ValueError("filenames and pcmreaders differ in length")
    if wave_header is not None or wave_footer is not None:
        raise ValueError("external RIFF WAVE header / footer are not supported")
    if not pcmreaders:
        return
    totals = (list(total_pcm_frames) if isinstance(total_pcm_frames, (list, tuple))
              else [total_pcm_frames] * len(pcmreaders))
    if len(totals) != len(pcmreaders):
        raise ValueError("total_pcm_frames and pcmreaders differ in length")
    channels, mask, bps, rate = _shared_format(
        pcmreaders, ("channels", "channel_mask", "bits_per_sample", "sample_rate"))
    block_size = int(block_size)
    if block_size < 1:
        raise ValueError("block size must be at least 1")
    files = [open(fn, "wb") for fn in filenames]
    try:
        pcm, tracks = _drain(pcmreaders, block_size, channels, bps, irregular=ValueError(
            "WavPack is encoded from whole blocks: every read but the last must return "
            "block_size frames"))
        enc = _atgpu.wv_encoder()
        opts = enc.options(block_size, correlation_passes, false_stereo, wasted_bits,
                           joint_stereo)
        try:
            out, results, bsb = enc.encode(opts, pcm, tracks, channels, mask, bps, rate)
        except _atgpu.ATGError as err:
            if err.status in (_atgpu.ATG_ERR_INVALID, _atgpu.ATG_ERR_UNSUPPORTED):
                raise ValueError(err.message)
            raise
        for res, total in zip(results, totals):
            if total and int(total) != res.pcm_frames:
                # the declared total stays in every header: the reference
                # fixes the field up only when it was given as 0
                pos = res.out_offset
                for size in list(bsb[res.first_block:res.first_block + res.n_blocks]) + [50]:
                    out[pos + 12:pos + 16] = np.frombuffer(
                        (int(total) & 0xFFFFFFFF).to_bytes(4, "little"), dtype=np.uint8)
                    pos += int(size)
        _write_images(files, out, results)
        for r in pcmreaders:
            r.close()
    finally:
        for f in files:
            f.close()


def encode_wavpack(filename, pcmreader, block_size, total_pcm_frames=0, false_stereo=False,
                   wasted_bits=False, joint_stereo=False, correlation_passes=0,
                   wave_header=None, wave_footer=None):
    """encode_wavpack(filename, pcmreader, block_size, ...) writes the file
    the reference's does (src/encoders/wavpack.c:31-249).

    With total_pcm_frames 0, or equal to the frames read, every header holds
    the frames read.  A different total is written as declared, which is what
    the reference's source does; its stand-alone encoder cannot reach that
    path, so no reference vector covers it.  wave_header / wave_footer
    (from_wave) are not supported: anything but None raises ValueError."""
    encode_wavpack_batch([filename], [pcmreader], block_size, total_pcm_frames, false_stereo,
                         wasted_bits, joint_stereo, correlation_passes, wave_header,
                         wave_footer)


# ------------------------------------------- uncompressed: AIFF, Sun AU, files
def _pack_batch(filenames, pcmreaders, check, finish):
    """what encode_aiff_batch and encode_au_batch share: the readers drained
    as _collect drains them, their samples uploaded as integers, packed big
    endian on the device (pcm_bytes.hip) and the packed image brought down at
    1 to 3 bytes per sample; finish(file object, reader, frames, data bytes)
    writes each file.  Readers of one batch may differ in every parameter."""
    from . import EncodingError, FRAMELIST_SIZE
    filenames = list(filenames)
    pcmreaders = list(pcmreaders)
    if len(filenames) != len(pcmreaders):
        raise ValueError("filenames and pcmreaders differ in length")
    for name, r in zip(filenames, pcmreaders):
        check(name, r)
    drained = []
    for r in pcmreaders:
        try:
            samples, _ = _collect(r, FRAMELIST_SIZE)
        except (IOError, ValueError) as err:
            raise EncodingError(str(err))
        drained.append(samples)
    eng = _atgpu.engine()
    packed = [None] * len(pcmreaders)
    # one launch per sample width; up to 16 bits the samples go up as int16
    for width in (1, 2, 3):
        idx = [k for k, r in enumerate(pcmreaders) if r.bits_per_sample // 8 == width]
        if not idx:
            continue
        dtype, fmt = (np.int32, _atgpu.PCM_S32) if width == 3 else (np.int16, _atgpu.PCM_S16)
        group = 16 // np.dtype(dtype).itemsize
        runs, pos, slot = [], 0, 0
        for k in idx:
            n = len(drained[k])
            runs.append((pos, n, slot))
            pos += n * width
            slot += (n + group - 1) // group * group
        if not pos:
            for k in idx:
                packed[k] = np.zeros(0, dtype=np.uint8)
            continue
        pcm = np.zeros(slot, dtype=dtype)
        for k, (_, n, s) in zip(idx, runs):
            pcm[s:s + n] = drained[k]
        out = np.empty(pos, dtype=np.uint8)
        d_pcm, d_bytes = eng.device_alloc(pcm.nbytes), eng.device_alloc(pos)
        try:
            eng.copy_to_device(d_pcm, pcm)
            _atgpu.pcm_pack_device(d_pcm, fmt, slot, _atgpu.pcm_layout(width, True, True), runs,
                                   d_bytes, pos)
            eng.copy_to_host(out, d_bytes)
        finally:
            eng.device_free(d_pcm)
            eng.device_free(d_bytes)
        for k, (off, n, _) in zip(idx, runs):
            packed[k] = out[off:off + n * width]
    for name, r, data in zip(filenames, pcmreaders, packed):
        try:
            with open(name, "wb") as f:
                finish(f, r, len(data) // (r.channels * (r.bits_per_sample // 8)), data)
        except IOError as err:
            raise EncodingError(str(err))
    for r in pcmreaders:
        r.close()


def _check_bits(name, r):
    if r.bits_per_sample not in (8, 16, 24):
        from .m4a import UnsupportedBitsPerSample
        raise UnsupportedBitsPerSample(name, r.bits_per_sample)


def encode_aiff_batch(filenames, pcmreaders):
    """several PCMReaders -> one AIFF file each, the samples packed on the GPU
    in one batch; the files are those AiffAudio.from_pcm writes"""
    from . import EncodingError
    from .aiff import aiff_header, ERR_AIFF_TOO_LARGE

    def finish(f, r, frames, data):
        data_size = 8 + len(data)
        if 4 + 8 + 18 + 8 + data_size + data_size % 2 >= (1 << 32):
            raise EncodingError(ERR_AIFF_TOO_LARGE)
        f.write(aiff_header(r.sample_rate, r.channels, r.bits_per_sample, frames, data_size))
        f.write(memoryview(data))
        if data_size % 2:
            f.write(b"\0")

    _pack_batch(filenames, pcmreaders, _check_bits, finish)


def encode_au_batch(filenames, pcmreaders):
    """several PCMReaders -> one Sun AU file each, the samples packed on the
    GPU in one batch; the files are those AuAudio.from_pcm writes"""
    from . import EncodingError
    from .au import au_header, ERR_AU_TOO_LARGE

    def finish(f, r, frames, data):
        if len(data) >= (1 << 32):
            raise EncodingError(ERR_AU_TOO_LARGE)
        f.write(au_header(len(data), r.bits_per_sample, r.sample_rate, r.channels))
        f.write(memoryview(data))

    _pack_batch(filenames, pcmreaders, _check_bits, finish)


def encode_flac_files_batch(filenames, sources, block_size, max_lpc_order,
                            min_residual_partition_order, max_residual_partition_order,
                            mid_side=0, adaptive_mid_side=0, exhaustive_model_search=0,
                            disable_verbatim_subframes=0, disable_constant_subframes=0,
                            disable_fixed_subframes=0, disable_lpc_subframes=0,
                            padding_size=4096):
    """WaveAudio / AiffAudio / AuAudio objects (same channels / bits / rate) ->
    one .flac file each, the PCM never unpacked on the host: the files' data
    chunks are uploaded as they lie on disk (1 to 3 bytes per sample),
    unpacked on the device (pcm_bytes.hip) into the engine's int16 / int32
    container and encoded from there, the tracks sharded over the node's GPUs
    as encode_flac_batch shards them.  The files are those
    encode_flac_batch(filenames, [s.to_pcm() for s in sources], ...) writes.
    Returns one (bytes written, pcm frames) per file; IOError with the
    reader's message for a file whose data ends early."""
    from . import pcmfiles
    filenames = list(filenames)
    sources = list(sources)
    if len(filenames) != len(sources):
        raise ValueError("filenames and sources differ in length")
    if not sources:
        return []
    images, infos = [], []
    for s in sources:
        with open(s.filename, "rb") as f:
            images.append(f.read())
        infos.append(pcmfiles.image_info(images[-1]))
        if infos[-1].frames < infos[-1].total_pcm_frames:
            raise IOError(pcmfiles.TRUNCATED[infos[-1].kind])
    i0 = infos[0]
    channels, bps, rate = i0.channels, i0.bits_per_sample, i0.sample_rate
    for i in infos:
        if (i.channels, i.bits_per_sample, i.sample_rate) != (channels, bps, rate):
            raise ValueError("all sources of a batch must share channels, "
                             "bits-per-sample and sample rate")
    files = [open(fn, "wb") for fn in filenames]
    try:
        opts = _atgpu.make_options(block_size, max_lpc_order, min_residual_partition_order,
                                   max_residual_partition_order, mid_side, adaptive_mid_side,
                                   exhaustive_model_search, disable_verbatim_subframes,
                                   disable_constant_subframes, disable_fixed_subframes,
                                   disable_lpc_subframes, padding_size)
        fmt, dtype = ((_atgpu.PCM_S16, np.int16) if bps <= 16 else (_atgpu.PCM_S32, np.int32))
        devs = _atgpu.batch_devices()
        ranges = (_atgpu.shard_ranges([i.frames for i in infos], len(devs))
                  if len(devs) > 1 else [(0, len(infos))])

        def shard(k):
            t0, t1 = ranges[k]
            eng = (_atgpu.engine() if len(ranges) == 1
                   else _atgpu.shard_object("engine", k, devs[k]))
            part = infos[t0:t1]
            # every track's first frame on a 16-byte boundary of the container
            runs, cap, n_samples = pcmfiles.plan(part, 8 * channels)
            tracks = [(slot // channels, i.frames, None) for i, (_, _, slot) in zip(part, runs)]
            _, nb = eng.bounds(opts, tracks, channels, bps)
            out = np.empty(max(1, nb), dtype=np.uint8)
            bufs = []
            try:
                for nbytes in (max(cap, 16), max(16, n_samples * np.dtype(dtype).itemsize),
                               max(16, nb)):
                    bufs.append(eng.device_alloc(nbytes))
                d_bytes, d_pcm, d_out = bufs
                eng.copy_to_device(d_bytes, pcmfiles.gather(images[t0:t1], part, cap))
                pcmfiles.unpack_groups(part, runs, d_bytes, cap, d_pcm, fmt, n_samples)
                results = eng.encode_device(opts, d_pcm, fmt, tracks, channels, bps, rate,
                                            d_out, nb)
                eng.copy_to_host(out, d_out)
            finally:
                for d in bufs:
                    eng.device_free(d)
            return out, results

        written = []
        for (t0, t1), (out, results) in zip(ranges, _atgpu.run_shards(shard, len(ranges))):
            _write_images(files[t0:t1], out, results)
            written += [(int(res.bytes), i.frames) for res, i in zip(results, infos[t0:t1])]
        return written
    finally:
        for f in files:
            f.close()
