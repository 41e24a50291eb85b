"""audiotools.targets — the writers of a batch: converted tracks that lie in
device memory (DevicePcm) written as files of any format the engine writes.

convert_files_batch and tensors.save_batch end here.  A track's target type
is one of nine AudioFile classes; what its from_pcm refuses is refused
before any GPU work (prepare); the tracks that share what an encoder entry
fixes per call are encoded in one encode_device / encode_oggflac_device /
pcm_pack_device call (write_tracks), the images come down, and every file is
finished on the host as its from_pcm finishes it, with the functions from_pcm
itself uses.  The PCM never comes to the host.

Two things a from_pcm takes from its surroundings stay outside the byte
identity: an Ogg FLAC stream's serial number is random (here one draw per
encode call, file j of the call getting the draw + j, where from_pcm draws
per file), and an .m4a carries its creation time.
"""

import os
import random
from collections import OrderedDict, namedtuple

import numpy as np

from . import EncodingError, InvalidFile
from . import _atgpu
from .aiff import AiffAudio, ERR_AIFF_TOO_LARGE, aiff_header
from .au import AuAudio, ERR_AU_TOO_LARGE, au_header
from .flac import (COMPRESSION_PRESETS, FlacAudio, OggFlacAudio, oggflac_layout, padding_for,
                   target_layout, _unlink)
from .m4a import ALACAudio, check_stream, m4a_file
from .shn import ShortenAudio, wave_parts
from .tta import TrueAudio, tta_header, tta_seektable
from .wav import WaveAudio, wave_header
from .wavpack import WavPackAudio

CLASSES = (FlacAudio, OggFlacAudio, ALACAudio, TrueAudio, WavPackAudio, ShortenAudio, WaveAudio,
           AiffAudio, AuAudio)
SUFFIXES = dict([(c.SUFFIX, c) for c in CLASSES] + [("aif", AiffAudio)])

# one track to write: k is the caller's index of it, d its DevicePcm, mask
# the channel mask its stream reports (pcmreader.channel_mask of the reader
# path), `ready` what prepare() returned for it
Track = namedtuple("Track", "k target cls compression d channels bits_per_sample sample_rate "
                   "mask ready")


def _per_target(value, n, what):
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError("%s has %d entries for %d targets" % (what, len(value), n))
        return list(value)
    return [value] * n


def resolve_types(target_types, targets):
    """target_types (one value or one per target: an AudioFile class of
    CLASSES, one of their SUFFIX strings, or "suffix" for the type the
    target's file name ends in, ".aif" counting as ".aiff") -> one class per
    target; ValueError otherwise"""
    out = []
    for t, target in zip(_per_target(target_types, len(targets), "target_types"), targets):
        if t == "suffix":
            suffix = os.path.splitext(str(target))[1][1:].lower()
            if suffix not in SUFFIXES:
                raise ValueError("no target type for the suffix of %s" % target)
            t = SUFFIXES[suffix]
        elif isinstance(t, str):
            if t not in SUFFIXES:
                raise ValueError("unknown target type %r" % t)
            t = SUFFIXES[t]
        if t not in CLASSES:
            raise ValueError("unknown target type %r" % (t,))
        out.append(t)
    return out


def resolve_compression(compression, classes):
    """one value or one per target -> per target the mode its class's
    from_pcm would use: the class's default for None or an unknown value"""
    out = []
    for c, cls in zip(_per_target(compression, len(classes), "compression"), classes):
        if c is None or c not in getattr(cls, "COMPRESSION_MODES", ()):
            c = getattr(cls, "DEFAULT_COMPRESSION", None)
        out.append(c)
    return out


def prepare(cls, filename, channels, channel_mask, bits_per_sample, sample_rate, frames):
    """what cls.from_pcm decides about a stream of these parameters before it
    encodes: raises the exception from_pcm raises for a stream the type
    cannot hold, else -> what the writer needs of the decision"""
    if cls is FlacAudio:
        return target_layout(filename, channels, channel_mask)
    if cls is OggFlacAudio:
        return oggflac_layout(filename, channels, channel_mask, bits_per_sample)
    if cls is ALACAudio:
        check_stream(filename, bits_per_sample, channel_mask)
    elif cls is ShortenAudio:
        from .m4a import UnsupportedBitsPerSample
        if bits_per_sample not in (8, 16):
            raise UnsupportedBitsPerSample(filename, bits_per_sample)
        return wave_parts(sample_rate, channels, channel_mask, bits_per_sample, frames)
    elif cls is WaveAudio:
        try:
            return wave_header(sample_rate, channels, channel_mask, bits_per_sample, frames)
        except ValueError as err:
            raise EncodingError(str(err))
    return None


# ------------------------------------------------------------- device encodes
def _images(eng, d_out, nbytes, results):
    """the images of one encode call, brought down"""
    out = eng.copy_to_host(np.empty(max(1, nbytes), dtype=np.uint8), d_out)
    return [out[r.out_offset:r.out_offset + r.bytes].tobytes() for r in results]


def _sized(eng, free, guess, call):
    """an encode whose output size is known once it ran: call(d_out, cap) ->
    (results, bytes needed) into `guess` bytes, once more into the size it
    asks for when it reports ATG_ERR_CAPACITY -> (d_out, results, needed)"""
    cap = max(16, int(guess))
    for _ in range(2):
        d_out = eng.device_alloc(cap)
        free.append(d_out)
        try:
            results, need = call(d_out, cap)
            return d_out, results, need
        except _atgpu.ATGError as err:
            if err.status != _atgpu.ATG_ERR_CAPACITY or getattr(err, "needed", 0) <= cap:
                raise
            cap = int(err.needed)
    raise EncodingError("the encoder's output does not fit the size it asked for")


def _tracks_of(members):
    return [(t.d.sample_offset // t.channels, t.d.frames, None) for t in members]


def _raw_bytes(members):
    return sum(t.d.frames * t.channels * ((t.bits_per_sample + 7) // 8) for t in members)


def _encode_flac(eng, free, key, members):
    d_pcm, fmt, ch, bits, rate, pad, compression = key[1:]
    preset = COMPRESSION_PRESETS[compression]
    opts = _atgpu.make_options(padding_size=pad, **preset)
    tracks = _tracks_of(members)
    _, nb = eng.bounds(opts, tracks, ch, bits)
    d_out = eng.device_alloc(max(16, nb))
    free.append(d_out)
    res = eng.encode_device(opts, d_pcm, fmt, tracks, ch, bits, rate, d_out, nb)
    from .convert import _finish
    return [lambda t=t, r=r, image=image: _finish(t.target, image, r.status, t, t.ready,
                                                  t.d.frames, preset["block_size"])
            for t, r, image in zip(members, res, _images(eng, d_out, nb, res))]


def _encode_oggflac(eng, free, key, members):
    d_pcm, fmt, ch, bits, rate, compression, mask = key[1:]
    opts = _atgpu.make_options(**COMPRESSION_PRESETS[compression])
    ogg = _atgpu.oggflac_enc_options(random.getrandbits(32), channel_mask=mask)
    tracks = _tracks_of(members)
    _, nb = eng.oggflac_bounds(opts, ogg, tracks, ch, bits)
    d_out = eng.device_alloc(max(16, nb))
    free.append(d_out)
    res, _, _ = eng.encode_oggflac_device(opts, ogg, d_pcm, fmt, tracks, ch, bits, rate, d_out, nb)
    return [lambda t=t, r=r, image=image: _whole(t, image, r.status)
            for t, r, image in zip(members, res, _images(eng, d_out, nb, res))]


def _encode_alac(eng, free, key, members):
    d_pcm, fmt, ch, bits = key[1:]
    enc = _atgpu.alac_encoder()
    opts = enc.options(ALACAudio.BLOCK_SIZE, ALACAudio.INITIAL_HISTORY,
                       ALACAudio.HISTORY_MULTIPLIER, ALACAudio.MAXIMUM_K)
    tracks = _tracks_of(members)
    nf, nb = enc.bounds(opts, tracks, ch, bits)
    d_out = eng.device_alloc(max(16, nb))
    free.append(d_out)
    fsb = np.zeros(max(1, nf), dtype=np.uint32)
    res = enc.encode_device(opts, d_pcm, fmt, tracks, ch, bits, d_out, nb, fsb)

    def finish(t, r, mdat):
        sizes = [int(x) for x in fsb[r.first_frameset:r.first_frameset + r.n_framesets]]
        return m4a_file(t.channels, t.bits_per_sample, t.sample_rate, ALACAudio.BLOCK_SIZE,
                        int(r.pcm_frames), mdat, sizes)

    return [lambda t=t, r=r, image=image: _whole(t, lambda: finish(t, r, image), r.status)
            for t, r, image in zip(members, res, _images(eng, d_out, nb, res))]


def _encode_tta(eng, free, key, members):
    d_pcm, fmt, ch, bits, rate = key[1:]
    enc = _atgpu.tta_encoder()
    tracks = _tracks_of(members)
    nf = enc.frame_count(tracks, rate)
    fsb = np.zeros(max(1, nf), dtype=np.uint32)
    d_out, res, need = _sized(
        eng, free, _raw_bytes(members) + 64 * nf + 16 * len(members) + 64,
        lambda d_out, cap: enc.encode_device(d_pcm, fmt, tracks, ch, bits, rate, d_out, cap, fsb))

    def finish(t, r, frames):
        sizes = [int(x) for x in fsb[r.first_frame:r.first_frame + r.n_frames]]
        return (tta_header(t.channels, t.bits_per_sample, t.sample_rate, t.d.frames) +
                tta_seektable(sizes) + frames)

    return [lambda t=t, r=r, image=image: _whole(t, lambda: finish(t, r, image), r.status)
            for t, r, image in zip(members, res, _images(eng, d_out, need, res))]


def _encode_wavpack(eng, free, key, members):
    d_pcm, fmt, ch, mask, bits, rate, compression = key[1:]
    enc = _atgpu.wv_encoder()
    o = WavPackAudio.__options__[compression]
    opts = enc.options(o["block_size"], o["correlation_passes"], o["false_stereo"],
                       o["wasted_bits"], o["joint_stereo"])
    tracks = _tracks_of(members)
    nb = enc.block_count(tracks, ch, mask, opts.block_size)
    # every header already holds the frames written, which are the declared
    # total: encode_wavpack's fix-up of another total has nothing to do
    d_out, res, need = _sized(
        eng, free, _raw_bytes(members) + 320 * nb + 128 * len(members) + 64,
        lambda d_out, cap: enc.encode_device(opts, d_pcm, fmt, tracks, ch, mask, bits, rate,
                                             d_out, cap))
    return [lambda t=t, r=r, image=image: _whole(t, image, r.status)
            for t, r, image in zip(members, res, _images(eng, d_out, need, res))]


def _encode_shn(eng, free, key, members):
    d_pcm, fmt, ch, bits = key[1:]
    enc = _atgpu.shn_encoder()
    tracks = _tracks_of(members)
    headers = [t.ready[0] for t in members]
    footers = [t.ready[1] for t in members]
    d_out, res, need = _sized(
        eng, free, 2 * _raw_bytes(members) + sum(len(h) + 64 for h in headers) + 64,
        lambda d_out, cap: enc.encode_device(
            d_pcm, fmt, tracks, ch, bits, d_out, cap, 256, False, bits == 16, headers,
            footers if any(footers) else None))
    return [lambda t=t, image=image: _whole(t, image, 0)
            for t, image in zip(members, _images(eng, d_out, need, res))]


def _encode_packed(eng, free, key, members):
    d_pcm, fmt, width, big_endian, signed = key[1:]
    runs, pos = [], 0
    for t in members:
        n = t.d.frames * t.channels
        runs.append((pos, n, t.d.sample_offset))
        pos += n * width
    cap = (pos + 15) // 16 * 16
    packed = np.zeros(0, dtype=np.uint8)
    if pos:
        d_bytes = eng.device_alloc(max(16, cap))
        free.append(d_bytes)
        pcm_cap = max(r[2] + r[1] for r in runs)
        _atgpu.pcm_pack_device(d_pcm, fmt, pcm_cap, _atgpu.pcm_layout(width, big_endian, signed),
                               runs, d_bytes, cap)
        packed = eng.copy_to_host(np.empty(cap, dtype=np.uint8), d_bytes)

    def finish(t, data):
        if t.cls is WaveAudio:
            return t.ready + data + (b"\0" if t.d.frames % 2 else b"")
        if t.cls is AiffAudio:
            data_size = 8 + len(data)
            if 4 + 8 + 18 + 8 + data_size + data_size % 2 >= (1 << 32):
                raise EncodingError(ERR_AIFF_TOO_LARGE)
            return (aiff_header(t.sample_rate, t.channels, t.bits_per_sample, t.d.frames,
                                data_size) + data + (b"\0" if data_size % 2 else b""))
        if len(data) >= (1 << 32):
            raise EncodingError(ERR_AU_TOO_LARGE)
        return au_header(len(data), t.bits_per_sample, t.sample_rate, t.channels) + data

    return [lambda t=t, data=packed[off:off + n * width].tobytes(): _whole(t, lambda: finish(t, data), 0)
            for t, (off, n, _) in zip(members, runs)]


def _whole(t, data, status):
    """a finished file's bytes written -> the class's instance, or the
    EncodingError with no file left"""
    try:
        if status != 0:
            raise ValueError("the encoder reports status %d" % status)
        if callable(data):
            data = data()
        with open(t.target, "wb") as f:
            f.write(data)
        return t.cls(t.target)
    except (EncodingError, InvalidFile) as err:
        # InvalidFile: from_pcm's own last step, opening what it wrote (an
        # .m4a of no frames is one ALACAudio does not open)
        _unlink(t.target)
        return err
    except (IOError, OSError, ValueError) as err:
        _unlink(t.target)
        return EncodingError(str(err))


def _group_key(t):
    """what the entry that encodes t fixes per call"""
    d, ch, bits, rate = t.d, t.channels, t.bits_per_sample, t.sample_rate
    if t.cls is FlacAudio:
        return (_encode_flac, d.d_pcm, d.fmt, ch, bits, rate, padding_for(d.frames, rate * 10),
                t.compression)
    if t.cls is OggFlacAudio:
        return (_encode_oggflac, d.d_pcm, d.fmt, ch, bits, rate, t.compression, t.ready)
    if t.cls is ALACAudio:
        return (_encode_alac, d.d_pcm, d.fmt, ch, bits)
    if t.cls is TrueAudio:
        return (_encode_tta, d.d_pcm, d.fmt, ch, bits, rate)
    if t.cls is WavPackAudio:
        return (_encode_wavpack, d.d_pcm, d.fmt, ch, int(t.mask), bits, rate, t.compression)
    if t.cls is ShortenAudio:
        return (_encode_shn, d.d_pcm, d.fmt, ch, bits)
    # WAV: little endian, 8 bits unsigned; AIFF and AU: big endian, signed
    wav = t.cls is WaveAudio
    return (_encode_packed, d.d_pcm, d.fmt, bits // 8, not wav, not (wav and bits == 8))


def write_tracks(tracks):
    """[Track] -> {k: the class's instance, or the EncodingError of a track
    that could not be written, with no file left for it}.  One encode call
    per group of tracks that share what their entry fixes per call; a group
    whose call fails leaves its tracks that error and the others go on."""
    eng = _atgpu.engine()
    groups = OrderedDict()
    for t in tracks:
        groups.setdefault(_group_key(t), []).append(t)
    results = {}
    for key, members in groups.items():
        free = []
        try:
            finishers = key[0](eng, free, key, members)
        except (_atgpu.ATGError, EncodingError, ValueError) as err:
            for t in members:
                _unlink(t.target)
                results[t.k] = err if isinstance(err, EncodingError) else EncodingError(
                    getattr(err, "message", None) or str(err))
            continue
        finally:
            for d in free:
                eng.device_free(d)
        for t, finish in zip(members, finishers):
            results[t.k] = finish()
    return results
