"""What the GPU tests of split_image_batch, join_tracks_batch and the windows
of convert_files_batch share: sources written by the classes' own from_pcm,
and the oracle, which is always the single-file reader path written out."""

import functools
from fractions import Fraction

import audiotools
from audiotools import Sheet, SheetIndex, SheetTrack, pcmconverter
from test_gpu_convert_files import classes, read, zeros  # noqa: F401

MASKS = {1: 0x4, 2: 0x3, 6: 0x3F}
TYPES = ["flac", "oga", "m4a", "tta", "wv", "shn", "wav", "aiff", "au"]


def write_source(kind, path, x, rate, channels, bits, compression=None):
    """samples x (interleaved) as a file of `kind` (a key of classes())"""
    cls, kw = classes()[kind]
    cls.from_pcm(path, audiotools.FrameListReader(x, rate, channels, bits, MASKS[channels]),
                 compression, total_pcm_frames=len(x) // channels, **kw)
    return path


def from_pcm_kw(suffix, got_path=None):
    """the keywords of the reference call for a type: an Ogg FLAC file is
    given the serial number the batch drew"""
    from audiotools import encoders
    if suffix == "oga":
        serial = int.from_bytes(read(got_path)[14:18], "little") if got_path else 0
        return dict(encoding_function=functools.partial(encoders.encode_oggflac,
                                                        serial_number=serial))
    if suffix == "wv":
        return dict(encoding_function=encoders.encode_wavpack)
    return {}


def window_oracle(kind, path, target, suffix, offset, frames, got_path=None, compression=None,
                  rand=zeros, **convert):
    """cls.from_pcm(target, PCMConverter(BufferedPCMReader(PCMReaderWindow(
    source.to_pcm(), offset, frames)), ...), compression,
    total_pcm_frames=frames) -> the file's bytes, or the exception"""
    pcm = classes()[kind][0](path).to_pcm()
    ch = pcm.channels if convert.get("channels") is None else convert["channels"]
    mask = convert.get("channel_mask")
    if mask is None:
        mask = int(pcm.channel_mask) if ch == pcm.channels else 0
    rate = pcm.sample_rate if convert.get("sample_rate") is None else convert["sample_rate"]
    bits = (pcm.bits_per_sample if convert.get("bits_per_sample") is None
            else convert["bits_per_sample"])
    assert rate == pcm.sample_rate, "the oracle here counts no resampled frames"
    reader = audiotools.PCMConverter(
        audiotools.BufferedPCMReader(audiotools.PCMReaderWindow(pcm, offset, frames)),
        rate, ch, mask, bits)
    if isinstance(reader, pcmconverter.BPSConverter):
        reader._rand = rand
    cls = audiotools.targets.SUFFIXES[suffix]
    try:
        cls.from_pcm(target, reader, compression, total_pcm_frames=frames,
                     **from_pcm_kw(suffix, got_path))
    except (audiotools.EncodingError, audiotools.InvalidFile) as err:
        return err
    return read(target)


def sheet_at(rate, starts, pregaps=None, **kw):
    """a Sheet whose tracks' index 1 are at the PCM frames `starts`;
    pregaps: {track number: PCM frame of its index 0}"""
    tracks = []
    for n, at in enumerate(starts):
        indexes = [SheetIndex(1, Fraction(at, rate))]
        if pregaps and n + 1 in pregaps:
            indexes.insert(0, SheetIndex(0, Fraction(pregaps[n + 1], rate)))
        tracks.append(SheetTrack(n + 1, indexes))
    return Sheet(tracks, **kw)


def cuts_of(starts, total):
    return [(a, b - a) for a, b in zip(starts, list(starts[1:]) + [total])]
