"""GPU: the uncompressed containers through the batch entry points:
decoders.decode_pcm_batch (WAV, AIFF and AU images mixed in one call),
encoders.encode_aiff_batch / encode_au_batch against from_pcm, and
encoders.encode_flac_files_batch against encode_flac_batch over the same
files' readers."""
import os
import struct

import numpy as np
import pytest

import audiotools
import oracle_port
import signals
from audiotools import _atgpu
from test_aiff import Reader, make_pcm, read_all

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def decoders(gpu_engine):
    # imported late: the compiled extensions bring libatgpu's HIP runtime up,
    # which in a GPU run must come after torch's (conftest)
    from audiotools import decoders
    return decoders


@pytest.fixture(scope="module")
def encoders(gpu_engine):
    from audiotools import encoders
    return encoders

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "fixtures")
AIFF_OK = ["aiff-1ch", "aiff-2ch", "aiff-6ch", "aiff-8bit", "aiff-metadata", "aiff-misordered"]
# the fixtures whose single-file reader raises: no stream to compare
BAD = {"aiff-nossnd.aiff": "SSND chunk not found",
       "wav-misordered.wav": "data chunk found before fmt"}
WAVS = [os.path.join(HERE, "golden", "wav-2ch.wav")] + [
    os.path.join(FIX, n + ".wav") for n in ("wav-1ch", "wav-6ch", "wav-8bit")]


def open_any(path):
    head = open(path, "rb").read(4)
    cls = {b"FORM": audiotools.AiffAudio, b".snd": audiotools.AuAudio,
           b"RIFF": audiotools.WaveAudio}[head]
    return cls(path)


def reader_pcm(path):
    r = open_any(path).to_pcm()
    try:
        return r, read_all(r)
    finally:
        r.close()


def made_files(tmp_path):
    """AU at 8 / 16 / 24 bits (one with an annotation field) and 24-bit AIFF
    and WAV, written by from_pcm"""
    paths = []
    for k, (cls, ext, ch, bits, frames) in enumerate([
            (audiotools.AuAudio, "au", 2, 8, 1001), (audiotools.AuAudio, "au", 1, 16, 4097),
            (audiotools.AuAudio, "au", 3, 24, 333), (audiotools.AiffAudio, "aiff", 2, 24, 5001),
            (audiotools.WaveAudio, "wav", 2, 24, 4099), (audiotools.AiffAudio, "aiff", 1, 8, 77)]):
        p = str(tmp_path / ("made%d.%s" % (k, ext)))
        cls.from_pcm(p, Reader(make_pcm(frames, ch, bits, seed=k), ch, bits))
        paths.append(p)
    # an AU file whose data starts at an odd offset
    note = b"odd.\0"
    raw = audiotools.pcm.FrameList._wrap(make_pcm(50, 2, 16, seed=9), 2, 16).to_bytes(True, True)
    p = str(tmp_path / "note.au")
    open(p, "wb").write(struct.pack(">4s5I", b".snd", 24 + len(note), len(raw), 3, 8000, 2) +
                        note + raw)
    return paths + [p]


def test_decode_pcm_batch_mixed(decoders, tmp_path):
    """the reference's fixtures that have a readable stream (six of the seven
    AIFF, four of the five WAV) and files made here, in one call: each the PCM
    of its own reader"""
    paths = [os.path.join(FIX, n + ".aiff") for n in AIFF_OK] + WAVS + made_files(tmp_path)
    res = decoders.decode_pcm_batch([open(p, "rb").read() for p in paths])
    assert len(res) == len(paths)
    for p, (status, info, pcm, frames) in zip(paths, res):
        r, want = reader_pcm(p)
        assert status == 0, p
        assert (info.channels, info.bits_per_sample, info.sample_rate, info.channel_mask) == (
            r.channels, r.bits_per_sample, r.sample_rate, r.channel_mask), p
        assert frames == r.total_pcm_frames and pcm.dtype == np.int32
        assert np.array_equal(pcm, want), p
    assert decoders.decode_pcm_batch([]) == []


@pytest.mark.parametrize("name", sorted(BAD))
def test_decode_pcm_batch_header_errors_raise(decoders, name):
    """the two fixtures without a readable stream: the batch raises what
    the file's own reader raises, also with good files around them"""
    good = open(os.path.join(FIX, "aiff-2ch.aiff"), "rb").read()
    bad = open(os.path.join(FIX, name), "rb").read()
    with pytest.raises(ValueError, match=BAD[name]):
        open_any(os.path.join(FIX, name)).to_pcm()
    with pytest.raises(ValueError, match=BAD[name]):
        decoders.decode_pcm_batch([good, bad, good])
    with pytest.raises(ValueError):
        decoders.decode_pcm_batch([good, b"OggS" + bytes(40)])


def test_decode_pcm_batch_truncated(decoders, tmp_path):
    paths = made_files(tmp_path)[:5]
    images, want = [], []
    for p in paths:
        img = open(p, "rb").read()
        a = open_any(p)
        per_frame = a.channels() * a.bits_per_sample() // 8
        _, pcm = reader_pcm(p)
        pad = 1 if p.endswith(".wav") and a.total_frames() % 2 else 0   # from_pcm's pad byte
        pad += 1 if p.endswith(".aiff") and (a.total_frames() * per_frame) % 2 else 0
        for cut in (1, per_frame - 1, 10):
            if cut == 0:
                continue
            images.append(img[:len(img) - pad - cut])
            lost = -(-cut // per_frame)
            want.append((_atgpu.PCMF_TRUNCATED, pcm[:len(pcm) - lost * a.channels()],
                         a.total_frames() - lost))
        images.append(img)
        want.append((0, pcm, a.total_frames()))
    res = decoders.decode_pcm_batch(images)
    for k, ((status, info, pcm, frames), (wstatus, wpcm, wframes)) in enumerate(zip(res, want)):
        assert (status, frames) == (wstatus, wframes), k
        assert np.array_equal(pcm, wpcm), k


@pytest.mark.parametrize("kind", ["aiff", "au"])
def test_encode_batch_matches_from_pcm(encoders, tmp_path, kind):
    cls, batch = {"aiff": (audiotools.AiffAudio, encoders.encode_aiff_batch),
                  "au": (audiotools.AuAudio, encoders.encode_au_batch)}[kind]
    cases = [(ch, bits, frames) for ch in (1, 2, 6) for bits in (8, 16, 24)
             for frames in (0, 1, 4097)]
    pcms = [make_pcm(frames, ch, bits, seed=31) for ch, bits, frames in cases]
    single = [str(tmp_path / ("s%d.%s" % (k, kind))) for k in range(len(cases))]
    batched = [str(tmp_path / ("b%d.%s" % (k, kind))) for k in range(len(cases))]
    for path, pcm, (ch, bits, _) in zip(single, pcms, cases):
        cls.from_pcm(path, Reader(pcm, ch, bits, 48000))
    readers = [Reader(pcm, ch, bits, 48000, step=999) for pcm, (ch, bits, _) in zip(pcms, cases)]
    batch(batched, readers)
    assert all(r.closed for r in readers)
    for a, b, case in zip(single, batched, cases):
        assert open(a, "rb").read() == open(b, "rb").read(), case
    with pytest.raises(audiotools.EncodingError):
        batch([str(tmp_path / "x")], [Reader(np.zeros(2), 2, 32)])
    assert not os.path.exists(str(tmp_path / "x"))


# (container class, extension, bits): two tracks each of 4096 * 2 + 333 and 100 frames
FILE_CASES = [(audiotools.WaveAudio, "wav", 16), (audiotools.WaveAudio, "wav", 24),
              (audiotools.WaveAudio, "wav", 8), (audiotools.AiffAudio, "aiff", 16),
              (audiotools.AiffAudio, "aiff", 24), (audiotools.AuAudio, "au", 8)]


@pytest.mark.parametrize("cls,ext,bits", FILE_CASES,
                         ids=["%s%d" % (e, b) for _, e, b in FILE_CASES])
def test_encode_flac_files_batch(encoders, decoders, tmp_path, cls, ext, bits):
    preset = dict(oracle_port.PRESETS["8"])
    srcs = []
    for k, frames in enumerate((4096 * 2 + 333, 100)):
        pcm = signals.make("tone" if k == 0 else "noise", frames, 2, bits, seed=k + 1)
        p = str(tmp_path / ("in%d.%s" % (k, ext)))
        cls.from_pcm(p, Reader(pcm, 2, bits))
        srcs.append(cls(p))
    want = [str(tmp_path / ("want%d.flac" % k)) for k in range(2)]
    got = [str(tmp_path / ("got%d.flac" % k)) for k in range(2)]
    encoders.encode_flac_batch(want, [s.to_pcm() for s in srcs], **preset)
    written = encoders.encode_flac_files_batch(got, srcs, **preset)
    for w, g, s, (nbytes, frames) in zip(want, got, srcs, written):
        image = open(g, "rb").read()
        assert image == open(w, "rb").read()
        assert (nbytes, frames) == (len(image), s.total_frames())
    # one image decoded back, its STREAMINFO MD5 verified at the end of the stream
    dec = decoders.FlacDecoder(got[0])
    assert (dec.channels, dec.bits_per_sample) == (2, bits)
    back = read_all(dec)
    assert np.array_equal(back, read_all(srcs[0].to_pcm()))


def test_encode_flac_files_batch_mixed_containers(encoders, tmp_path):
    """WAV, AIFF and AU sources of the same stream parameters in one call"""
    preset = dict(oracle_port.PRESETS["8"])
    srcs = []
    for k, cls in enumerate((audiotools.WaveAudio, audiotools.AiffAudio, audiotools.AuAudio)):
        pcm = signals.make("tone", 5000 + 7 * k, 2, 16, seed=k + 5)
        p = str(tmp_path / ("in%d.%s" % (k, cls.SUFFIX)))
        cls.from_pcm(p, Reader(pcm, 2, 16))
        srcs.append(cls(p))
    want = [str(tmp_path / ("want%d.flac" % k)) for k in range(3)]
    got = [str(tmp_path / ("got%d.flac" % k)) for k in range(3)]
    encoders.encode_flac_batch(want, [s.to_pcm() for s in srcs], **preset)
    encoders.encode_flac_files_batch(got, srcs, **preset)
    for w, g in zip(want, got):
        assert open(g, "rb").read() == open(w, "rb").read()
    cut = str(tmp_path / "cut.aiff")
    open(cut, "wb").write(open(srcs[1].filename, "rb").read()[:-10])
    with pytest.raises(IOError, match="premature end of SSND chunk"):
        encoders.encode_flac_files_batch([got[0]], [audiotools.AiffAudio(cut)], **preset)
