"""GPU: tensors.save_batch against cls.from_pcm over FloatFrameList.to_int(),
byte for byte, for the nine types the engine writes; the files load back
through load_batch exactly; save_flac_batch writes what it wrote."""
import os
import types

import numpy as np
import pytest
import torch

import audiotools
from audiotools import pcm
from test_gpu_convert_targets import TYPES, from_pcm_kw, read

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 4097]
SHAPES = [(ch, depth) for ch in (1, 2, 6) for depth in (16, 24)]


@pytest.fixture(autouse=True)
def still_clock(monkeypatch):
    monkeypatch.setattr(audiotools.m4a, "time", types.SimpleNamespace(time=lambda: 1.7e9))


def floats(rng, n, ch):
    return rng.uniform(-1.05, 1.05, size=(ch, n)).astype(np.float32)


def from_pcm_writes(suffix, target, plane, depth, rate, n, got_path):
    """the file, or the exception from_pcm raises for the stream"""
    ch = plane.shape[0]
    ints = pcm.FloatFrameList(plane[:, :n].T.reshape(-1).astype(np.float64).tolist(),
                              ch).to_int(depth)
    cls = audiotools.targets.SUFFIXES[suffix]
    try:
        cls.from_pcm(target, audiotools.FrameListReader(ints, rate, ch, depth, 0),
                     total_pcm_frames=n, **from_pcm_kw(suffix, got_path))
    except (audiotools.EncodingError, audiotools.InvalidFile) as err:
        return err
    return read(target)


@pytest.mark.parametrize("ch,depth", SHAPES, ids=["%dch-%dbit" % s for s in SHAPES])
@pytest.mark.parametrize("suffix", TYPES)
def test_save_batch_writes_what_from_pcm_writes(suffix, ch, depth, tmp_path):
    rng = np.random.RandomState(ch * depth)
    host = np.stack([floats(rng, max(LENGTHS) + 3, ch) for _ in LENGTHS])
    audio = torch.from_numpy(host).cuda()
    targets = [str(tmp_path / ("%d.%s" % (k, suffix))) for k in range(len(LENGTHS))]
    got = audiotools.save_batch(audio, LENGTHS, targets, 44100, depth)
    cls = audiotools.targets.SUFFIXES[suffix]
    written = []
    for k, (g, n, t) in enumerate(zip(got, LENGTHS, targets)):
        ref = str(tmp_path / ("%d.ref.%s" % (k, suffix)))
        want = from_pcm_writes(suffix, ref, host[k], depth, 44100, n,
                               t if os.path.exists(t) else None)
        if isinstance(want, Exception):
            # what the type refuses, it refuses here in from_pcm's words
            assert type(g) is type(want) and str(g) == str(want).replace(ref, t), (k, g)
            assert not os.path.exists(t)
            continue
        assert isinstance(g, cls), (k, g)
        assert read(t) == want, k
        assert g.total_frames() == n
        if n:  # a WavPack file of no blocks does not say what it would hold
            assert (g.channels(), g.bits_per_sample(), g.sample_rate()) == (ch, depth, 44100)
            written.append((k, t))
    if suffix == "shn" and depth == 24:
        assert not written  # Shorten holds 16 bits at most
    else:
        assert [k for k, _ in written] == [1, 2]
        if suffix == "m4a":
            assert isinstance(got[0], audiotools.InvalidFile)  # as from_pcm: see above
        else:
            assert isinstance(got[0], cls)
        # and the files load back exactly
        batch = audiotools.load_batch([t for _, t in written], dtype=torch.int32)
        assert batch.errors == [None] * len(written)
        assert batch.lengths.tolist() == LENGTHS[1:]
        ints = torch.clamp((audio.double() * (1 << (depth - 1))).trunc(),
                           -(1 << (depth - 1)), (1 << (depth - 1)) - 1).to(torch.int32)
        for (k, _), row in zip(written, batch.audio):
            assert torch.equal(row[:, :LENGTHS[k]], ints[k, :, :LENGTHS[k]]), k


def test_types_by_suffix_class_and_list(tmp_path):
    rng = np.random.RandomState(9)
    host = np.stack([floats(rng, 600, 2) for _ in range(3)])
    audio = torch.from_numpy(host).cuda()
    targets = [str(tmp_path / n) for n in ("a.wav", "b.tta", "c.aif")]
    got = audiotools.save_batch(audio, [600, 500, 1], targets, [44100, 48000, 8000], [16, 24, 8])
    assert [type(g) for g in got] == [audiotools.WaveAudio, audiotools.TrueAudio,
                                      audiotools.AiffAudio]
    assert [g.bits_per_sample() for g in got] == [16, 24, 8]
    again = [str(tmp_path / n) for n in ("a2", "b2", "c2")]
    audiotools.save_batch(audio, [600, 500, 1], again, [44100, 48000, 8000], [16, 24, 8],
                          target_types=[audiotools.WaveAudio, "tta", "aiff"])
    assert [read(t) for t in targets] == [read(t) for t in again]
    with pytest.raises(ValueError):
        audiotools.save_batch(audio, [1, 1, 1], ["a.flac", "b.flac", "c.mp3"], 44100)
    with pytest.raises(ValueError):
        audiotools.save_batch(audio, [1, 1, 1], ["a.flac", "b.flac"], 44100)
    # a row that cannot be written is that row's error alone
    targets = [str(tmp_path / "ok.au"), str(tmp_path / "no-such-directory" / "x.au")]
    got = audiotools.save_batch(audio[:2], [5, 5], targets, 44100)
    assert [type(g) for g in got] == [audiotools.AuAudio, audiotools.EncodingError]
    assert [os.path.exists(t) for t in targets] == [True, False]


def test_save_flac_batch_is_unchanged(tmp_path):
    """the FLAC files of save_batch are save_flac_batch's, which are
    FlacAudio.from_pcm's (tests/test_gpu_tensors.py)"""
    rng = np.random.RandomState(4)
    host = np.stack([floats(rng, 5000, 2) for _ in range(3)])
    audio = torch.from_numpy(host).cuda()
    lengths = [5000, 4096, 0]
    a = [str(tmp_path / ("a%d.flac" % k)) for k in range(3)]
    b = [str(tmp_path / ("b%d.flac" % k)) for k in range(3)]
    for compression in (None, "0"):
        got = audiotools.save_flac_batch(audio, lengths, a, 44100, 16, None, compression)
        assert all(isinstance(g, audiotools.FlacAudio) for g in got)
        audiotools.save_batch(audio, lengths, b, 44100, 16, None, "flac", compression)
        assert [read(x) for x in a] == [read(x) for x in b]
        want = from_pcm_writes("flac", str(tmp_path / "ref.flac"), host[0], 16, 44100, 5000, None)
        if compression is None:
            assert read(a[0]) == want
