"""GPU: audiotools.tensors -- load_batch against the single-file readers and
FrameList.to_float(), save_flac_batch byte for byte against
FlacAudio.from_pcm over FloatFrameList.to_int(), and the two row functions
between them."""
import os

import numpy as np
import pytest
import torch

import pcm_tensor_port as port
import signals
import audiotools
from audiotools import pcm
from pcm_tensor_port import bits

pytestmark = pytest.mark.gpu

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fixtures")
MASKS = {1: 0x4, 2: 0x3, 6: 0x3F}
PORT_DTYPE = {torch.float16: port.F16, torch.float32: port.F32, torch.float64: port.F64,
              torch.int32: port.I32}


def classes():
    from audiotools import encoders
    return {
        "flac": (audiotools.FlacAudio, {}),
        "oga": (audiotools.OggFlacAudio, dict(encoding_function=encoders.encode_oggflac)),
        "m4a": (audiotools.ALACAudio, {}),
        "tta": (audiotools.TrueAudio, {}),
        "wv": (audiotools.WavPackAudio, dict(encoding_function=encoders.encode_wavpack)),
        "shn": (audiotools.ShortenAudio, {}),
        "wav": (audiotools.WaveAudio, {}),
        "aiff": (audiotools.AiffAudio, {}),
        "au": (audiotools.AuAudio, {}),
    }


# one stereo source per format: kind -> (frames, channels, bits, rate)
SOURCES = {
    "flac": (4096 + 100, 2, 24, 96000),
    "oga": (3000, 2, 16, 48000),
    "m4a": (4096, 2, 16, 44100),
    "tta": (3000, 2, 16, 44100),
    "wv": (4097, 2, 16, 48000),
    "shn": (3, 2, 16, 44100),
    "wav": (2500, 2, 24, 96000),
    "aiff": (100, 2, 16, 44100),
    "au": (4500, 2, 24, 44100),
}
KINDS = list(SOURCES)


def drain(reader):
    parts = []
    while True:
        fl = reader.read(4096)
        if fl.frames == 0:
            break
        parts.append(np.asarray(fl.samples, dtype=np.int32))
    reader.close()
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    """kind -> (path, the PCM its own single-file reader gives)"""
    d = tmp_path_factory.mktemp("tensor_src")
    out = {}
    for k, (kind, (n, ch, depth, rate)) in enumerate(SOURCES.items()):
        x = signals.make("tone", n, ch, depth, seed=40 + k)
        cls, kw = classes()[kind]
        path = str(d / ("source." + kind))
        cls.from_pcm(path, audiotools.FrameListReader(x, rate, ch, depth, MASKS[ch]),
                     total_pcm_frames=n, **kw)
        out[kind] = (path, drain(cls(path).to_pcm()))
    return out


def check_rows(batch, pcms, params, dtype, t=None):
    """audio[k] is to_float() of pcms[k], channel by channel, zeros behind"""
    t = max(len(x) // p[0] for x, p in zip(pcms, params)) if t is None else t
    ch = params[0][0]
    assert tuple(batch.audio.shape) == (len(pcms), ch, t) and batch.audio.dtype == dtype
    assert batch.audio.is_cuda and batch.lengths.dtype == torch.int64
    assert not batch.lengths.is_cuda
    got = batch.audio.cpu().numpy()
    for k, (x, (_, depth)) in enumerate(zip(pcms, params)):
        n = len(x) // ch
        assert int(batch.lengths[k]) == n
        want = np.zeros((ch, t), dtype=got.dtype)
        want[:, :n] = port.to_values(x, ch, depth, PORT_DTYPE[dtype])
        assert np.array_equal(bits(got[k]), bits(want)), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_load_batch_nine_formats(sources, dtype):
    batch = audiotools.load_batch([sources[k][0] for k in KINDS], dtype=dtype)
    assert batch.errors == [None] * len(KINDS)
    assert batch.sample_rates == [SOURCES[k][3] for k in KINDS]
    assert batch.bits_per_sample == [SOURCES[k][2] for k in KINDS]
    assert batch.channel_masks == [0x3] * len(KINDS)
    for k in KINDS:
        assert len(sources[k][1]) == SOURCES[k][0] * 2, k
    check_rows(batch, [sources[k][1] for k in KINDS], [(2, SOURCES[k][2]) for k in KINDS], dtype)


FIXTURE_SETS = {
    "stereo": [("aiff-2ch.aiff", "aiff"), ("trueaudio.tta", "tta"), ("wavpack-combo.wv", "wv")],
    "mono": [("alac-allframes.m4a", "m4a"), ("shorten-lpc.shn", "shn"), ("wav-8bit.wav", "wav")],
}


@pytest.mark.parametrize("name", list(FIXTURE_SETS))
def test_load_batch_golden_fixtures(name):
    files = [(os.path.join(FIXTURES, f), kind) for f, kind in FIXTURE_SETS[name]]
    pcms, params = [], []
    for path, kind in files:
        a = classes()[kind][0](path)
        pcms.append(drain(a.to_pcm()))
        params.append((a.channels(), a.bits_per_sample()))
    images = [read(path) for path, _ in files]  # byte images open as filenames do
    for srcs in ([p for p, _ in files], images):
        batch = audiotools.load_batch(srcs, dtype=torch.float32)
        assert batch.errors == [None] * len(files)
        check_rows(batch, pcms, params, torch.float32)


def test_an_unreadable_file_is_a_zero_row(sources, tmp_path):
    whole = read(sources["flac"][0])
    srcs = [sources["wav"][0], whole[:len(whole) // 2], str(tmp_path / "is-not-there.flac"),
            b"not audio at all", sources["shn"][0]]
    batch = audiotools.load_batch(srcs)
    assert [type(e) for e in batch.errors] == [type(None), audiotools.DecodingError,
                                               audiotools.DecodingError,
                                               audiotools.DecodingError, type(None)]
    assert batch.lengths.tolist() == [2500, 0, 0, 0, 3]
    assert batch.sample_rates == [96000, 0, 0, 0, 44100]
    assert tuple(batch.audio.shape) == (5, 2, 2500)
    assert not batch.audio[1:4].any()
    check_rows(audiotools.tensors.AudioBatch(batch.audio[[0, 4]], batch.lengths[[0, 4]], None,
                                             None, None, None),
               [sources["wav"][1], sources["shn"][1]], [(2, 24), (2, 16)], torch.float32)
    # nothing readable at all: zero rows, no channels to tell
    none = audiotools.load_batch([b"junk", b""], frames=7)
    assert tuple(none.audio.shape) == (2, 0, 7) and none.lengths.tolist() == [0, 0]
    assert all(isinstance(e, audiotools.DecodingError) for e in none.errors)


class Stream(object):
    def __init__(self, seed=5):
        self.rng = np.random.RandomState(seed)

    def __call__(self, n):
        return self.rng.bytes(n)


@pytest.mark.parametrize("target", [dict(bits_per_sample=16), dict(channels=1, channel_mask=0x4),
                                    dict(sample_rate=48000, bits_per_sample=8)],
                         ids=["bits", "mono", "rate-bits"])
def test_targets_equal_convert_pcm_batch(sources, target):
    kinds = ["flac", "oga", "wav", "au", "aiff"]
    params = [(2, 0x3, SOURCES[k][2], SOURCES[k][3]) for k in kinds]
    want = audiotools.convert_pcm_batch([sources[k][1] for k in kinds], params, dither=Stream(),
                                        **target)
    batch = audiotools.load_batch([sources[k][0] for k in kinds], dither=Stream(), **target)
    assert batch.errors == [None] * len(kinds)
    ch = target.get("channels", 2)
    depths = [target.get("bits_per_sample", SOURCES[k][2]) for k in kinds]
    assert batch.bits_per_sample == depths
    assert batch.sample_rates == [target.get("sample_rate", SOURCES[k][3]) for k in kinds]
    assert batch.channel_masks == [MASKS[ch]] * len(kinds)
    check_rows(batch, want, [(ch, d) for d in depths], torch.float32)


def test_frames_pads(sources):
    batch = audiotools.load_batch([sources["aiff"][0], sources["shn"][0]], frames=1031,
                                  dtype=torch.float16)
    check_rows(batch, [sources["aiff"][1], sources["shn"][1]], [(2, 16), (2, 16)], torch.float16,
               t=1031)
    with pytest.raises(ValueError):
        audiotools.load_batch([sources["aiff"][0]], frames=99)


def test_differing_channel_counts_raise_before_decoding(sources, monkeypatch):
    from audiotools import batchfiles

    def no_decode(self):
        raise AssertionError("decoded")
    monkeypatch.setattr(batchfiles._Batch, "decode", no_decode)
    mono = os.path.join(FIXTURES, "wav-8bit.wav")
    with pytest.raises(ValueError) as e:
        audiotools.load_batch([sources["flac"][0], mono])
    assert "1, 2" in str(e.value) and "channels=" in str(e.value)


# ------------------------------------------------------------------- saving
def floats(rng, n, ch):
    """float32 in and a little past [-1, 1)"""
    return (rng.uniform(-1.05, 1.05, size=(ch, n))).astype(np.float32)


def from_pcm_writes(target, plane, depth, rate, mask, compression, n):
    ch = plane.shape[0]
    ints = pcm.FloatFrameList(plane[:, :n].T.reshape(-1).astype(np.float64).tolist(),
                              ch).to_int(depth)
    audiotools.FlacAudio.from_pcm(target, audiotools.FrameListReader(ints, rate, ch, depth, mask),
                                  compression, total_pcm_frames=n)
    return read(target)


SAVES = [
    ("mono 16", 1, 16, 44100, None, [1000, 0, 4097, 1]),
    ("stereo 24", 2, 24, 96000, None, [4097, 0, 2000]),
    ("six channels with a mask", 6, 16, 48000, 0x3F, [700, 4097]),
]


@pytest.mark.parametrize("compression", ["8", "0"])
@pytest.mark.parametrize("what,ch,depth,rate,mask,lengths", SAVES, ids=[s[0] for s in SAVES])
def test_save_flac_batch_writes_what_from_pcm_writes(what, ch, depth, rate, mask, lengths,
                                                     compression, tmp_path):
    rng = np.random.RandomState(ch)
    t = max(lengths) + 3
    host = np.stack([floats(rng, t, ch) for _ in lengths])
    targets = [str(tmp_path / ("%d.flac" % k)) for k in range(len(lengths))]
    got = audiotools.save_flac_batch(torch.from_numpy(host).cuda(), lengths, targets, rate, depth,
                                     mask, compression)
    for k, (g, n) in enumerate(zip(got, lengths)):
        assert isinstance(g, audiotools.FlacAudio), g
        assert (g.channels(), g.bits_per_sample(), g.sample_rate(), g.total_frames()) == (
            ch, depth, rate, n)
        want = from_pcm_writes(str(tmp_path / ("%d.ref.flac" % k)), host[k], depth, rate,
                               mask or 0, compression, n)
        assert read(targets[k]) == want, k  # SEEKTABLE, PADDING and MD5 included
    # a torch tensor of lengths and per-row lists are taken as well
    again = [str(tmp_path / ("%d.again.flac" % k)) for k in range(len(lengths))]
    audiotools.save_flac_batch(torch.from_numpy(host).cuda(), torch.tensor(lengths), again,
                               [rate] * len(lengths), [depth] * len(lengths), mask, compression)
    assert [read(a) for a in again] == [read(t) for t in targets]


def test_saved_files_load_back_exactly(tmp_path):
    lengths, depths = [4097, 10, 0, 2222], [16, 24, 8, 16]
    rates = [44100, 96000, 8000, 44100]
    t = max(lengths)
    host = np.zeros((4, 2, t), dtype=np.float32)
    for k, (n, d) in enumerate(zip(lengths, depths)):
        host[k, :, :n] = port.to_values(signals.make("noise", n, 2, d, seed=k + 1), 2, d, port.F32)
    audio = torch.from_numpy(host).cuda()
    targets = [str(tmp_path / ("%d.flac" % k)) for k in range(4)]
    got = audiotools.save_flac_batch(audio, lengths, targets, rates, depths)
    assert all(isinstance(g, audiotools.FlacAudio) for g in got), got
    batch = audiotools.load_batch(targets)
    assert batch.errors == [None] * 4 and batch.lengths.tolist() == lengths
    assert batch.sample_rates == rates and batch.bits_per_sample == depths
    assert np.array_equal(bits(batch.audio.cpu().numpy()), bits(host))


def test_a_slice_saves_as_its_contiguous_copy(tmp_path):
    rng = np.random.RandomState(11)
    audio = torch.from_numpy(np.stack([floats(rng, 3000, 2) for _ in range(3)])).cuda()
    view = audio[:, :, 3:-2]
    assert not view.is_contiguous() and view.stride(2) == 1
    lengths = [2995, 100, 2000]
    a = [str(tmp_path / ("a%d.flac" % k)) for k in range(3)]
    b = [str(tmp_path / ("b%d.flac" % k)) for k in range(3)]
    c = [str(tmp_path / ("c%d.flac" % k)) for k in range(3)]
    audiotools.save_flac_batch(view, lengths, a, 44100)
    audiotools.save_flac_batch(view.contiguous(), lengths, b, 44100)
    # a last stride of 2: the one case that is copied
    audiotools.save_flac_batch(audio[:, :, 3:-2:2], [1000] * 3, c, 44100)
    audiotools.save_flac_batch(audio[:, :, 3:-2:2].contiguous(), [1000] * 3,
                               [x + ".ref" for x in c], 44100)
    assert [read(x) for x in a] == [read(x) for x in b]
    assert [read(x) for x in c] == [read(x + ".ref") for x in c]
    want = from_pcm_writes(str(tmp_path / "ref.flac"), audio[0].cpu().numpy()[:, 3:], 16, 44100,
                           0, "8", 2995)
    assert read(a[0]) == want


def test_an_unwritable_target_returns_its_error(tmp_path):
    rng = np.random.RandomState(12)
    audio = torch.from_numpy(np.stack([floats(rng, 500, 2) for _ in range(3)])).cuda()
    targets = [str(tmp_path / "good1.flac"), str(tmp_path / "no-such-directory" / "x.flac"),
               str(tmp_path / "good2.flac")]
    got = audiotools.save_flac_batch(audio, [500, 500, 400], targets, 44100)
    assert [type(g) for g in got] == [audiotools.FlacAudio, audiotools.EncodingError,
                                      audiotools.FlacAudio]
    assert [os.path.exists(t) for t in targets] == [True, False, True]
    # a mask FLAC cannot write is that row's error as well
    got = audiotools.save_flac_batch(audio[:1], [500], [str(tmp_path / "mask.flac")], 44100,
                                     channel_mask=0x30)
    assert isinstance(got[0], audiotools.EncodingError)
    assert not os.path.exists(str(tmp_path / "mask.flac"))


# ------------------------------------------------------- the row functions
def test_rows_of_mixed_depths_go_there_and_back():
    """8- and 16-bit rows land in int16, the 24-bit row in int32, in one owner"""
    from audiotools import _atgpu
    depths, lengths = [8, 16, 24, 16], [1500, 7, 1031, 0]
    host = np.zeros((4, 3, 1500), dtype=np.float64)
    for k, (n, d) in enumerate(zip(lengths, depths)):
        host[k, :, :n] = port.to_values(signals.make("noise", n, 3, d, seed=k + 3), 3, d, port.F64)
    for dtype in (torch.float64, torch.float32):
        audio = torch.from_numpy(host).cuda().to(dtype)
        rows, owner = audiotools.tensor_to_pcm(audio, lengths, depths)
        assert [r.fmt for r in rows] == [_atgpu.PCM_S16, _atgpu.PCM_S16, _atgpu.PCM_S32,
                                         _atgpu.PCM_S16]
        for r in rows:
            width = 2 if r.fmt == _atgpu.PCM_S16 else 4
            assert (r.d_pcm + r.sample_offset * width) % 16 == 0 and r.sample_offset % 3 == 0
        assert [r.frames for r in rows] == lengths
        back, n = audiotools.pcm_to_tensor([(r, 3, d) for r, d in zip(rows, depths)], dtype)
        assert n.tolist() == lengths and back.dtype == dtype
        assert np.array_equal(bits(back.cpu().numpy()), bits(host.astype(back.cpu().numpy().dtype)))
    ints, n = audiotools.pcm_to_tensor([(r, 3, d) for r, d in zip(rows, depths)], torch.int32,
                                       frames=1503)
    assert tuple(ints.shape) == (4, 3, 1503) and owner.is_cuda
    assert np.array_equal(ints.cpu().numpy()[2, :, :1031],
                          port.to_values(signals.make("noise", 1031, 3, 24, seed=5), 3, 24,
                                         port.I32))
