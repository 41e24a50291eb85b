"""GPU: convert_files_batch with starts= / lengths= against the reader path
over the window cut to the stream, cls.from_pcm(PCMConverter(
BufferedPCMReader(PCMReaderWindow(source.to_pcm(), start, kept)), ...)), byte
for byte; one source per format, in the shapes of test_gpu_convert_files."""
import os

import pytest

import audiotools
from cdimage_cases import read, window_oracle, zeros
from test_gpu_convert_files import CD, KINDS, SOURCES, sources  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

BLOCK = 4096


def windows(n):
    """(start, length) -> as asked; the frames kept of an n-frame stream"""
    asked = [(0, None), (1, 1), (BLOCK - 1, 2), (n - 1, 5), (n, 3), (0, 0)]
    kept = []
    for start, length in asked:
        room = max(0, n - start)
        kept.append(room if length is None else min(length, room))
    return asked, kept


@pytest.mark.parametrize("kind", KINDS)
def test_windows_of_one_source(sources, tmp_path, kind):
    path = sources[kind][0]
    n, ch, bits, rate = SOURCES[kind]
    asked, kept = windows(n)
    targets = [str(tmp_path / ("%s.%d.flac" % (kind, k))) for k in range(len(asked))]
    got = audiotools.convert_files_batch([path] * len(asked), targets,
                                         starts=[a for a, _ in asked],
                                         lengths=[b for _, b in asked])
    for k, ((start, _), frames, t, g) in enumerate(zip(asked, kept, targets, got)):
        assert isinstance(g, audiotools.FlacAudio), (kind, k, g)
        assert g.total_frames() == frames, (kind, k)
        want = window_oracle(kind, path, str(tmp_path / ("ref%d.flac" % k)), "flac",
                             min(start, n), frames)
        assert read(t) == want, (kind, k)


def test_one_value_for_all_and_a_conversion(sources, tmp_path):
    kinds = ["flac", "au", "wav"]   # 24 bits each
    targets = [str(tmp_path / (k + ".wv")) for k in kinds]
    got = audiotools.convert_files_batch([sources[k][0] for k in kinds], targets, starts=97,
                                         lengths=BLOCK + 1, bits_per_sample=16, dither=zeros,
                                         target_types="wv")
    for k, t, g in zip(kinds, targets, got):
        assert isinstance(g, audiotools.WavPackAudio), (k, g)
        frames = min(BLOCK + 1, SOURCES[k][0] - 97)
        assert read(t) == window_oracle(k, sources[k][0], str(tmp_path / (k + ".ref.wv")), "wv", 97,
                                        frames, bits_per_sample=16), k
    # lengths alone: from the start
    one = str(tmp_path / "head.flac")
    got = audiotools.convert_files_batch([sources["tta"][0]], [one], lengths=10)
    assert read(one) == window_oracle("tta", sources["tta"][0], str(tmp_path / "head.ref.flac"),
                                      "flac", 0, 10)
    # a WAVE target's header holds the window's length
    wav = str(tmp_path / "cut.wav")
    got = audiotools.convert_files_batch([sources["m4a"][0]], [wav], starts=[4000], lengths=[500],
                                         target_types="suffix")
    assert got[0].total_frames() == 96
    assert read(wav) == window_oracle("m4a", sources["m4a"][0], str(tmp_path / "cut.ref.wav"),
                                      "wav", 4000, 96)


def test_without_the_keywords_nothing_changes(sources, tmp_path):
    kinds = ["flac", "shn", "wv"]
    a = [str(tmp_path / (k + ".a.flac")) for k in kinds]
    b = [str(tmp_path / (k + ".b.flac")) for k in kinds]
    audiotools.convert_files_batch([sources[k][0] for k in kinds], a, dither=zeros, **CD)
    audiotools.convert_files_batch([sources[k][0] for k in kinds], b, dither=zeros, starts=None,
                                   lengths=None, **CD)
    assert [read(p) for p in a] == [read(p) for p in b]


def test_a_source_in_three_rows_goes_up_once(sources, tmp_path, monkeypatch):
    from audiotools import _atgpu
    path = sources["wv"][0]
    uploads = []
    real = _atgpu.Engine.copy_to_device

    def counting(self, d_dst, src):
        uploads.append(len(src))
        return real(self, d_dst, src)
    monkeypatch.setattr(_atgpu.Engine, "copy_to_device", counting)
    targets = [str(tmp_path / ("row%d.flac" % k)) for k in range(3)]
    got = audiotools.convert_files_batch([path] * 3, targets, starts=[0, 0, 10],
                                         lengths=[None, None, None])
    assert all(isinstance(g, audiotools.FlacAudio) for g in got)
    # one upload holds the source's bytes, once (its blocks and some slack),
    # whatever the rows; the others (tables, no PCM) are small beside it
    size = os.path.getsize(path)
    big = [u for u in uploads if u >= size // 2]
    assert len(big) == 1 and big[0] <= size + 128, uploads


def test_refusals_come_before_any_gpu_work(sources, tmp_path, monkeypatch):
    from audiotools import _atgpu
    path = sources["aiff"][0]
    audiotools.batchfiles._open(read(path))  # the library is loaded by now
    monkeypatch.setattr(_atgpu, "engine", lambda: pytest.fail("GPU work was begun"))
    for kw in (dict(starts=-1), dict(starts=0, lengths=-1), dict(starts=[0, -5], lengths=[1, 1])):
        with pytest.raises(ValueError):
            audiotools.convert_files_batch([path, path], [str(tmp_path / "a.flac"),
                                                          str(tmp_path / "b.flac")], **kw)
    with pytest.raises(ValueError):
        audiotools.convert_files_batch([path], [str(tmp_path / "a.flac")], starts=[0, 0])
    assert not os.path.exists(str(tmp_path / "a.flac"))
