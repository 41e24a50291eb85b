"""GPU: audiotools.join_tracks_batch against the reader path it replaces,
cls.from_pcm(target, PCMCat([f.to_pcm() for f in files]), compression,
total_pcm_frames=<sum>), byte for byte.  The pieces are 1, 588, 4097 and 3
frames of mono 16-bit audio in four formats: every piece starts at another
sample alignment in the image, and the long one crosses a FLAC block."""
import os

import numpy as np
import pytest

import signals
import audiotools
from audiotools import DecodingError, FlacAudio
from cdimage_cases import classes, from_pcm_kw, read, sheet_at, write_source

pytestmark = pytest.mark.gpu

PIECES = [("flac", 1), ("tta", 588), ("wv", 4097), ("wav", 3)]
STARTS = [0, 1, 589, 4686]
TOTAL = 4689


@pytest.fixture(scope="module")
def pieces(tmp_path_factory):
    d = tmp_path_factory.mktemp("join_src")
    out = []
    for k, (kind, n) in enumerate(PIECES):
        x = signals.make("noise", n, 1, 16, seed=40 + k)
        out.append((kind, write_source(kind, str(d / ("piece%d.%s" % (k, kind))), x, 44100, 1, 16),
                    x))
    return out


def cat_oracle(files, target, suffix, compression=None, sheet=None):
    """the reader path: [(kind, path)] -> the file's bytes"""
    readers = [classes()[kind][0](path).to_pcm() for kind, path in files]
    total = sum(classes()[kind][0](path).total_frames() for kind, path in files)
    cls = audiotools.targets.SUFFIXES[suffix]
    out = cls.from_pcm(target, audiotools.PCMCat(readers), compression, total_pcm_frames=total,
                       **from_pcm_kw(suffix))
    if sheet is not None:
        out.set_cuesheet(sheet)
    return read(target)


@pytest.mark.parametrize("suffix,compression", [("flac", "8"), ("flac", "0"), ("wav", None),
                                                ("wv", None)])
def test_four_formats_into_one_image(pieces, tmp_path, suffix, compression):
    files = [(kind, path) for kind, path, _ in pieces]
    target = str(tmp_path / ("image." + suffix))
    got = audiotools.join_tracks_batch([[p for _, p in files]], [target], target_types=suffix,
                                       compression=compression)
    assert type(got[0]) is audiotools.targets.SUFFIXES[suffix], got[0]
    assert got[0].total_frames() == TOTAL
    assert read(target) == cat_oracle(files, str(tmp_path / ("ref." + suffix)), suffix, compression)
    from test_gpu_convert_files import drain
    assert np.array_equal(drain(got[0].to_pcm()),
                          np.concatenate([x for _, _, x in pieces]).astype(np.int32))


def test_sheet_embedded_in_a_flac_image(pieces, tmp_path):
    files = [(kind, path) for kind, path, _ in pieces]
    sheet = sheet_at(44100, STARTS, {3: 300}, catalog_number="0000000000017")
    sheet_file = str(tmp_path / "image.cue")
    whole = sheet_at(44100, [0, 588, 4116])  # a .cue file holds whole sectors
    with open(sheet_file, "w", newline="") as f:
        audiotools.cue.write_cuesheet(whole, "image.flac", f)
    targets = [str(tmp_path / "a.flac"), str(tmp_path / "b.flac"), str(tmp_path / "c.wav")]
    got = audiotools.join_tracks_batch([[p for _, p in files]] * 3, targets,
                                       sheets=[sheet, sheet_file, sheet],
                                       target_types="suffix")
    assert read(targets[0]) == cat_oracle(files, str(tmp_path / "ref.a.flac"), "flac", None, sheet)
    assert read(targets[1]) == cat_oracle(files, str(tmp_path / "ref.b.flac"), "flac", None, whole)
    assert got[0].get_cuesheet() == sheet and FlacAudio(targets[0]).get_cuesheet() == sheet
    assert got[1].get_cuesheet() == whole
    # a type that carries no sheet is written as without one
    assert read(targets[2]) == cat_oracle(files, str(tmp_path / "ref.c.wav"), "wav")
    # and the joined image splits by its own sheet into the pieces' files
    back = [str(tmp_path / ("back%d.%s" % (k, kind))) for k, (kind, _) in enumerate(PIECES)]
    split = audiotools.split_image_batch([targets[0]], [back], target_types=["suffix"])
    for (kind, path, _), b, t in zip(pieces, back, split[0].tracks):
        assert type(t) is classes()[kind][0], (kind, t)
        assert read(b) == read(path), kind


def test_mismatches_are_refused_with_trackcats_words(pieces, tmp_path):
    base = signals.make("noise", 50, 1, 16, seed=1)
    mono = write_source("wav", str(tmp_path / "mono.wav"), base, 44100, 1, 16)
    cases = [
        (write_source("flac", str(tmp_path / "rate.flac"), base, 48000, 1, 16),
         "all audio files must have the same sample rate"),
        (write_source("tta", str(tmp_path / "stereo.tta"), signals.make("noise", 50, 2, 16, seed=2),
                      44100, 2, 16), "all audio files must have the same channel count"),
        (write_source("au", str(tmp_path / "bits.au"), signals.make("noise", 50, 1, 24, seed=3),
                      44100, 1, 24), "all audio files must have the same bits per sample"),
    ]
    masks = []
    for mask in (0x7, 0xB):
        path = str(tmp_path / ("mask%x.wav" % mask))
        audiotools.WaveAudio.from_pcm(path, audiotools.FrameListReader(
            signals.make("noise", 50, 3, 16, seed=mask), 44100, 3, 16, mask), total_pcm_frames=50)
        masks.append(path)
    albums = [[mono, other] for other, _ in cases] + [masks, [mono, pieces[1][1]]]
    targets = [str(tmp_path / ("out%d.flac" % k)) for k in range(len(albums))]
    sheets = [None] * 4 + [sheet_at(44100, [0, 0])]
    got = audiotools.join_tracks_batch(albums, targets, sheets=sheets)
    messages = [m for _, m in cases] + ["all audio files must have the same channel assignment",
                                        "cuesheet not formatted for disc images"]
    for g, m, t in zip(got, messages, targets):
        assert isinstance(g, ValueError) and str(g) == m, (g, m)
        assert not os.path.exists(t)
    got = audiotools.join_tracks_batch([[mono, pieces[1][1]]], [targets[0]],
                                       sheets=[sheet_at(44100, [0, 639])])
    assert isinstance(got[0], ValueError)
    assert str(got[0]) == "cuesheet too long for track being split"
    # a last track of no frames is let through, as trackcat lets it
    got = audiotools.join_tracks_batch([[mono, pieces[1][1]]], [targets[0]],
                                       sheets=[sheet_at(44100, [0, 638])])
    assert isinstance(got[0], FlacAudio) and got[0].total_frames() == 638


def test_three_albums_and_a_bad_piece_in_one_call(pieces, tmp_path):
    files = [(kind, path) for kind, path, _ in pieces]
    damaged = bytearray(read(pieces[2][1]))
    damaged[len(damaged) // 2] ^= 0x04
    albums = [[p for _, p in files],
              [files[1][1], bytes(damaged), files[0][1]],
              [files[3][1], files[3][1], files[2][1], files[1][1]],
              [files[2][1]]]
    targets = [str(tmp_path / ("album%d.flac" % k)) for k in range(4)]
    got = audiotools.join_tracks_batch(albums, targets)
    assert isinstance(got[1], DecodingError), got[1]
    assert not os.path.exists(targets[1])
    for k, order in ((0, [0, 1, 2, 3]), (2, [3, 3, 2, 1]), (3, [2])):
        assert isinstance(got[k], FlacAudio), got[k]
        assert read(targets[k]) == cat_oracle([files[i] for i in order],
                                              str(tmp_path / ("ref%d.flac" % k)), "flac"), k
