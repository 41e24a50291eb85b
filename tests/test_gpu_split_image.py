"""GPU: audiotools.split_image_batch against the reader path it replaces,
cls.from_pcm(PCMConverter(BufferedPCMReader(PCMReaderWindow(image.to_pcm(),
offset, length)), ...)) once per track, byte for byte.

The main image is 32 CD sectors (18,816 frames) of 44.1 kHz stereo 16-bit
audio cut 7 / 1 / 13 / 2 / 9 sectors, tracks 3 and 5 with an index 0 in
front of their index 1: at a block size of 4096 every cut falls inside a
FLAC frame, and track 2 is shorter than a block."""
import os
import types

import numpy as np
import pytest

import dither_port as port
import signals
import audiotools
from audiotools import DecodingError, SheetException, SplitResult, accuraterip, cue
from cdimage_cases import (TYPES, cuts_of, from_pcm_kw, read, sheet_at, window_oracle,  # noqa: F401
                           write_source, zeros)
from test_gpu_convert_files import KINDS

pytestmark = pytest.mark.gpu

SECTOR = 588
STARTS = [SECTOR * s for s in (0, 7, 8, 21, 23)]
TOTAL = SECTOR * 32
CUTS = cuts_of(STARTS, TOTAL)
SEED = 0x5EEDC0FFEE123457


@pytest.fixture(autouse=True)
def still_clock(monkeypatch):
    monkeypatch.setattr(audiotools.m4a, "time", types.SimpleNamespace(time=lambda: 1.7e9))


def cd_sheet():
    # index 0 of track 3 lies inside the one-sector track 2, 300 frames in
    return sheet_at(44100, STARTS, {3: 7 * SECTOR + 300, 5: 22 * SECTOR}, catalog_number="1234567890123")


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    """the CD image in each of the nine formats -> {kind: path}, and its samples"""
    d = tmp_path_factory.mktemp("split_src")
    x = signals.make("tone", TOTAL, 2, 16, seed=71)
    return {k: write_source(k, str(d / ("image." + k)), x, 44100, 2, 16) for k in KINDS}, x


def check_tracks(result, kind, path, targets, suffixes, cuts, tmp_path, **kw):
    assert isinstance(result, SplitResult), result
    assert len(result.tracks) == len(cuts)
    for j, ((offset, n), t, s, got) in enumerate(zip(cuts, targets, suffixes, result.tracks)):
        ref = str(tmp_path / ("ref%d.%s.%s" % (j, kind, s)))
        want = window_oracle(kind, path, ref, s, offset, n, t if os.path.exists(t) else None, **kw)
        if isinstance(want, Exception):
            assert type(got) is type(want) and str(got) == str(want).replace(ref, t), (kind, j)
            assert not os.path.exists(t)
        else:
            assert type(got) is audiotools.targets.SUFFIXES[s], (kind, j, got)
            assert got.total_frames() == n
            assert read(t) == want, (kind, j, s)


@pytest.mark.parametrize("kind", KINDS)
def test_each_source_format_to_flac(images, tmp_path, kind):
    paths, _ = images
    targets = [str(tmp_path / ("%s.%d.flac" % (kind, j))) for j in range(5)]
    got = audiotools.split_image_batch([paths[kind]], [targets], [cd_sheet()], compression="8")
    check_tracks(got[0], kind, paths[kind], targets, ["flac"] * 5, CUTS, tmp_path, compression="8")
    assert got[0].checksums is None and got[0].offsets is None
    assert got[0].stats["decoded_frames"] == TOTAL
    assert got[0].stats["uploaded_bytes"] == os.path.getsize(paths[kind])
    assert got[0].stats["encode_calls"] == 1


@pytest.mark.parametrize("suffix", TYPES)
def test_flac_image_to_each_type(images, tmp_path, suffix):
    paths, _ = images
    targets = [str(tmp_path / ("t%d.%s" % (j, suffix))) for j in range(5)]
    # the sheet from a .cue file this time: whole sectors, so without the
    # index 0 of track 3, which changes no cut
    sheet_file = str(tmp_path / "image.cue")
    with open(sheet_file, "w", newline="") as f:
        cue.write_cuesheet(sheet_at(44100, STARTS, {5: 22 * SECTOR}), "image.flac", f)
    got = audiotools.split_image_batch([paths["flac"]], [targets], [sheet_file],
                                       target_types=suffix)
    check_tracks(got[0], "flac", paths["flac"], targets, [suffix] * 5, CUTS, tmp_path)


def test_types_and_compression_per_track(images, tmp_path):
    paths, _ = images
    suffixes = ["flac", "wav", "tta", "flac", "wv"]
    targets = [str(tmp_path / ("p%d.%s" % (j, s))) for j, s in enumerate(suffixes)]
    got = audiotools.split_image_batch([paths["wv"]], [targets], [cd_sheet()],
                                       target_types=["suffix"], compression=[["0", None, None,
                                                                              "8", "veryfast"]])
    for j, mode in enumerate(["0", None, None, "8", "veryfast"]):
        check_tracks(SplitResult(got[0].tracks[j:j + 1], None, None, {}), "wv", paths["wv"],
                     targets[j:j + 1], suffixes[j:j + 1], CUTS[j:j + 1], tmp_path,
                     compression=mode)
    # FLAC-0 and FLAC-8 tracks differ in padding or preset: at least two FLAC calls
    assert got[0].stats["encode_calls"] >= 4


@pytest.mark.parametrize("case", ["cue-file", "whole-samples"])
def test_8000_hz_mono(tmp_path, case):
    """a CD frame is 106 2/3 samples at 8000 Hz, so no track but the first
    starts on a multiple of 4 samples.  cue-file: index 1 at CD frames 0, 1,
    2 and 4, the differences cut to 106, 106 and 213; whole-samples: a Sheet
    whose offsets are the samples 0, 106, 213 and 426, cuts of 106, 107 and
    213"""
    total = 1000
    x = signals.make("noise", total, 1, 16, seed=5)
    image = write_source("tta", str(tmp_path / "image.tta"), x, 8000, 1, 16)
    if case == "cue-file":
        sheet = str(tmp_path / "image.cue")
        with open(sheet, "w") as f:
            f.write('FILE "image.tta" WAVE\n' + "".join(
                "  TRACK %02d AUDIO\n    INDEX 01 00:00:%02d\n" % (n + 1, at)
                for n, at in enumerate((0, 1, 2, 4))))
        cuts = [(0, 106), (106, 106), (212, 213), (425, 575)]
    else:
        sheet = sheet_at(8000, [0, 106, 213, 426])
        cuts = [(0, 106), (106, 107), (213, 213), (426, 574)]
    targets = [str(tmp_path / ("t%d.flac" % j)) for j in range(4)]
    got = audiotools.split_image_batch([image], [targets], [sheet])
    check_tracks(got[0], "tta", image, targets, ["flac"] * 4, cuts, tmp_path)


def test_embedded_sheet_of_a_surround_image(tmp_path):
    """48 kHz, 24 bits, 6 channels, cut by the sheet the FLAC file carries"""
    total = 4096 + 2001
    x = signals.make("tone", total, 6, 24, seed=9)
    image = write_source("flac", str(tmp_path / "image.flac"), x, 48000, 6, 24)
    starts = [0, 1001, 4095, 4099]
    sheet = sheet_at(48000, starts, {2: 999})
    # without a sheet of either kind the image is refused, with tracksplit's words
    got = audiotools.split_image_batch([image], [["a", "b"]])
    assert isinstance(got[0], SheetException)
    assert str(got[0]) == "you must specify a cuesheet to split audio file"
    audiotools.FlacAudio(image).set_cuesheet(sheet)
    assert audiotools.FlacAudio(image).get_cuesheet() == sheet
    targets = [str(tmp_path / ("t%d.flac" % j)) for j in range(4)]
    got = audiotools.split_image_batch([image], [targets], sheets=None)
    check_tracks(got[0], "flac", image, targets, ["flac"] * 4, cuts_of(starts, total), tmp_path)
    assert b"WAVEFORMATEXTENSIBLE_CHANNEL_MASK=0x003F" in read(targets[1])
    # another format carries no sheet
    wav = write_source("wav", str(tmp_path / "image.wav"), x, 48000, 6, 24)
    got = audiotools.split_image_batch([wav], [targets])
    assert isinstance(got[0], SheetException)


class StreamDither(object):
    """the k-th draw gets the head of the port's stream streams[k]"""

    def __init__(self, streams):
        self.streams, self.draws = list(streams), 0

    def __call__(self, n):
        self.draws += 1
        return port.stream_bytes(SEED, self.streams[self.draws - 1], n)


class OneStream(object):
    """the reader path's source of one track: the bytes of one stream of the
    port, on from where the draw before ended"""

    def __init__(self, stream):
        self.stream, self.at = stream, 0

    def __call__(self, n):
        self.at += n
        return port.stream_bytes(SEED, self.stream, n, first_byte=self.at - n)


def test_24_to_16_bits_while_splitting(tmp_path):
    """two 24-bit images of 2 and 3 tracks in one call: under an all-zero
    dither, and under a DeviceDither, which gives track j of image k the
    stream (tracks before image k) + j -- the same bytes a callable gives that
    hands out those streams of the port, in the call and in the reader path"""
    totals, starts = [4096 + 300, 5000], [[0, 4095], [0, 1, 4098]]
    xs = [signals.make("tone", n, 2, 24, seed=30 + k) for k, n in enumerate(totals)]
    kinds = ["flac", "au"]
    images = [write_source(kind, str(tmp_path / ("image%d.%s" % (k, kind))), x, 44100, 2, 24)
              for k, (kind, x) in enumerate(zip(kinds, xs))]
    sheets = [sheet_at(44100, s) for s in starts]

    def run(name, dither):
        targets = [[str(tmp_path / ("%s.%d.%d.flac" % (name, k, j))) for j in range(len(s))]
                   for k, s in enumerate(starts)]
        got = audiotools.split_image_batch(images, targets, sheets, bits_per_sample=16,
                                           dither=dither)
        assert all(isinstance(g, SplitResult) for g in got), got
        return targets, got

    targets, got = run("zero", zeros)
    for k in range(2):
        check_tracks(got[k], kinds[k], images[k], targets[k], ["flac"] * len(starts[k]),
                     cuts_of(starts[k], totals[k]), tmp_path, bits_per_sample=16)
    device, got = run("device", audiotools.DeviceDither(SEED))
    ported, _ = run("port", StreamDither(range(5)))
    stream = 0
    for k in range(2):
        for j, (offset, n) in enumerate(cuts_of(starts[k], totals[k])):
            want = window_oracle(kinds[k], images[k], str(tmp_path / "ref.flac"), "flac", offset, n,
                                 rand=OneStream(stream), bits_per_sample=16)
            assert read(device[k][j]) == want, (k, j)
            assert read(ported[k][j]) == want, (k, j)
            if n >= 64:  # 128 dither bits or more are not all zero
                assert read(targets[k][j]) != want, (k, j)
            stream += 1


def test_three_images_and_their_failures_in_one_call(images, tmp_path):
    """a damaged image, an over-long sheet and one file named twice with two
    sheets: each failure is its image's alone, and the file named twice goes
    up once"""
    paths, _ = images
    damaged = bytearray(read(paths["flac"]))
    damaged[len(damaged) - 1000] ^= 0x10
    too_long = sheet_at(44100, [0, TOTAL])
    halves = sheet_at(44100, [0, 9999])
    names = ["damaged", "long", "five", "two"]
    counts = [5, 2, 5, 2]
    targets = [[str(tmp_path / ("%s.%d.flac" % (name, j))) for j in range(c)]
               for name, c in zip(names, counts)]
    got = audiotools.split_image_batch(
        [bytes(damaged), paths["tta"], paths["wv"], paths["wv"]], targets,
        [cd_sheet(), too_long, cd_sheet(), halves])
    assert isinstance(got[0], DecodingError), got[0]
    assert isinstance(got[1], SheetException)
    assert str(got[1]) == "cuesheet too long for track being split"
    assert not any(os.path.exists(t) for t in targets[0] + targets[1])
    check_tracks(got[2], "wv", paths["wv"], targets[2], ["flac"] * 5, CUTS, tmp_path)
    check_tracks(got[3], "wv", paths["wv"], targets[3], ["flac"] * 2,
                 cuts_of([0, 9999], TOTAL), tmp_path)
    size = os.path.getsize(paths["wv"])
    assert [got[2].stats["uploaded_bytes"], got[3].stats["uploaded_bytes"]] == [size, 0]
    assert [got[2].stats["decoded_frames"], got[3].stats["decoded_frames"]] == [TOTAL, 0]
    # a wrong number of targets and a sheet not made for an image, likewise
    got = audiotools.split_image_batch(
        [paths["au"], paths["au"], paths["shn"]],
        [targets[0][:4], targets[0], [str(tmp_path / ("ok.%d.flac" % j)) for j in range(2)]],
        [cd_sheet(), sheet_at(44100, [0, 0, 1, 2, 3]), halves])
    assert isinstance(got[0], ValueError) and not isinstance(got[0], SheetException)
    assert isinstance(got[1], SheetException)
    assert str(got[1]) == "cuesheet not formatted for disc images"
    assert isinstance(got[2], SplitResult)
    assert all(isinstance(t, audiotools.FlacAudio) for t in got[2].tracks)


def test_24_bits_into_shorten_is_that_tracks_error(tmp_path):
    x = signals.make("tone", 3000, 2, 24, seed=3)
    image = write_source("wav", str(tmp_path / "image.wav"), x, 44100, 2, 24)
    targets = [str(tmp_path / "a.shn"), str(tmp_path / "b.flac"), str(tmp_path / "c.shn")]
    got = audiotools.split_image_batch([image], [targets], [sheet_at(44100, [0, 1000, 2000])],
                                       target_types=[["shn", "flac", "shn"]])
    check_tracks(got[0], "wav", image, targets, ["shn", "flac", "shn"],
                 cuts_of([0, 1000, 2000], 3000), tmp_path)
    assert isinstance(got[0].tracks[0], audiotools.EncodingError)
    assert isinstance(got[0].tracks[1], audiotools.FlacAudio)


def test_accuraterip_of_the_tracks_in_place(images, tmp_path):
    paths, x = images
    tracks = [accuraterip.track(offset, n, 44100, is_first=(j == 0), is_last=(j == 4),
                                lo_frame=0, hi_frame=TOTAL) for j, (offset, n) in enumerate(CUTS)]
    want, want_table = accuraterip.checksum_batch(x.astype(np.int16), tracks, max_offset=7)
    targets = [[str(tmp_path / ("%s.%d.flac" % (k, j))) for j in range(5)] for k in ("a", "b")]
    mono = write_source("tta", str(tmp_path / "mono.tta"),
                        signals.make("tone", 3000, 1, 16, seed=4), 44100, 1, 16)
    got = audiotools.split_image_batch(
        [paths["flac"], paths["m4a"], mono], targets + [[str(tmp_path / "m.flac")]],
        [cd_sheet(), cd_sheet(), sheet_at(44100, [0])], accuraterip=True, max_offset=7)
    for g in got[:2]:
        assert g.checksums == [(int(a), int(b)) for a, b in want]
        assert g.offsets.shape == (5, 15) and np.array_equal(g.offsets, want_table)
        assert [c[0] for c in g.checksums] == [int(v) for v in g.offsets[:, 7]]
    # not CD audio: no checksums, and the file still written
    assert got[2].checksums is None and got[2].offsets is None
    assert isinstance(got[2].tracks[0], audiotools.FlacAudio)
    # without max_offset there is no table
    got = audiotools.split_image_batch([paths["flac"]], [targets[0]], [cd_sheet()],
                                       accuraterip=True)
    assert got[0].checksums == [(int(a), int(b)) for a, b in want] and got[0].offsets is None
    check_tracks(got[0], "flac", paths["flac"], targets[0], ["flac"] * 5, CUTS, tmp_path)


def test_accuraterip_with_tracks_longer_than_a_seek_interval(tmp_path):
    """a FLAC image into four FLAC tracks of more than 10 s each: finishing
    such a track decodes the encoder's image on the decoder handle that holds
    the image's PCM, so the checksums have to be taken before it.  A sheet
    with an index-less track beside it is its own image's error."""
    interval = 441000
    starts = [0, interval + SECTOR, 2 * interval + 3 * SECTOR, 3 * interval + 4 * SECTOR]
    total = 4 * interval + 9 * SECTOR
    cuts = cuts_of(starts, total)
    x = signals.make("tone", total, 2, 16, seed=12)
    image = write_source("flac", str(tmp_path / "long.flac"), x, 44100, 2, 16)
    tracks = [accuraterip.track(offset, n, 44100, is_first=(j == 0), is_last=(j == 3),
                                lo_frame=0, hi_frame=total) for j, (offset, n) in enumerate(cuts)]
    want, want_table = accuraterip.checksum_batch(x.astype(np.int16), tracks, max_offset=5)
    targets = [str(tmp_path / ("long.%d.flac" % j)) for j in range(4)]
    bad = cue.read_cuesheet_string('FILE "a" WAVE\nTRACK 01 AUDIO\nINDEX 01 00:00:00\n'
                                   "TRACK 02 AUDIO\n")
    got = audiotools.split_image_batch([image, image], [["x", "y"], targets],
                                       [bad, sheet_at(44100, starts)], accuraterip=True,
                                       max_offset=5)
    assert isinstance(got[0], SheetException)
    assert str(got[0]) == "a track of the cuesheet has no index"
    assert got[1].checksums == [(int(a), int(b)) for a, b in want]
    assert np.array_equal(got[1].offsets, want_table)
    for t, (_, n), g in zip(targets, cuts, got[1].tracks):
        assert isinstance(g, audiotools.FlacAudio) and g.total_frames() == n
        # two seek points: the finishing walked the encoder's image
        data = read(t)
        assert data[4 + 4 + 34] & 0x7F == 3
        assert int.from_bytes(data[4 + 4 + 34 + 1:4 + 4 + 34 + 4], "big") == 2 * 18
    # the first track, from the head of the image, is the file the reader path writes
    assert read(targets[0]) == window_oracle("flac", image, str(tmp_path / "ref.flac"), "flac",
                                             0, cuts[0][1])


def test_checksums_of_an_image_at_an_odd_sample_offset():
    """an image whose first sample is an odd one of its decoder's output (a
    stereo file behind a mono one): the pass takes whole frames from a
    16-byte boundary, so the image is copied to one first"""
    from collections import namedtuple
    from audiotools import _atgpu, cdimage
    from audiotools.batchfiles import _Pcm
    x = signals.make("tone", TOTAL, 2, 16, seed=71).astype(np.int32)
    eng = _atgpu.engine()
    lead = 3
    host = np.concatenate([np.full(lead, 12345, dtype=np.int32), x, np.zeros(5, dtype=np.int32)])
    d = eng.device_alloc(host.nbytes)
    free = []
    try:
        eng.copy_to_device(d, host)
        Header = namedtuple("Header", "sample_rate channels bits_per_sample")
        Batch = namedtuple("Batch", "headers views")
        batch = Batch([Header(44100, 2, 16)], {0: (d, _Pcm(True, lead, TOTAL))})
        got = cdimage._checksums(eng, free, batch, 0, CUTS,
                                 SplitResult([None] * 5, None, None, {}), 7)
        assert len(free) == 1
    finally:
        for p in free + [d]:
            eng.device_free(p)
    tracks = [accuraterip.track(offset, n, 44100, is_first=(j == 0), is_last=(j == 4),
                                lo_frame=0, hi_frame=TOTAL) for j, (offset, n) in enumerate(CUTS)]
    want, want_table = accuraterip.checksum_batch(x, tracks, max_offset=7)
    assert got.checksums == [(int(a), int(b)) for a, b in want]
    assert np.array_equal(got.offsets, want_table)
