"""GPU: decode_windows_batch.  For one source in each of the nine formats
(written by the existing writers; 1, 2 and 6 channels, 16 and 24 bits) every
window of the start/length grid equals the source PCM sliced, which is what
the full decode gives; the FLAC source comes with from_pcm's SEEKTABLE, with
none and with placeholder points only.  Then a mixed 60-row call with one file
in 8 rows, unreadable and damaged sources, and the work bound that keeps a
silent whole-file decode from passing."""
import itertools
import os

import numpy as np
import pytest

import decode_cases
import flac_index_port
import oracle_port
import signals
import audiotools
from audiotools import _atgpu, flac
from test_gpu_convert_files import MASKS, classes

pytestmark = pytest.mark.gpu

# kind -> (frames, channels, bits, rate, nominal unit in frames): low rates
# keep the PCM small and the units many
SOURCES = {
    "flac": (8000 * 25 + 1, 1, 16, 8000, 4096),
    "flac6": (4096 * 6 + 100, 6, 24, 96000, 4096),
    "oga": (4096 * 4 + 9, 2, 16, 8000, 4096),
    "m4a": (4096 * 5 + 100, 2, 16, 8000, 4096),
    "tta": (8359 * 3 + 500, 1, 16, 8000, 8359),
    "wv": (44100 * 3 + 77, 2, 16, 44100, 44100),
    "shn": (256 * 9 + 3, 2, 16, 8000, 256),
    "wav": (5000, 6, 24, 96000, 1024),
    "aiff": (3000, 2, 16, 44100, 1024),
    "au": (4500, 2, 24, 44100, 1024),
}
CLASS_OF = {"flac6": "flac"}
EXACT = {k: k not in ("oga", "shn") for k in SOURCES}


def rewrite_seektable(data, how):
    """a .flac image without its SEEKTABLE, or with placeholder points only"""
    blocks, frames_at = flac._blocks(data)
    out = []
    for t, body in blocks:
        if t == flac.SEEKTABLE:
            if how == "none":
                continue
            body = (b"\xff" * 8 + bytes(10)) * (len(body) // 18)
        out.append((t, body))
    return flac._build(out) + data[frames_at:]


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    d = tmp_path_factory.mktemp("window_src")
    out = {}
    for k, (kind, (n, ch, bits, rate, _)) in enumerate(SOURCES.items()):
        x = signals.make("tone", n, ch, bits, seed=70 + k)
        cls, kw = classes()[CLASS_OF.get(kind, kind)]
        path = str(d / ("source." + kind))
        cls.from_pcm(path, audiotools.FrameListReader(x, rate, ch, bits, MASKS[ch]),
                     total_pcm_frames=n, **kw)
        out[kind] = (path, x)
    data = open(out["flac"][0], "rb").read()
    assert len(_atgpu.read_metadata(data)[2]) == 3  # a point per 10 s
    for how in ("none", "placeholders"):
        path = str(d / ("source.%s.flac" % how))
        with open(path, "wb") as f:
            f.write(rewrite_seektable(data, how))
        out["flac-" + how] = (path, out["flac"][1])
        SOURCES["flac-" + how] = SOURCES["flac"]
        EXACT["flac-" + how] = True
    pts = _atgpu.read_metadata(open(out["flac-placeholders"][0], "rb").read())[2]
    assert len(pts) == 3 and all(s == 0xFFFFFFFFFFFFFFFF for s, _, _ in pts)
    assert _atgpu.read_metadata(open(out["flac-none"][0], "rb").read())[2] == []
    return out


def grid(kind, points=()):
    n, _, _, _, unit = SOURCES[kind]
    starts = {0, 1, unit - 1, unit, unit + 1, n - 1, n, n + 5}
    for p in points:
        starts |= {p - 1, p, p + 1}
    return list(itertools.product(sorted(s for s in starts if s >= 0), [0, 1, unit, None, n + 7]))


def want(x, ch, start, length):
    n = len(x) // ch
    stop = n if length is None else min(n, start + length)
    return x[min(start, n) * ch:max(stop, min(start, n)) * ch]


KINDS = ["flac", "flac-none", "flac-placeholders", "flac6", "oga", "m4a", "tta", "wv", "shn",
         "wav", "aiff", "au"]


@pytest.mark.parametrize("kind", KINDS)
def test_every_window_of_the_grid(sources, kind):
    path, x = sources[kind]
    n, ch, bits, rate, _ = SOURCES[kind]
    points = [s for s, _, _ in _atgpu.read_metadata(open(path, "rb").read())[2]
              if s < n] if kind == "flac" else []
    windows = grid(kind, points)
    got = audiotools.decode_windows_batch([path] * len(windows), [s for s, _ in windows],
                                          [l for _, l in windows])
    try:
        assert got.errors == [None] * len(windows)
        for k, (start, length) in enumerate(windows):
            assert np.array_equal(got.fetch(k), want(x, ch, start, length)), (start, length)
            assert got.rows[k].frames == len(want(x, ch, start, length)) // ch
            assert got.stats[k]["exact"] is EXACT[kind]
            assert (got.sample_rate[k], got.channels[k], got.bits_per_sample[k]) == \
                (rate, ch, bits)
        # one source, one upload: at most the file
        assert 0 < got.uploaded_total <= os.path.getsize(path)
    finally:
        got.close()


def test_images_and_per_row_arguments(sources):
    """byte images as well as filenames; an int start with per-row lengths"""
    kinds = ["flac", "tta", "wav"]
    images = [open(sources[k][0], "rb").read() for k in kinds]
    got = audiotools.decode_windows_batch(images, 100, [5, None, 0])
    try:
        for k, (kind, length) in enumerate(zip(kinds, [5, None, 0])):
            assert np.array_equal(got.fetch(k), want(sources[kind][1], SOURCES[kind][1], 100,
                                                     length))
    finally:
        got.close()


def test_sixty_mixed_rows_share_uploads(sources):
    kinds = ["flac", "m4a", "tta", "wv", "wav", "au", "oga", "shn", "flac6", "aiff"]
    rnd = np.random.default_rng(60)
    rows = [("flac", int(s), 3000) for s in np.linspace(0, 190000, 8)]  # one file, 8 windows
    while len(rows) < 60:
        kind = kinds[len(rows) % len(kinds)]
        n = SOURCES[kind][0]
        rows.append((kind, int(rnd.integers(0, n)), int(rnd.integers(0, n // 2))))
    order = rnd.permutation(60)
    rows = [rows[i] for i in order]
    got = audiotools.decode_windows_batch([sources[k][0] for k, _, _ in rows],
                                          [s for _, s, _ in rows], [l for _, _, l in rows])
    try:
        assert got.errors == [None] * 60
        for k, (kind, start, length) in enumerate(rows):
            assert np.array_equal(got.fetch(k), want(sources[kind][1], SOURCES[kind][1], start,
                                                     length)), (kind, start, length)
        # every source went up once: the union of its rows' bytes, never their sum
        per_row = sum(s["uploaded_bytes"] for s in got.stats)
        files = sum(os.path.getsize(sources[k][0]) for k in set(k for k, _, _ in rows))
        assert got.uploaded_total <= files and got.uploaded_total < per_row
        # the FLAC file's 8 windows lie in 3 seek intervals that overlap: its
        # share of the upload is at most the file, once
        flac_rows = [k for k, r in enumerate(rows) if r[0] == "flac"]
        assert len(flac_rows) >= 8
        assert sum(got.stats[k]["uploaded_bytes"] for k in flac_rows) > \
            os.path.getsize(sources["flac"][0])
    finally:
        got.close()


def damaged_case():
    """a golden case with one bad CRC-16 frame in the middle of a stream that
    walks to its end -> (image, clean image, PCM frames before the bad frame,
    the frames' block sizes, the bad frame's number)"""
    for case in decode_cases.load_cases():
        if case["code"] != 14 or case["cut"] is not None or not case["file"].startswith("tone"):
            continue
        bad = decode_cases.case_bytes(case)
        walk = oracle_port.decode_frames(bad, check_crc=False)
        if walk["code"] not in (0, 16):
            continue
        _, info, _, _ = oracle_port.read_metadata(bad)
        good = case["pcm_bytes"] // (info["channels"] * ((info["bits_per_sample"] + 7) // 8))
        sizes = [b for _, b in walk["offsets"]]
        k = int(np.searchsorted(np.cumsum(sizes), good, side="right"))
        if sum(sizes[:k]) == good and 0 < k < len(sizes) - 1:
            clean = open(os.path.join(decode_cases.FIX, case["file"]), "rb").read()
            return bad, clean, good, sizes, k
    raise AssertionError("no golden case with a bad frame in mid-stream")


def test_unreadable_and_damaged_sources(sources, tmp_path):
    bad, clean, good, sizes, k = damaged_case()
    pcm, ch, bits, _ = oracle_port.decode(clean)
    after = good + sizes[k]
    tone = sources["tta"]
    srcs = [bad, bad, bad, "/nonexistent/window.flac", tone[0], b"junk", bad]
    starts = [0, good - 10, after, 0, 50, 0, 5]
    lengths = [good, 11, 100, 10, 60, 1, None]
    got = audiotools.decode_windows_batch(srcs, starts, lengths)
    try:
        kinds = [type(e).__name__ if e else None for e in got.errors]
        assert kinds == [None, "DecodingError", None, "DecodingError", None, "DecodingError",
                         "DecodingError"]
        assert np.array_equal(got.fetch(0), pcm[:good * ch])          # ends before the frame
        assert np.array_equal(got.fetch(2), pcm[after * ch:(after + 100) * ch])  # starts after
        assert np.array_equal(got.fetch(4), tone[1][50:110])          # untouched either way
        with pytest.raises(audiotools.DecodingError):
            got.fetch(1)
        assert got.rows[1] is None and got.rows[3] is None
    finally:
        got.close()


# ------------------------------------------------------------ the work bound
@pytest.fixture(scope="module")
def minute(tmp_path_factory):
    """60 s of FLAC-8 stereo at 44.1 kHz, block 4096, with from_pcm's
    SEEKTABLE and without"""
    d = tmp_path_factory.mktemp("window_minute")
    n = 44100 * 60
    t = np.arange(n)
    x = np.stack([np.round(9000 * np.sin(t * 0.031)), np.round(7000 * np.sin(t * 0.047))], 1)
    x = x.reshape(-1).astype(np.int32)
    path = str(d / "minute.flac")
    audiotools.FlacAudio.from_pcm(path, audiotools.FrameListReader(x, 44100, 2, 16, 0x3), "8",
                                  total_pcm_frames=n)
    bare = str(d / "minute.bare.flac")
    with open(bare, "wb") as f:
        f.write(rewrite_seektable(open(path, "rb").read(), "none"))
    return path, bare, x


def test_work_bound_flac(minute):
    path, bare, x = minute
    start, length = 44100 * 30, 44100
    data = open(path, "rb").read()
    rc, si, pts = _atgpu.read_metadata(data)
    assert si.max_block_size == 4096 and len(pts) == 6
    # the two seek intervals round the window, and the port lists every frame
    # of them: the stream carries no junk, so the bound below can be relied on
    lo = max(p for p in pts if p[0] <= start)
    hi = min(p for p in pts if p[0] > start + length)
    span = hi[1] - lo[1]
    listed = flac_index_port.index_range(data, si.frames_offset + lo[1], span, si)
    assert [e[1] for e in listed] == list(range(lo[0], hi[0], 4096))
    got = audiotools.decode_windows_batch([path, bare], start, length)
    try:
        assert got.errors == [None, None]
        for k in (0, 1):
            assert np.array_equal(got.fetch(k), x[start * 2:(start + length) * 2])
            assert got.stats[k]["exact"] is True
            assert length <= got.stats[k]["decoded_frames"] <= length + 2 * 4096
        assert got.stats[0]["uploaded_bytes"] == span
        assert got.stats[0]["uploaded_bytes"] < os.path.getsize(path) // 2
        # with no SEEKTABLE the whole frame region goes up
        assert got.stats[1]["uploaded_bytes"] == os.path.getsize(bare) - \
            _atgpu.read_metadata(open(bare, "rb").read())[1].frames_offset
    finally:
        got.close()


def unit_bytes(kind, image, start, length):
    """the bytes of the units that hold [start, start + length), walked from
    the file's own table -> (bytes, the unit's frames)"""
    end = start + length
    if kind == "tta":
        _, info, sizes = _atgpu.tta_read_info(image)
        unit = int(info.block_size)
        return sum(int(sizes[k]) for k in range(len(sizes))
                   if k * unit < end and (k + 1) * unit > start), unit
    if kind == "m4a":
        _, info, _, sizes = _atgpu.alac_read_info(image)
        unit = int(info.max_samples_per_frame)
        return sum(int(sizes[k]) for k in range(len(sizes))
                   if k * unit < end and (k + 1) * unit > start), unit
    _, info, blocks = _atgpu.wv_read_info(image)
    total, unit = 0, 0
    for k in range(info.n_blocks - info.tail_blocks):
        b = blocks[k]
        if b.block_index < end and b.block_index + b.block_samples > start:
            total += 32 + b.size
            unit = max(unit, int(b.block_samples))
    return total, unit


def test_work_bound_other_formats(sources):
    for kind in ("tta", "m4a", "wv"):
        path, x = sources[kind]
        n, ch = SOURCES[kind][:2]
        start, length = n // 2 + 17, 300
        nbytes, unit = unit_bytes(kind, open(path, "rb").read(), start, length)
        assert unit == SOURCES[kind][4] and 0 < nbytes < os.path.getsize(path) // 2, kind
        got = audiotools.decode_windows_batch([path], start, length)
        try:
            assert got.errors == [None] and got.stats[0]["exact"] is True
            assert np.array_equal(got.fetch(0), want(x, ch, start, length))
            assert length <= got.stats[0]["decoded_frames"] <= length + 2 * unit, kind
            # exactly the one or two units round the window
            assert got.stats[0]["uploaded_bytes"] == nbytes, kind
        finally:
            got.close()
    for kind in ("wav", "aiff", "au"):
        path, x = sources[kind]
        n, ch, bits = SOURCES[kind][:3]
        got = audiotools.decode_windows_batch([path], 1000, 700)
        try:
            assert got.stats[0]["decoded_frames"] == 700
            assert got.stats[0]["uploaded_bytes"] == 700 * ch * bits // 8
            assert np.array_equal(got.fetch(0), want(x, ch, 1000, 700))
        finally:
            got.close()
    for kind in ("oga", "shn"):
        got = audiotools.decode_windows_batch([sources[kind][0]], 10, 20)
        try:
            assert got.stats[0]["exact"] is False and got.errors == [None]
        finally:
            got.close()
