"""CPU: windows.plan_window for every kind of source against a brute-force
walk of the same tables, over the grid of starts and lengths round the unit
and seek point edges; placeholder seek points, an empty SEEKTABLE, negative
arguments; and refine_flac over a frame index.  The headers are built by
hand: plan_window reads nothing but the tables."""
import itertools
from types import SimpleNamespace as NS

import numpy as np
import pytest

from audiotools import _atgpu, pcmfiles, windows
from audiotools.batchfiles import _Header

PLACEHOLDER = windows.PLACEHOLDER


def header(kind, total, info, image_bytes, channels=2, bits=16):
    return _Header(kind, 44100, channels, bits, 0x3, total, info, bytes(image_bytes))


def grid(unit, total, points=()):
    starts = {0, 1, unit - 1, unit, unit + 1, total - 1, total, total + 5}
    for p in points:
        starts |= {p - 1, p, p + 1}
    starts = sorted(s for s in starts if s >= 0)
    lengths = [0, 1, unit, None, total + 7]
    return list(itertools.product(starts, lengths))


def clipped(total, start, length):
    if start >= total:
        return 0
    return total - start if length is None else min(length, total - start)


def check_common(p, total, start, length):
    keep = clipped(total, start, length)
    assert p.keep == keep
    if keep == 0:
        assert p.byte_start == p.byte_end and p.lead == 0
    else:
        assert p.first_sample + p.lead == start and p.lead >= 0
        assert p.byte_end > p.byte_start
        # whole units are asked of the decoder, never past the stream's end
        assert p.lead + p.keep <= p.decode <= total - p.first_sample


# --------------------------------------------------------------------- FLAC
BLOCK, NFRAMES = 1152, 40
FRAME_BYTES = [700 + 13 * (k % 7) for k in range(NFRAMES)]
FRAME_AT = np.concatenate([[0], np.cumsum(FRAME_BYTES)]).tolist()
FLAC_TOTAL = BLOCK * (NFRAMES - 1) + 500
F0 = 4242


def flac_header(n_points):
    si = NS(frames_offset=F0, total_samples=FLAC_TOTAL, n_seekpoints=n_points,
            min_block_size=BLOCK, max_block_size=BLOCK, sample_rate=44100, channels=2,
            bits_per_sample=16)
    return header("flac", FLAC_TOTAL, si, F0 + FRAME_AT[-1])


def flac_brute(points, start, keep):
    """the last usable point at or before start, the first past the window's end"""
    usable = [(s, b) for s, b, _ in points if s != PLACEHOLDER]
    s0, b0 = 0, 0
    for s, b in usable:
        if s <= start:
            s0, b0 = s, b
    b1 = FRAME_AT[-1]
    for s, b in usable:
        if s > start + keep:
            b1 = b
            break
    return s0, F0 + b0, F0 + b1


SEEK_FRAMES = [0, 9, 18, 27, 36]
POINTS = [(BLOCK * k, FRAME_AT[k], BLOCK) for k in SEEK_FRAMES]
TABLES = {
    "seektable": POINTS,
    "none": [],
    "placeholders only": [(PLACEHOLDER, 0, 0)] * 3,
    "placeholders between": POINTS[:2] + [(PLACEHOLDER, 0, 0)] + POINTS[2:] +
                            [(PLACEHOLDER, 0, 0)],
}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_flac(name):
    points = TABLES[name]
    h = flac_header(len(points))
    seek = [s for s, _, _ in points if s != PLACEHOLDER]
    for start, length in grid(BLOCK, FLAC_TOTAL, seek):
        p = windows.plan_window(h, start, length, seekpoints=points)
        check_common(p, FLAC_TOTAL, start, length)
        if p.keep:
            s0, b0, b1 = flac_brute(points, start, p.keep)
            assert (p.first_sample, p.byte_start, p.byte_end, p.unit) == (s0, b0, b1, b0)
            assert p.exact
            # up to the sample the end point names, else the stream's end
            ends = [s for s, b, _ in points if s != PLACEHOLDER and F0 + b == b1]
            assert p.first_sample + p.decode == (ends[0] if ends else FLAC_TOTAL)
            # the bytes hold every frame the window touches
            first, last = start // BLOCK, (start + p.keep - 1) // BLOCK
            assert p.byte_start <= F0 + FRAME_AT[first] and F0 + FRAME_AT[last + 1] <= p.byte_end
    if name == "seektable":  # two seek intervals round a window inside one
        p = windows.plan_window(h, BLOCK * 10, BLOCK, seekpoints=points)
        assert (p.byte_start, p.byte_end) == (F0 + FRAME_AT[9], F0 + FRAME_AT[18])


def test_flac_table_that_runs_backwards_is_cut():
    # samples ascend, the third point's byte does not: points 0 and 1 serve
    points = [POINTS[0], POINTS[1], (POINTS[2][0], FRAME_AT[3], BLOCK), POINTS[3]]
    p = windows.plan_window(flac_header(4), BLOCK * 30, 10, seekpoints=points)
    assert p.first_sample == POINTS[1][0] and p.byte_end == F0 + FRAME_AT[-1]
    # listed out of order they are sorted first
    points = [POINTS[0], POINTS[2], POINTS[1], POINTS[3]]
    p = windows.plan_window(flac_header(4), BLOCK * 30, 10, seekpoints=points)
    assert p.first_sample == POINTS[3][0]


def test_refine_flac():
    h = flac_header(len(POINTS))
    start, length = BLOCK * 12 + 7, BLOCK * 2
    plan = windows.plan_window(h, start, length, seekpoints=POINTS)
    base = plan.byte_start - F0
    entries = [(FRAME_AT[k] - base, BLOCK * k, BLOCK) for k in range(9, 18)]
    got = windows.refine_flac(plan, entries)
    assert got.first_sample == BLOCK * 12 and got.lead == 7 and got.keep == length
    assert got.byte_start == got.unit == F0 + FRAME_AT[12]
    assert got.byte_end == F0 + FRAME_AT[15]  # the first frame at or past the end
    assert got.decode == BLOCK * 3            # whole frames 12, 13 and 14
    # nothing listed: the plan stands
    assert windows.refine_flac(plan, []) == plan
    # frame 12 not listed: the frame before it
    got = windows.refine_flac(plan, [e for e in entries if e[1] != BLOCK * 12])
    assert got.first_sample == BLOCK * 11 and got.lead == BLOCK + 7
    assert got.decode == BLOCK * 4
    # headers that all carry one number place nothing past the first
    same = [(FRAME_AT[k] - base, BLOCK * 9, BLOCK) for k in range(9, 18)]
    got = windows.refine_flac(plan, same)
    assert got.first_sample == BLOCK * 9 and got.byte_start == plan.byte_start
    assert got.byte_end == plan.byte_end
    # a window that ends with the stream keeps the range's end
    plan = windows.plan_window(h, FLAC_TOTAL - 10, None, seekpoints=POINTS)
    base = plan.byte_start - F0
    got = windows.refine_flac(plan, [(FRAME_AT[k] - base, BLOCK * k, BLOCK)
                                     for k in range(36, 40)])
    assert got.first_sample == BLOCK * 39 and got.byte_end == F0 + FRAME_AT[-1]
    assert got.decode == 500


# ------------------------------------------------------- True Audio and ALAC
def test_tta():
    block, total = 46080, 46080 * 6 + 1234
    sizes = np.array([5000 + 37 * k for k in range(7)], dtype=np.uint32)
    info = NS(block_size=block, frames_offset=130, total_pcm_frames=total)
    h = header("tta", total, (info, sizes), 130 + int(sizes.sum()))
    at = [130 + int(sizes[:k].sum()) for k in range(8)]
    for start, length in grid(block, total):
        p = windows.plan_window(h, start, length)
        check_common(p, total, start, length)
        if p.keep:
            first, last = start // block, (start + p.keep - 1) // block
            assert (p.unit, p.first_sample) == (first, first * block)
            assert (p.byte_start, p.byte_end) == (at[first], at[last + 1])
            assert p.exact and p.lead < block
            assert p.decode == min((last + 1) * block, total) - first * block


def test_alac():
    per, total = 4096, 4096 * 9 + 77
    sizes = np.array([3000 + 11 * k for k in range(10)], dtype=np.uint32)
    info = NS(max_samples_per_frame=per, mdat_offset=9000, total_frames=total)
    h = header("alac", total, (info, sizes), 9000 + int(sizes.sum()) + 300)
    at = [9000 + int(sizes[:k].sum()) for k in range(11)]
    for start, length in grid(per, total):
        p = windows.plan_window(h, start, length)
        check_common(p, total, start, length)
        if p.keep:
            first, last = start // per, (start + p.keep - 1) // per
            assert (p.unit, p.first_sample) == (first, first * per)
            assert (p.byte_start, p.byte_end) == (at[first], at[last + 1])
            assert p.exact and p.lead < per
    # no stsz sizes: the walk from mdat's start, and the row says so
    h = header("alac", total, (info, sizes[:0]), 50000)
    p = windows.plan_window(h, per * 3 + 1, 10)
    assert (p.exact, p.byte_start, p.byte_end, p.lead, p.keep) == (False, 9000, 50000,
                                                                  per * 3 + 1, 10)


# ------------------------------------------------------------------ WavPack
def test_wavpack():
    per, n_sets, per_set = 22050, 8, 3  # six channels: three stereo blocks a set
    total = per * (n_sets - 1) + 999
    blocks = (_atgpu.WvBlock * (n_sets * per_set + 1))()
    pos = 0
    for s in range(n_sets):
        for c in range(per_set):
            b = blocks[s * per_set + c]
            b.offset, b.size = pos, 2000 + 7 * s + c
            b.block_index = per * s
            b.block_samples = per if s < n_sets - 1 else 999
            b.set, b.first_channel = s, 2 * c
            pos += 32 + b.size
    end_of = [int(blocks[s * per_set + per_set - 1].offset) + 32 +
              int(blocks[s * per_set + per_set - 1].size) for s in range(n_sets)]
    info = NS(n_blocks=n_sets * per_set + 1, tail_blocks=1)
    h = header("wavpack", total, (info, blocks), pos + 100, channels=6)
    for start, length in grid(per, total):
        p = windows.plan_window(h, start, length)
        check_common(p, total, start, length)
        if p.keep:
            first, last = start // per, (start + p.keep - 1) // per
            assert (p.unit, p.first_sample) == (first, first * per)
            assert p.byte_start == int(blocks[first * per_set].offset)
            assert p.byte_end == end_of[last]
            assert p.exact and p.lead < per


# ------------------------------------------------------- WAV, AIFF and Sun AU
@pytest.mark.parametrize("channels,bits", [(1, 8), (2, 16), (6, 24)])
def test_pcm(channels, bits):
    total, per = 5000, channels * (bits // 8)
    info = pcmfiles.PcmImage("wav", channels, bits, 44100, 0, total, 44, total * per, total,
                             False, bits != 8)
    h = header("pcm", total, info, 44 + total * per, channels, bits)
    for start, length in grid(1024, total):
        p = windows.plan_window(h, start, length)
        check_common(p, total, start, length)
        if p.keep:
            assert (p.lead, p.unit, p.first_sample) == (0, start, start)
            assert (p.byte_start, p.byte_end) == (44 + start * per, 44 + (start + p.keep) * per)
    # a data chunk cut short ends the window sooner
    short = info._replace(frames=3000, data_bytes=3000 * per)
    h = header("pcm", total, short, 44 + 3000 * per, channels, bits)
    assert windows.plan_window(h, 2990, 100).keep == 10
    assert windows.plan_window(h, 3000, 100).keep == 0


# ----------------------------------------------------------- no table at all
@pytest.mark.parametrize("kind", ["oggflac", "shn"])
def test_decoded_whole(kind):
    total = 30000
    h = header(kind, total, NS(), 12345)
    for start, length in grid(4096, total):
        p = windows.plan_window(h, start, length)
        check_common(p, total, start, length)
        assert not p.exact
        if p.keep:
            assert (p.byte_start, p.byte_end, p.first_sample, p.lead) == (0, 12345, 0, start)


@pytest.mark.parametrize("start,length", [(-1, 10), (0, -1), (-5, None)])
def test_negative_arguments(start, length):
    for h in (flac_header(0), header("shn", 100, NS(), 10)):
        with pytest.raises(ValueError):
            windows.plan_window(h, start, length, seekpoints=[])
    from audiotools import decode_windows_batch
    with pytest.raises(ValueError):
        decode_windows_batch([b"", b""], start, length)


def test_batch_arguments_need_no_gpu():
    from audiotools import decode_windows_batch
    with pytest.raises(ValueError):
        decode_windows_batch([b"x"], [0, 1])
    got = decode_windows_batch([b"not audio", "/nonexistent/file.flac"], 0)
    assert [type(e).__name__ for e in got.errors] == ["DecodingError"] * 2
    assert got.rows == [None, None]
    got.close()
    assert decode_windows_batch([], 0).rows == []
