"""GPU: the FLAC frame index (csrc/flac_index.hip) against the Python
restatement of its listing rule (flac_index_port), record for record, and
against the reference decoder's walk where the stream is whole: the fixtures,
GPU-encoded streams of 1/2/6 channels and 16/24 bits at three block sizes,
8-bit white noise (VERBATIM frames full of sync patterns), ranges at every
byte phase, ranges cut inside frames, empty and frameless ranges, junk after a
frame, 300 ragged ranges in one call with canaries round the entry rows, and
the too-small-capacity report."""
import ctypes
import os
import random

import numpy as np
import pytest

import flac_index_port as port
import oracle_port
import signals
from test_flac_index_port import FIXTURES, load, walked

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def both(data, ranges):
    """ranges: [(start, nbytes, si)] -> (GPU entries, port entries)"""
    from audiotools import _atgpu
    got = _atgpu.flac_index_host(data, [_atgpu.flac_index_range(a, n, si) for a, n, si in ranges])
    return got, port.index_ranges(data, ranges)


def pack(bodies, gap=0):
    """bodies one after another, `gap` bytes of 0xFF 0xF8 noise between them
    -> (buffer, [start])"""
    buf, starts = bytearray(), []
    for b in bodies:
        starts.append(len(buf))
        buf += b + b"\xff\xf8\xc9\x18"[:gap]
    return bytes(buf), starts


def whole(name):
    data = load(name)
    si, want = walked(data)
    return data[si.frames_offset:], si, want


def encode(kind, n, channels, bps, block_size, seed=1, rate=44100):
    """one GPU-encoded .flac image (FLAC-8 at `block_size`)"""
    from audiotools import _atgpu
    pcm = signals.make(kind, n, channels, bps, seed=seed)
    opts = dict(oracle_port.PRESETS["8"], block_size=block_size)
    out, res, _, _ = _atgpu.engine().encode(
        _atgpu.make_options(**opts), pcm.astype(np.int16 if bps == 16 else np.int32), [(0, n)],
        channels, bps, rate)
    assert res[0].status == 0
    return out[res[0].out_offset:res[0].out_offset + res[0].bytes].tobytes()


def test_fixtures_in_one_call():
    from audiotools import _atgpu
    streams = [whole(name) for name in FIXTURES]
    data, starts = pack([b for b, _, _ in streams])
    ranges = [(a, len(b), si) for a, (b, si, _) in zip(starts, streams)]
    got, want = both(data, ranges)
    assert got == want
    for r, (name, (_, _, frames)) in enumerate(zip(FIXTURES, streams)):
        mine = [e[1:] for e in got if e[0] == r]
        if name.endswith("flac-allframes.flac"):  # every header numbered 0
            frames = [(off, 0, bs) for off, _, bs in frames]
        assert mine == frames, name
    assert sorted(_atgpu.flac_index_kernel_times()) == ["confirm", "header", "sync"]


def test_public_entry_on_whole_images():
    from audiotools import decoders
    names = ["fixtures/tone2.flac", "fixtures/1h.flac", "fixtures/flac-seektable.flac"]
    got = decoders.flac_frame_index_batch([load(n) for n in names])
    assert got == [walked(load(n))[1] for n in names]
    assert len(got[1]) == 879


@pytest.mark.parametrize("block_size", [576, 1152, 4096])
def test_gpu_encoded_streams(block_size):
    images = [encode("tone", block_size * 11 + 123, ch, bps, block_size, seed=ch + bps)
              for ch in (1, 2, 6) for bps in (16, 24)]
    streams = []
    for img in images:
        si, want = walked(img)
        assert len(want) == 12 and si.max_block_size == block_size
        streams.append((img[si.frames_offset:], si, want))
    data, starts = pack([b for b, _, _ in streams], gap=3)
    got, want = both(data, [(a, len(b), si) for a, (b, si, _) in zip(starts, streams)])
    assert got == want
    for r, (_, _, frames) in enumerate(streams):
        assert [e[1:] for e in got if e[0] == r] == frames


def test_white_noise_8_bit():
    """VERBATIM frames of noise hold sync patterns of their own: every entry
    is a frame start of the reference's walk, and every frame is an entry"""
    found = 0
    for channels in (1, 2):
        img = encode("noise", 4096 * 39 + 5, channels, 8, 4096, seed=40 + channels)
        si, frames = walked(img)
        body = img[si.frames_offset:]
        a = np.frombuffer(body, np.uint8)
        found += int(np.count_nonzero((a[:-1] == 0xFF) & ((a[1:] & 0xFE) == 0xF8))) - len(frames)
        got, want = both(body, [(0, len(body), si)])
        assert got == want
        assert [e[1:] for e in got] == frames
    assert found > 0  # there were false patterns to refuse


def test_every_byte_phase():
    body, si, frames = whole("fixtures/tone2.flac")
    buf, ranges = bytearray(), []
    for phase in range(16):
        buf += bytes((-len(buf)) % 64 + phase)
        ranges.append((len(buf), len(body), si))
        buf += body
    got, want = both(bytes(buf), ranges)
    assert got == want
    for phase in range(16):
        assert [e[1:] for e in got if e[0] == phase] == frames


def test_device_entry_off_16_byte_alignment():
    """the device entry promises 4-byte alignment only"""
    import torch
    from audiotools import _atgpu
    body, si, frames = whole("fixtures/tone3.flac")
    for shift in (0, 4, 8, 12):
        raw = bytes(shift) + body + bytes((-len(body)) % 4)
        t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
        assert t.data_ptr() % 16 == 0
        got = _atgpu.flac_index_device(t.data_ptr() + shift, len(body),
                                       [_atgpu.flac_index_range(0, len(body), si)])
        torch.cuda.synchronize()
        assert [e[1:] for e in got] == frames


def test_ranges_cut_inside_frames():
    body, si, frames = whole("fixtures/tone2.flac")
    a, b = frames[3][0], frames[9][0]
    ranges = [(a - 5, (b + 7) - (a - 5), si), (a, b - a, si), (a + 1, frames[4][0] - a - 1, si),
              (a + 1, len(body) - a - 1, si), (0, b - 1, si)]
    got, want = both(body, ranges)
    assert got == want
    assert [e[1:] for e in got if e[0] == 0] == [(o - (a - 5), s, n) for o, s, n in frames[3:9]]
    assert [e[1:] for e in got if e[0] == 1] == [(o - a, s, n) for o, s, n in frames[3:9]]
    assert [e for e in got if e[0] == 2] == []
    assert [e[1:] for e in got if e[0] == 3] == [(o - a - 1, s, n) for o, s, n in frames[4:]]
    assert [e[1:] for e in got if e[0] == 4] == frames[:8]


def test_empty_and_frameless_ranges():
    body, si, frames = whole("fixtures/tone1.flac")
    junk = np.random.default_rng(3).integers(0, 256, 70000).astype(np.uint8).tobytes()
    data = body + junk + bytes(5000)
    ranges = [(0, 0, si), (len(body), len(junk), si), (len(body) + len(junk), 5000, si),
              (7, 8, si), (len(data), 0, si), (0, len(body), si)]
    got, want = both(data, ranges)
    assert got == want
    assert [e[1:] for e in got] == frames and {e[0] for e in got} == {5}


def test_junk_after_the_first_frame():
    body, si, frames = whole("fixtures/tone2.flac")
    cut = frames[1][0]
    for junk, first in ((b"\0\0", frames[:1]), (b"\x5a\xa5", [])):
        bent = body[:cut] + junk + body[cut:]
        got, want = both(bent, [(0, len(bent), si)])
        assert got == want
        assert [e[1:] for e in got] == first + [(o + 2, s, n) for o, s, n in frames[1:]]


def raw_call(data, ranges, cap, pad=8):
    """atg_flac_index_host into `cap` entry rows with `pad` canary rows on
    either side -> (status, count, the whole array as bytes)"""
    from audiotools import _atgpu
    lib = _atgpu.load_library()
    arr = (_atgpu.FlacIndexRange * len(ranges))(
        *[_atgpu.flac_index_range(a, n, si) for a, n, si in ranges])
    rows = np.full((cap + 2 * pad) * 24, 0xA5, dtype=np.uint8)
    count = ctypes.c_uint64()
    ents = ctypes.cast(rows.ctypes.data + pad * 24, ctypes.POINTER(_atgpu.FlacIndexEntry))
    st = lib.atg_flac_index_host(_atgpu.default_device(), data, len(data), arr, len(ranges), ents,
                                 cap, ctypes.byref(count))
    return st, count.value, rows


def ragged_300():
    """300 ranges over four small streams packed with junk between them, every
    third one the whole of 1h.flac (879 frames of about 15 bytes)"""
    streams = [whole(n) for n in ("fixtures/1h.flac", "fixtures/tone2.flac", "fixtures/1m.flac",
                                  "fixtures/flac-seektable.flac")]
    data, starts = pack([b for b, _, _ in streams], gap=2)
    rnd = random.Random(300)
    ranges = []
    for k in range(300):
        s = 0 if k % 3 == 0 else 1 + (k // 3) % 3
        body, si, _ = streams[s]
        a, n = 0, len(body)
        if s:
            a = rnd.randrange(0, len(body))
            n = rnd.randrange(0, min(len(body) - a, 3000) + 1)
        ranges.append((starts[s] + a, n, si))
    return data, starts, ranges, port.index_ranges(data, ranges)


def test_300_ragged_ranges_and_canaries():
    from audiotools import _atgpu
    data, starts, ranges, want = ragged_300()
    # more starts than the lists' first capacity holds: the call runs twice
    assert len(want) > 4096 + sum(n for _, n, _ in ranges) // 64
    cap, pad = len(want) + 50, 8
    st, count, rows = raw_call(data, ranges, cap, pad)
    assert st == _atgpu.ATG_OK, _atgpu.load_library().atg_flac_index_last_error()
    assert count == len(want)
    got = np.frombuffer(rows[pad * 24:(pad + count) * 24].tobytes(),
                        dtype=_atgpu.FLAC_INDEX_ENTRY_DTYPE)
    assert [(int(r), int(o), int(s), int(b)) for o, s, b, r in got.tolist()] == want
    assert (rows[:pad * 24] == 0xA5).all()             # before the rows
    assert (rows[(pad + count) * 24:] == 0xA5).all()   # the unused rows and after
    st2, count2, rows2 = raw_call(data, ranges, cap, pad)
    assert st2 == st and count2 == count and np.array_equal(rows2, rows)


def test_too_small_capacity_is_reported():
    from audiotools import _atgpu
    body, si, frames = whole("fixtures/tone2.flac")
    for cap in (0, 1, len(frames) - 1):
        st, count, rows = raw_call(body, [(0, len(body), si)], cap)
        assert st == _atgpu.ATG_ERR_CAPACITY and count == len(frames)
        assert (rows == 0xA5).all()  # nothing written
        assert str(len(frames)).encode() in _atgpu.load_library().atg_flac_index_last_error()
    st, count, _ = raw_call(body, [(0, len(body), si)], len(frames))
    assert st == _atgpu.ATG_OK and count == len(frames)
    # the Python wrapper answers the report with one more call
    got = _atgpu.flac_index_host(body, [_atgpu.flac_index_range(0, len(body), si)], cap=1)
    assert [e[1:] for e in got] == frames
