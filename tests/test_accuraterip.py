"""CPU: the AccurateRip port (tests/accuraterip_port.py) against the
reference's known answers, the Python layer's contract (ChecksumV1 /
ChecksumV2 errors, DiscID, parse_response, match) and every argument check of
atg_accuraterip_device / _host, which run before any GPU call."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

import accuraterip_port as port
import bad_device
import oracle_port
from audiotools import _accuraterip, _atgpu, accuraterip, pcm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
VECTORS = json.load(open(os.path.join(GOLDEN, "accuraterip_vectors.json")))


@pytest.fixture(scope="module")
def tone():
    data = open(os.path.join(GOLDEN, VECTORS["fixture"]), "rb").read()
    samples, ch, bps, rate = oracle_port.decode(data)
    assert (ch, bps) == (2, 16)
    return samples, rate


@pytest.mark.parametrize("vec", VECTORS["vectors"],
                         ids=lambda v: "first%d-last%d" % (v["is_first"], v["is_last"]))
def test_port_reproduces_reference_values(tone, vec):
    samples, rate = tone
    v1, v2 = port.checksums(samples, vec["is_first"], vec["is_last"], rate)
    assert ("%08X" % v1, "%08X" % v2) == (vec["v1"], vec["v2"])


def _image(lengths, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-32768, 32768, size=2 * sum(lengths)).astype(np.int32)


def test_port_sweep_is_the_shifted_window():
    """3-track image, K = 7: offset 0 is the plain checksum, offset k the
    plain checksum of the window k frames on (silence outside the image)"""
    lengths, rate, K = [700, 1211, 650], 8000, 7  # skip: 530 frames
    img = _image(lengths, 3)
    total, start = sum(lengths), 0
    for t, n in enumerate(lengths):
        first, last = t == 0, t == len(lengths) - 1
        table = port.sweep(img, start, n, 0, total, first, last, rate, K)
        assert len(table) == 2 * K + 1
        for k in range(-K, K + 1):
            shifted = port.window(img, start + k, n, 0, total)
            assert table[k + K] == port.checksums(shifted, first, last, rate)[0], (t, k)
        assert table[K] == port.checksums(img[2 * start:2 * (start + n)], first, last, rate)[0]
        start += n
    # the first track at a negative offset begins in the silence before the image
    assert port.window(img, -3, 5, 0, total)[:6].tolist() == [0] * 6


def test_port_end_offset_wraps():
    """total = 100 on a last track: 100 - 2940 wraps to a huge end, so
    nothing is cut -- the same sum as a middle track"""
    x = _image([100], 5)
    assert port.offsets(False, True, 44100, 100) == (0, (100 - 2940) & 0xFFFFFFFF)
    assert port.checksums(x, False, True, 44100) == port.checksums(x, False, False, 44100)
    assert port.checksums(x, False, True, 44100)[0] != 0


def test_port_empty_range():
    """total = 4000, first and last: start 2940 > end 1060, the sum is 0"""
    x = _image([4000], 6)
    assert port.offsets(True, True, 44100, 4000) == (2940, 1060)
    assert port.checksums(x, True, True, 44100) == (0, 0)


@pytest.mark.parametrize("cls", [_accuraterip.ChecksumV1, _accuraterip.ChecksumV2])
def test_checksum_class_errors(cls):
    with pytest.raises(ValueError, match="^sample rate must be > 0$"):
        cls(False, False, 0, 100)
    with pytest.raises(ValueError, match="^sample rate must be > 0$"):
        cls(False, False, -1, 100)
    with pytest.raises(ValueError, match="^total PCM frames must be > 0$"):
        cls(False, False, 44100, 0)
    with pytest.raises(TypeError):
        cls(False, False, "44100", 100)
    c = cls(True, True, 44100, 100)
    with pytest.raises(TypeError, match="^objects must be of type FrameList$"):
        c.update(b"\0\0\0\0")
    with pytest.raises(ValueError, match="^FrameList must be 2 channels$"):
        c.update(pcm.FrameList(b"\0" * 4, 1, 16, False, True))
    with pytest.raises(ValueError, match="^FrameList must be 16 bits per sample$"):
        c.update(pcm.FrameList(b"\0" * 6, 2, 24, False, True))
    # nothing fed, nothing to sum: no GPU is needed for the answer
    assert c.checksum() == 0


def test_disc_id():
    # a hand-made table of contents: 3 tracks at CD frames 0, 15000, 33000,
    # lead-out at 50000
    d = accuraterip.DiscID([1, 2, 3], [0, 15000, 33000], 50000, 0x1A02B703)
    assert d.track_numbers() == [1, 2, 3]
    assert d.id1() == 0 + 15000 + 33000 + 50000
    # track 1's offset 0 counts as 1
    assert d.id2() == 1 * 1 + 2 * 15000 + 3 * 33000 + 4 * 50000
    assert d.freedb_disc_id() == 0x1A02B703
    # 98000 = 0x17ed0, 329001 = 0x50529
    assert str(d) == "dBAR-003-00017ed0-00050529-1a02b703.bin"
    assert repr(d) == "AccurateRipDiscID([1, 2, 3], [0, 15000, 33000], 50000, 436385539)"
    assert accuraterip.DiscID([1], [0], 10, "77").freedb_disc_id() == 77


def _chunk(disc_id, entries, ids=None):
    id1, id2, fdb = ids or (disc_id.id1(), disc_id.id2(), disc_id.freedb_disc_id())
    out = struct.pack("<BIII", len(entries), id1, id2, fdb)
    for e in entries:
        out += struct.pack("<BII", *e)
    return out


def test_parse_response():
    d = accuraterip.DiscID([1, 2, 3], [0, 15000, 33000], 50000, 0x1A02B703)
    a = [(7, 0x11111111, 0xA1), (8, 0x22222222, 0xA2), (9, 0x33333333, 0xA3)]
    b = [(1, 0x44444444, 0xB1), (2, 0x55555555, 0xB2), (3, 0x66666666, 0xB3)]
    # two matching chunks: entries appended per track, in order
    assert accuraterip.parse_response(_chunk(d, a) + _chunk(d, b), d) == {
        1: [a[0], b[0]], 2: [a[1], b[1]], 3: [a[2], b[2]]}
    # an empty body
    assert accuraterip.parse_response(b"", d) == {1: [], 2: [], 3: []}
    # the last entry cut short: dropped, the rest kept
    assert accuraterip.parse_response((_chunk(d, a) + _chunk(d, b))[:-1], d) == {
        1: [a[0], b[0]], 2: [a[1], b[1]], 3: [a[2]]}
    # a chunk with other ids: its 27 entry bytes are not skipped -- 13 of
    # them are read as a header, then 13 more, and the last byte with the
    # next 12 -- so the matching chunk behind it is never seen as one
    other = _chunk(d, a, ids=(1, 2, 3))
    assert accuraterip.parse_response(other + _chunk(d, b), d) == {1: [], 2: [], 3: []}
    # with 26 entry bytes (two headers' worth) the next chunk is found again
    pad = struct.pack("<BIII", 0, 9, 9, 9)
    assert accuraterip.parse_response(
        struct.pack("<BIII", 3, 1, 2, 3) + pad + pad + _chunk(d, b), d) == {
        1: [b[0]], 2: [b[1]], 3: [b[2]]}
    # a track number the disc does not list leaves its entry unread
    d2 = accuraterip.DiscID([2], [0], 50000, 5)
    assert accuraterip.parse_response(_chunk(d2, [(1, 2, 3), (4, 5, 6)]), d2) == {
        2: [(1, 2, 3)]}


def test_match():
    entries = [(4, 0xAAAA0001, 0), (200, 0xBBBB0002, 0)]
    assert accuraterip.match(0xBBBB0002, entries) == 200
    assert accuraterip.match(0xCCCC0003, entries) == accuraterip.AR_MISMATCH == -2
    assert accuraterip.match(0xCCCC0003, []) == accuraterip.AR_NOT_FOUND == -1


# ---- the library's argument checks (no GPU call is reached) ----------------
def _device_call(tracks, max_offset=0, fmt=_atgpu.PCM_S32, null=(), n=None):
    lib = _atgpu.load_library()
    n = len(tracks) if n is None else n
    arr = (_atgpu.ArTrack * max(1, len(tracks)))(*tracks)
    res = (_atgpu.ArResult * max(1, len(tracks)))()
    table = np.zeros(max(1, len(tracks)) * (2 * min(max_offset, 65535) + 1), dtype=np.uint32)
    buf = np.zeros(64, dtype=np.int32)
    return lib.atg_accuraterip_device(
        None if "pcm" in null else buf.ctypes.data_as(ctypes.c_void_p), fmt,
        None if "tracks" in null else arr, n, max_offset,
        None if "results" in null else res,
        None if "table" in null else table.ctypes.data_as(ctypes.c_void_p), None)


def _host_call(tracks, max_offset=0, frames_total=32, null=(), device=0):
    lib = _atgpu.load_library()
    arr = (_atgpu.ArTrack * max(1, len(tracks)))(*tracks)
    res = (_atgpu.ArResult * max(1, len(tracks)))()
    table = np.zeros(max(1, len(tracks)) * (2 * min(max_offset, 65535) + 1), dtype=np.uint32)
    buf = np.zeros(64, dtype=np.int32)
    return lib.atg_accuraterip_host(
        device, None if "pcm" in null else buf.ctypes.data_as(ctypes.c_void_p), _atgpu.PCM_S32,
        frames_total, None if "tracks" in null else arr, len(tracks), max_offset,
        None if "results" in null else res,
        None if "table" in null else table.ctypes.data_as(ctypes.c_void_p))


def _t(**kw):
    d = dict(pcm_offset=0, pcm_frames=16, sample_rate=44100)
    d.update(kw)
    return _atgpu.ar_track(**d)


BAD_TRACKS = {
    "sample_rate_0": lambda: _t(sample_rate=0),
    "pcm_frames_0": lambda: _atgpu.ArTrack(0, 0, 0, 16, 0, 16, 44100, 0),
    "total_pcm_frames_0": lambda: _atgpu.ArTrack(0, 16, 0, 16, 0, 0, 44100, 0),
    "lo_above_hi": lambda: _t(lo_frame=9, hi_frame=8),
    "index_reaches_2^32": lambda: _t(index0=0xFFFFFFF0, total_pcm_frames=16),
    "pcm_frames_2^32": lambda: _atgpu.ArTrack(0, 1 << 32, 0, 16, 0, 16, 44100, 0),
}


@pytest.mark.parametrize("call", [_device_call, _host_call], ids=["device", "host"])
@pytest.mark.parametrize("name", sorted(BAD_TRACKS))
def test_invalid_tracks_refused(call, name):
    assert call([_t(), BAD_TRACKS[name]()]) == _atgpu.ATG_ERR_INVALID
    assert _atgpu.load_library().atg_accuraterip_last_error()


@pytest.mark.parametrize("call", [_device_call, _host_call], ids=["device", "host"])
def test_null_arrays_refused(call):
    for null in (("pcm",), ("tracks",), ("results",)):
        assert call([_t()], null=null) == _atgpu.ATG_ERR_INVALID, null
    # the offset table may be NULL only when max_offset is 0
    assert call([_t()], max_offset=3, null=("table",)) == _atgpu.ATG_ERR_INVALID


def test_index_just_below_2_32_passes_the_check():
    """index0 + pcm_frames = 2^32 - 1 is allowed: what stops the call is the
    next check (the buffer), not the index"""
    ok = _t(index0=0xFFFFFFFF - 16, total_pcm_frames=16)
    assert _host_call([ok], frames_total=8) == _atgpu.ATG_ERR_INVALID
    assert b"hi_frame" in _atgpu.load_library().atg_accuraterip_last_error()


@pytest.mark.parametrize("call", [_device_call, _host_call], ids=["device", "host"])
def test_max_offset_limit(call):
    assert call([_t()], max_offset=65536) == _atgpu.ATG_ERR_UNSUPPORTED
    assert call([_t()], max_offset=1 << 31) == _atgpu.ATG_ERR_UNSUPPORTED


def test_unknown_format_and_empty_batch():
    assert _device_call([_t()], fmt=7) == _atgpu.ATG_ERR_INVALID
    # no tracks: nothing to do, NULL arrays allowed, no GPU needed
    assert _device_call([], null=("pcm", "tracks", "results", "table")) == _atgpu.ATG_OK
    assert _host_call([], null=("pcm", "tracks", "results", "table")) == _atgpu.ATG_OK


def test_host_region_must_lie_in_the_buffer():
    assert _host_call([_t(hi_frame=33)], frames_total=32) == _atgpu.ATG_ERR_INVALID


def test_host_entry_refuses_device_minus_1():
    bad_device.check_refused(_host_call([_t()], device=-1), "accuraterip")
    bad_device.check_refused(_host_call([_t()], max_offset=3, device=-1), "accuraterip")


def test_binding_raises_with_the_message():
    with pytest.raises(_atgpu.ATGError) as e:
        accuraterip.checksum_batch(np.zeros(64, dtype=np.int16), [_t(sample_rate=0)])
    assert e.value.status == _atgpu.ATG_ERR_INVALID
    assert "sample rate" in str(e.value)
    assert _atgpu.accuraterip_tile_frames() % 1024 == 0
