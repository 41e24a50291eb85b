"""GPU parity: libatgpu's True Audio decoder (tta_decode.hip) against the
reference decoder's recorded output (tests/golden/tta_vectors.json: md5 and
length of the PCM oracle/_ref/ttadec wrote) and, on damaged streams, against
tests/tta_port.py, which restates TTADecoder_read's order: the frame's bytes,
its CRC, then the Rice walk.  The TTADecoder interface."""
import functools
import hashlib
import io
import json
import os
import struct
import zlib

import numpy as np
import pytest

import signals
import tta_cases
import tta_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "tta_vectors.json")))
B = tta_cases.BLOCK


def fixture(name):
    with open(os.path.join(HERE, "golden", "fixtures", name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def vector_images():
    """the decoder vectors' files, encoded on the GPU and held to the
    recorded sha256 of the reference's files"""
    from audiotools import _atgpu
    cases = {c[0]: c for c in tta_cases.encoder_cases()}
    out = {}
    for name in tta_cases.DECODER_CASES:
        _, ch, bps, rate, x = cases[name]
        pcm = x.astype(np.int16 if bps <= 16 else np.int32)
        buf, (r,), sizes = _atgpu.tta_encoder().encode(pcm, [(0, len(x) // ch)], ch, bps, rate)
        img = tta_port.header(ch, bps, rate, len(x) // ch) + \
            tta_port.seektable([int(v) for v in sizes]) + \
            buf[r.out_offset:r.out_offset + r.bytes].tobytes()
        assert hashlib.sha256(img).hexdigest() == G["encoder"][name]["sha256"], name
        out[name] = img
    return out, cases


def test_decoder_vectors_and_fixtures():
    """mixed formats in one batch: the recorded md5 and length of every
    vector, and the source samples where they are known"""
    from audiotools import decoders
    images, cases = vector_images()
    names = list(tta_cases.DECODER_CASES) + list(tta_cases.FIXTURES)
    data = [images[n] if n in images else fixture(n) for n in names]
    for name, (status, info, pcm, bad) in zip(names, decoders.decode_tta_batch(data)):
        v = G["decoder"][name]
        assert status == 0 and bad is None, name
        raw = tta_cases.pcm_bytes(pcm, info.bits_per_sample)
        assert len(raw) == v["bytes"], name
        assert hashlib.md5(raw).hexdigest() == v["md5"], name
        if name in cases:
            assert np.array_equal(pcm, cases[name][4]), name


def test_long_unary_run():
    """the 24-bit quiet-then-full-scale image (runs of millions of one bits)
    decodes to its source"""
    from audiotools import decoders
    images, cases = vector_images()
    name = "quiet_loud_c2_b24"
    assert len(images[name]) > 5000000
    (status, info, pcm, bad), = decoders.decode_tta_batch([images[name]])
    assert status == 0 and np.array_equal(pcm, cases[name][4])


# ---------------------------------------------------------------- damage
@functools.lru_cache(maxsize=None)
def clean():
    """a four-frame mono file and a two-frame stereo file"""
    a = signals.make("tone", 3 * B + 500, 1, 16, seed=21)
    b = signals.make("tone", B + 90, 2, 24, seed=22)
    (ia, _), (ib, _) = tta_port.encode_many([(a, 1, 16, tta_cases.RATE),
                                             (b, 2, 24, tta_cases.RATE)])
    return (ia, a), (ib, b)


def frames_region(img):
    st, _, info, sizes = tta_port.read_info(img)
    assert st == 0
    return info["frames_offset"], sizes


def flip(img, bit):
    b = bytearray(img)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def refresh_crc(img, byte):
    """recompute the CRC of the frame holding `byte`"""
    pos, sizes = frames_region(img)
    for s in sizes:
        if pos <= byte < pos + s:
            crc = struct.pack("<I", zlib.crc32(img[pos:pos + s - 4]) & 0xFFFFFFFF)
            return img[:pos + s - 4] + crc + img[pos + s:]
        pos += s
    raise AssertionError("byte outside the frames")


def damaged():
    """[(name, image)]: 8 payload flips, 4 truncations, 4 payload flips with
    the frame CRC recomputed, over both files"""
    rng = np.random.default_rng(77)
    out = []
    files = [c[0] for c in clean()]
    for k in range(8):
        img = files[k % 2]
        lo, _ = frames_region(img)
        bit = int(rng.integers(lo * 8, len(img) * 8))
        out.append(("flip%d@%d" % (k, bit), flip(img, bit)))
    for k in range(4):
        img = files[k % 2]
        lo, sizes = frames_region(img)
        cut = [lo + 1, int(rng.integers(lo, len(img))), len(img) - 1, lo + sizes[0]][k]
        out.append(("cut%d@%d" % (k, cut), img[:cut]))
    for k in range(4):
        img = files[k % 2]
        lo, sizes = frames_region(img)
        # inside a payload, not in a CRC: early in a frame, so that the
        # walk goes on over damaged data for most of it
        frame = k % len(sizes)
        start = lo + sum(sizes[:frame])
        byte = start + int(rng.integers(0, max(1, (sizes[frame] - 4) // 4)))
        bad = flip(img, byte * 8 + int(rng.integers(0, 8)))
        out.append(("reflip%d@%d" % (k, byte), refresh_crc(bad, byte)))
    return out


def test_damaged_streams_match_port():
    """status for status, bad frame for bad frame, sample for sample; the
    frames before the bad one decode exactly, and so do the clean tracks that
    share the batch"""
    from audiotools import decoders
    (ia, a), (ib, b) = clean()
    cases = damaged()
    names = ["clean_a"] + [c[0] for c in cases] + ["clean_b"]
    data = [ia] + [c[1] for c in cases] + [ib]
    want = tta_port.decode_many(data)
    got = decoders.decode_tta_batch(data)
    seen = set()
    for name, w, g in zip(names, want, got):
        wst, _, wbad, wpcm, _ = w
        gst, info, gpcm, gbad = g
        print(name, "port", wst, wbad, len(wpcm), "gpu", gst, gbad, len(gpcm))
        assert gst == wst, name
        assert gbad == wbad, name
        assert np.array_equal(gpcm, wpcm), name
        src = a if info.channels == 1 else b
        if name.startswith(("flip", "cut")):
            # plain damage never gets past the CRC: what is decoded is the source
            assert np.array_equal(gpcm, src[:len(gpcm)]), name
        seen.add(wst)
    assert np.array_equal(got[0][2], a) and np.array_equal(got[-1][2], b)
    # the set exercises the CRC check, the missing bytes and the walk itself
    assert tta_port.CRC_MISMATCH in seen and tta_port.IO_ERROR in seen


def test_parse_runs_out_of_bits():
    """a frame cut short under a valid CRC and a matching seektable: the walk
    ends inside the frame with "I/O error during frame read", the frames
    before it and the track after it are exact"""
    from audiotools import decoders
    (ia, a), (ib, b) = clean()
    lo, sizes = frames_region(ia)
    # halve the payload of frame 1
    start = lo + sizes[0]
    keep = (sizes[1] - 4) // 2
    payload = ia[start:start + keep]
    frame = payload + struct.pack("<I", zlib.crc32(payload) & 0xFFFFFFFF)
    new_sizes = [sizes[0], len(frame)] + sizes[2:]
    img = tta_port.header(1, 16, tta_cases.RATE, len(a)) + tta_port.seektable(new_sizes) + \
        ia[lo:start] + frame + ia[start + sizes[1]:]
    want = tta_port.decode(img)
    assert want[0] == tta_port.FRAME_READ and want[2] == 1
    got = decoders.decode_tta_batch([img, ib])
    assert got[0][0] == 5 and got[0][3] == 1
    assert np.array_equal(got[0][2], a[:B]) and np.array_equal(got[0][2], want[3])
    assert got[1][0] == 0 and np.array_equal(got[1][2], b)
    with pytest.raises(ValueError, match="I/O error during frame read"):
        d = decoders.TTADecoder(img)
        d.read(1)
        d.read(1)


HEADER_DAMAGE = [
    ("signature", lambda d: flip(d, 1 * 8 + 2), ValueError, "invalid header signature"),
    ("format", lambda d: flip(d, 4 * 8), ValueError, "unsupported TTA format"),
    ("sample rate", lambda d: flip(d, 10 * 8 + 3), ValueError, "CRC error reading header"),
    ("seektable", lambda d: flip(d, 24 * 8 + 1), ValueError, "CRC error reading seektable"),
    ("short header", lambda d: d[:20], IOError, "I/O error reading header"),
]


@pytest.mark.parametrize("name,damage,exc,msg", HEADER_DAMAGE, ids=[h[0] for h in HEADER_DAMAGE])
def test_header_and_seektable_damage(name, damage, exc, msg):
    from audiotools import _atgpu, decoders
    img = damage(clean()[0][0])
    st, info, _ = _atgpu.tta_read_info(img)
    assert (st, info.stage) == tta_port.read_info(img)[:2]
    assert tta_port.decode(img)[0] == st != 0
    with pytest.raises(exc, match=msg):
        decoders.TTADecoder(io.BytesIO(img))
    with pytest.raises(exc, match=msg):
        decoders.decode_tta_batch([clean()[1][0], img])


def test_frame_errors_raised_by_read():
    from audiotools import decoders
    (ia, a), _ = clean()
    lo, sizes = frames_region(ia)
    d = decoders.TTADecoder(flip(ia, (lo + sizes[0] + 10) * 8))   # frame 1
    assert np.array_equal(d.read(4096).samples, a[:B])
    with pytest.raises(ValueError, match="CRC mismatch reading frame"):
        d.read(4096)
    d = decoders.TTADecoder(ia[:lo + sizes[0] + sizes[1] - 1])    # frame 1 cut
    assert d.read(4096).frames == B
    with pytest.raises(IOError, match="I/O error reading frame"):
        d.read(4096)


# ------------------------------------------------------------ TTADecoder
def test_decoder_read_seek_close():
    from audiotools import decoders
    (ia, a), _ = clean()
    d = decoders.TTADecoder(io.BytesIO(ia))
    assert (d.sample_rate, d.channels, d.bits_per_sample, d.channel_mask) == \
        (tta_cases.RATE, 1, 16, 0x4)
    got = []
    while True:
        fl = d.read(1)  # one TTA frame per call, whatever is asked for
        if fl.frames == 0:
            break
        got.append(fl)
    assert [f.frames for f in got] == [B, B, B, 500]
    assert np.array_equal(np.concatenate([f.samples for f in got]), a)
    assert d.read(4096).frames == 0
    # the reference's loop: skip a frame while current + block < offset
    assert d.seek(0) == 0
    assert np.array_equal(d.read(1).samples, a[:B])
    assert d.seek(2 * B + 5) == 2 * B
    assert np.array_equal(d.read(1).samples, a[2 * B:3 * B])
    assert d.read(1).frames == 500 and d.read(1).frames == 0
    assert d.seek(2 * B) == B            # on a boundary: one frame early
    assert np.array_equal(d.read(1).samples, a[B:2 * B])
    assert d.seek(10 ** 9) == 3 * B + 500  # past the end: nothing left
    assert d.read(1).frames == 0
    assert d.seek(1) == 0
    with pytest.raises(ValueError, match="cannot seek to negative value"):
        d.seek(-1)
    d.close()
    with pytest.raises(ValueError, match="cannot read closed stream"):
        d.read(1)
    with pytest.raises(ValueError, match="cannot seek closed stream"):
        d.seek(0)


def test_channel_masks():
    from audiotools import decoders
    _, (ib, _) = clean()
    assert decoders.TTADecoder(ib).channel_mask == 0x3
    x = signals.make("tone", 50, 3, 16)
    assert decoders.TTADecoder(tta_port.encode(x, 3, 16, tta_cases.RATE)[0]).channel_mask == 0


def test_more_channels_than_registers_hold():
    """9 and 12 channels (the decoder keeps the Rice states of more than 8
    channels in device memory), beside a stereo track in the same batch:
    encoded on the GPU to tta_port's bytes, decoded to the source"""
    from audiotools import _atgpu, decoders
    (_, _), (ib, b) = clean()
    data, srcs = [], []
    for ch, bps, n in ((9, 16, 700), (12, 24, 300)):
        x = signals.make("noise" if ch == 12 else "tone", n, ch, bps, seed=ch)
        img = tta_port.encode(x, ch, bps, tta_cases.RATE)[0]
        pcm = x.astype(np.int16 if bps <= 16 else np.int32)
        buf, (r,), sizes = _atgpu.tta_encoder().encode(pcm, [(0, n)], ch, bps, tta_cases.RATE)
        lo, _ = frames_region(img)
        assert buf[r.out_offset:r.out_offset + r.bytes].tobytes() == img[lo:]
        data.append(img)
        srcs.append(x)
    want = tta_port.decode_many(data)
    got = decoders.decode_tta_batch([data[0], ib, data[1]])
    for g, w, x in zip((got[0], got[2]), want, srcs):
        assert g[0] == 0 and w[0] == 0
        assert np.array_equal(g[2], x) and np.array_equal(w[3], x)
    assert got[1][0] == 0 and np.array_equal(got[1][2], b)
    # the Rice walk on damaged data, CRC recomputed, in the wide path too
    lo, sizes = frames_region(data[0])
    bad = refresh_crc(flip(data[0], (lo + 40) * 8 + 3), lo + 40)
    w = tta_port.decode(bad)
    g, = decoders.decode_tta_batch([bad])
    assert g[0] == w[0] and g[3] == w[2] and np.array_equal(g[2], w[3])


def test_kernel_times_named():
    from audiotools import _atgpu, decoders
    decoders.decode_tta_batch([clean()[1][0]])
    t = _atgpu.tta_decoder().kernel_times()
    assert set(t) == {"ttad_crc", "ttad_parse", "ttad_chain", "ttad_out", "ttad_total"}
