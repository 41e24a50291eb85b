"""GPU: accuraterip.hip against the reference's known answers and the numpy
port (tests/accuraterip_port.py) -- the classes, the batch call at the edge
lengths, a track fed in pieces, the offset sweep against brute force on an
image and on separate files, verify_flac_batch, and the host path."""
import functools
import json
import os

import numpy as np
import pytest

import accuraterip_port as port
import oracle_port
from audiotools import _accuraterip, _atgpu, accuraterip, pcm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
VECTORS = json.load(open(os.path.join(GOLDEN, "accuraterip_vectors.json")))
TONE = open(os.path.join(GOLDEN, VECTORS["fixture"]), "rb").read()
FLAGS = [(True, False), (False, False), (False, True), (True, True)]
FMTS = {"s16": (_atgpu.PCM_S16, np.int16), "s32": (_atgpu.PCM_S32, np.int32)}


@pytest.fixture(scope="module")
def tone():
    """tone.flac decoded on the GPU -> (int32 samples, rate)"""
    # imported here: decoders loads libatgpu.so, which must come after torch
    from audiotools import decoders
    ((status, si, samples),) = decoders.decode_flac_batch([TONE])
    assert status == 0 and (si.channels, si.bits_per_sample) == (2, 16)
    return samples.copy(), si.sample_rate


def _want(first, last):
    (v,) = [v for v in VECTORS["vectors"] if (v["is_first"], v["is_last"]) == (first, last)]
    return int(v["v1"], 16), int(v["v2"], 16)


# ---- known answers ----------------------------------------------------------
@pytest.mark.parametrize("first,last", FLAGS)
@pytest.mark.parametrize("chunk", [1, 4096, 4097, 262144])
def test_classes_give_the_reference_values(tone, chunk, first, last):
    samples, rate = tone
    total = len(samples) // 2
    c1 = _accuraterip.ChecksumV1(first, last, rate, total)
    c2 = _accuraterip.ChecksumV2(first, last, rate, total)
    for i in range(0, len(samples), 2 * chunk):
        fl = pcm.FrameList._wrap(samples[i:i + 2 * chunk], 2, 16)
        c1.update(fl)
        c2.update(fl)
    got = (c1.checksum(), c2.checksum())
    print("chunk %d first %d last %d: %08X %08X" % ((chunk, first, last) + got))
    assert got == _want(first, last)


def test_verify_flac_batch_gives_the_reference_values():
    ((r,),) = accuraterip.verify_flac_batch([[TONE]])
    print("verify_flac_batch: status %s %08X %08X" % (r.status, r.v1, r.v2))
    assert r.status == 0 and r.error is None
    assert (r.v1, r.v2) == _want(True, True)
    assert r.offsets is None and r.match is None


# ---- edge lengths -----------------------------------------------------------
def _signal(n, kind, seed):
    """interleaved stereo: noise, or noise with runs of -32768, 32767 and -1
    on both channels (0x80008000, 0x7FFF7FFF and 0xFFFFFFFF as frame values,
    so the products' high words carry)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, size=(n, 2)).astype(np.int32)
    if kind:
        run = (-32768, 32767, -1)[kind - 1]
        x[n // 4:n - n // 4] = run
    return x.reshape(-1)


def _lengths():
    tile = _atgpu.accuraterip_tile_frames()
    return [1, 2, 63, 64, 65, 2939, 2940, 2941, 5879, 5880, 5881, tile - 1, tile, tile + 1]


@pytest.mark.parametrize("rate", [44100, 48000, 8000])
@pytest.mark.parametrize("fmt", sorted(FMTS))
def test_batch_edge_lengths(fmt, rate):
    """70 tracks back to back (so they start mid-tile and mid-wave): every
    length with every first/last pair, then 14 more with the lengths turned
    round; v1 and v2 of each against the port"""
    code, dtype = FMTS[fmt]
    lens = _lengths()
    cases = [(n, f, l) for n in lens for (f, l) in FLAGS]
    cases += [(n, f, l) for n, (f, l) in zip(reversed(lens), FLAGS * 4)][:14]
    assert len(cases) == 70
    parts, tracks, pos = [], [], 0
    for i, (n, f, l) in enumerate(cases):
        parts.append(_signal(n, i % 4, seed=1000 + i))
        tracks.append(accuraterip.track(pos, n, rate, f, l))
        pos += n
    img = np.concatenate(parts).astype(dtype)
    got, table = accuraterip.checksum_batch(img, tracks)
    assert table.shape == (70, 1)
    for i, ((n, f, l), p) in enumerate(zip(cases, parts)):
        want = port.checksums(p, f, l, rate)
        assert got[i] == want, (i, n, f, l, "%08X %08X" % got[i], "%08X %08X" % want)
        assert table[i, 0] == want[0]


@pytest.mark.parametrize("fmt", sorted(FMTS))
def test_track_in_pieces_with_index0(fmt):
    """20,000 frames as pieces of 1, 4999 and 15,000 with the running
    index0; first and last, so the skip boundaries (2940 and 17,060) fall
    inside the second and third piece"""
    code, dtype = FMTS[fmt]
    n, rate = 20000, 44100
    x = _signal(n, 1, seed=7)
    tracks, pos = [], 0
    for m in (1, 4999, 15000):
        tracks.append(accuraterip.track(pos, m, rate, True, True, index0=pos,
                                        total_pcm_frames=n))
        pos += m
    tracks.append(accuraterip.track(0, n, rate, True, True))
    got, _ = accuraterip.checksum_batch(x.astype(dtype), tracks)
    want = port.checksums(x, True, True, rate)
    assert got[3] == want
    assert tuple(sum(g[i] for g in got[:3]) & 0xFFFFFFFF for i in (0, 1)) == want
    # and each piece is what the port gives for it
    pos = 0
    for g, m in zip(got, (1, 4999, 15000)):
        assert g == port.checksums(x[2 * pos:2 * (pos + m)], True, True, rate, n, pos)
        pos += m


# ---- sweep ------------------------------------------------------------------
IMAGE_LENGTHS = [6000, 20011, 7001]
RATE = 44100


@functools.lru_cache(maxsize=None)
def _image():
    parts = [_signal(n, k, seed=50 + k) for k, n in enumerate(IMAGE_LENGTHS)]
    return np.concatenate(parts), _signal(6000, 0, seed=60)


def _layout(lengths, as_image):
    """[(pcm_offset, frames, first, last, lo, hi)] of an image's tracks"""
    total, out, pos = sum(lengths), [], 0
    for t, n in enumerate(lengths):
        lo, hi = (0, total) if as_image else (pos, pos + n)
        out.append((pos, n, t == 0, t == len(lengths) - 1, lo, hi))
        pos += n
    return out


@functools.lru_cache(maxsize=None)
def _brute(K, which):
    """the port's brute-force tables, computed once per (K, layout)"""
    three, one = _image()
    img, lengths, as_image = {"image": (three, IMAGE_LENGTHS, True),
                              "files": (three, IMAGE_LENGTHS, False),
                              "single": (one, [6000], True)}[which]
    return [port.sweep(img, p, n, lo, hi, f, l, RATE, K)
            for (p, n, f, l, lo, hi) in _layout(lengths, as_image)]


def _gpu_sweep(img, lengths, as_image, K, dtype=np.int32):
    tracks = [accuraterip.track(p, n, RATE, f, l, lo, hi)
              for (p, n, f, l, lo, hi) in _layout(lengths, as_image)]
    return accuraterip.checksum_batch(img.astype(dtype), tracks, max_offset=K)


@pytest.mark.parametrize("K", [0, 1, 7, 588, 2940])
@pytest.mark.parametrize("which", ["image", "single"])
def test_sweep_equals_brute_force(which, K):
    three, one = _image()
    img, lengths = (three, IMAGE_LENGTHS) if which == "image" else (one, [6000])
    res, table = _gpu_sweep(img, lengths, True, K)
    want = np.array(_brute(K, which), dtype=np.uint32)
    assert table.shape == want.shape == (len(lengths), 2 * K + 1)
    bad = np.argwhere(table != want)
    assert len(bad) == 0, ("first mismatches (track, k + K):", bad[:8].tolist())
    assert [r[0] for r in res] == table[:, K].tolist()


@pytest.mark.parametrize("K", [7, 2940])
def test_sweep_separate_files(K):
    """the same tracks with the region cut to each track: neighbours are
    silent, so the tables leave the image's wherever a neighbour slid in"""
    three, _ = _image()
    _, files = _gpu_sweep(three, IMAGE_LENGTHS, False, K, np.int16)
    want = np.array(_brute(K, "files"), dtype=np.uint32)
    assert np.array_equal(files, want)
    image = np.array(_brute(K, "image"), dtype=np.uint32)
    assert np.array_equal(files[:, K], image[:, K])
    differs = files != image
    # the middle track has a neighbour on both sides: every k != 0 differs
    assert differs[1, :K].all() and differs[1, K + 1:].all()
    # the first only behind it (k > 0), the last only before it (k < 0)
    assert differs[0, K + 1:].all() and not differs[0, :K].any()
    assert differs[2, :K].all() and not differs[2, K + 1:].any()


@pytest.mark.parametrize("k", [-3, 5])
def test_v2_at_an_offset_by_shifted_pcm_offset(k):
    three, _ = _image()
    layout = _layout(IMAGE_LENGTHS, True)
    tracks = [accuraterip.track(p + k, n, RATE, f, l, lo, hi) for (p, n, f, l, lo, hi) in layout]
    got, _ = accuraterip.checksum_batch(three, tracks)
    for g, (p, n, f, l, lo, hi) in zip(got, layout):
        assert g == port.checksums(port.window(three, p + k, n, lo, hi), f, l, RATE)
    assert [g[0] for g in got] == [row[k + 7] for row in _brute(7, "image")]


# ---- verify_flac_batch ------------------------------------------------------
def _encode(gpu_engine, parts, bps=16):
    tracks, pos = [], 0
    for p in parts:
        tracks.append((pos, len(p) // 2))
        pos += len(p) // 2
    x = np.concatenate(parts).astype(np.int16 if bps == 16 else np.int32)
    opts = _atgpu.make_options(**oracle_port.PRESETS["8"])
    out, res, _, _ = gpu_engine.encode(opts, x, tracks, 2, bps, RATE)
    return [out[r.out_offset:r.out_offset + r.bytes].tobytes() for r in res]


ALBUM_LENGTHS = [[7000, 9001, 6500], [3001, 4100, 12345]]


@pytest.fixture(scope="module")
def albums(gpu_engine):
    pcms = [[_signal(n, (a + t) % 4, seed=200 + 10 * a + t) for t, n in enumerate(row)]
            for a, row in enumerate(ALBUM_LENGTHS)]
    flat = _encode(gpu_engine, [p for row in pcms for p in row])
    return pcms, [flat[:3], flat[3:]]


def test_verify_flac_batch_two_albums(albums):
    pcms, images = albums
    want = [[port.checksums(p, t == 0, t == 2, RATE) for t, p in enumerate(row)] for row in pcms]
    ar = [{1: [(9, 1, 0), (5, want[0][0][0], 0)], 2: [(3, want[0][1][0] ^ 1, 0)], 3: []}, None]
    got = accuraterip.verify_flac_batch(images, ar_matches=ar, max_offset=2)
    for a in range(2):
        for t in range(3):
            r = got[a][t]
            assert (r.status, r.error) == (0, None)
            assert (r.v1, r.v2) == want[a][t], (a, t)
            n = len(pcms[a][t]) // 2
            assert [r.offsets[k] for k in range(-2, 3)] == port.sweep(
                pcms[a][t], 0, n, 0, n, t == 0, t == 2, RATE, 2)
    assert [r.match for r in got[0]] == [5, accuraterip.AR_MISMATCH, accuraterip.AR_NOT_FOUND]
    assert [r.match for r in got[1]] == [accuraterip.AR_NOT_FOUND] * 3
    # without ar_matches and offsets the same checksums, nothing else
    plain = accuraterip.verify_flac_batch(images)
    assert [[(r.v1, r.v2, r.offsets, r.match) for r in row] for row in plain] == \
        [[w + (None, None) for w in row] for row in want]


def test_verify_flac_batch_damaged_and_24_bit(albums, gpu_engine):
    pcms, images = albums
    good = images[0]
    broken = bytearray(good[1])
    broken[len(broken) // 2] ^= 0x10  # inside a frame: its CRC-16 fails
    (wide,) = _encode(gpu_engine, [_signal(5000, 0, seed=9) * 200], bps=24)
    got = accuraterip.verify_flac_batch([[good[0], bytes(broken), wide, good[2]]])[0]
    assert got[0].status == 0 and got[3].status == 0
    assert (got[0].v1, got[0].v2) == port.checksums(pcms[0][0], True, False, RATE)
    assert (got[3].v1, got[3].v2) == port.checksums(pcms[0][2], False, True, RATE)
    assert got[1].status not in (0, None) and got[1].v1 is None and got[1].v2 is None
    assert "decode status" in got[1].error
    assert got[2].v1 is None and got[2].v2 is None and "24 bits" in got[2].error


# ---- host path --------------------------------------------------------------
def test_host_path_is_deterministic_and_equals_device_path():
    import torch
    three, _ = _image()
    tracks = [accuraterip.track(p, n, RATE, f, l, lo, hi)
              for (p, n, f, l, lo, hi) in _layout(IMAGE_LENGTHS, True)]
    a = accuraterip.checksum_batch(three, tracks, max_offset=588)
    b = accuraterip.checksum_batch(three, tracks, max_offset=588)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    d = torch.from_numpy(three).cuda()
    torch.cuda.synchronize()
    c = accuraterip.checksum_batch((d.data_ptr(), _atgpu.PCM_S32), tracks, max_offset=588,
                                   device_pcm=True)
    assert a[0] == c[0] and np.array_equal(a[1], c[1])
    d16 = torch.from_numpy(three.astype(np.int16)).cuda()
    torch.cuda.synchronize()
    e = accuraterip.checksum_batch((d16.data_ptr(), _atgpu.PCM_S16), tracks, max_offset=588,
                                   device_pcm=True)
    assert a[0] == e[0] and np.array_equal(a[1], e[1])
