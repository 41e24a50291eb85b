"""GPU parity: libatgpu's WavPack encoder (wavpack_encode.hip) against the
reference encoder: the 98 committed images of tests/golden/wavpack_images.bin
byte for byte, the recorded length and MD5 of the cases of
tests/wavpack_enc_cases.py, and tests/wavpack_enc_port.py wherever no
reference vector reaches."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import wavpack_cases as cases
import wavpack_enc_cases as enc_cases
import wavpack_enc_port as port

pytestmark = pytest.mark.gpu
G, IMAGES = cases.load_vectors()
VECTORS = enc_cases.load_vectors()


def options_of(opts):
    kw = port.parse_options(opts)
    fmt = (kw["channels"], kw["mask"], kw["bps"], kw["rate"])
    enc = (kw["block_size"], kw["passes"], kw["false"], kw["wasted"], kw["joint"])
    return fmt, enc


def encode_batch(fmt, enc, signals, out=None):
    """one atg_wv_encode_host call -> ([image bytes], results, block sizes)"""
    from audiotools import _atgpu
    channels, mask, bps, rate = fmt
    e = _atgpu.wv_encoder()
    tracks, start = [], 0
    for x in signals:
        tracks.append((start, len(x) // channels))
        start += len(x) // channels
    pcm = np.concatenate([np.asarray(x, dtype=np.int32) for x in signals] +
                         [np.zeros(0, dtype=np.int32)])
    pcm = pcm.astype(np.int16 if bps <= 16 else np.int32)
    buf, res, sizes = e.encode(e.options(*enc), pcm, tracks, channels, mask, bps, rate, out=out)
    return [buf[r.out_offset:r.out_offset + r.bytes].tobytes() for r in res], res, sizes


def encode_grouped(all_cases):
    """the cases that share a format and options go through one call"""
    groups = {}
    for name, opts, ch, bps, rate, x in all_cases:
        groups.setdefault(options_of(opts), []).append((name, x))
    got = {}
    for (fmt, enc), members in groups.items():
        images, res, _ = encode_batch(fmt, enc, [x for _, x in members])
        for (name, x), img, r in zip(members, images, res):
            assert r.status == 0 and r.pcm_frames == len(x) // fmt[0], name
            got[name] = (img, bytes(r.md5))
    return got


@functools.lru_cache(maxsize=None)
def committed_encoded():
    return encode_grouped(cases.cases())


@functools.lru_cache(maxsize=None)
def new_encoded():
    return encode_grouped(enc_cases.cases())


def test_the_98_committed_images():
    got = committed_encoded()
    assert len(got) == 98
    for name in sorted(got):
        assert got[name][0] == IMAGES[name], name


def test_result_md5_is_the_footer_md5():
    for name, (img, md5) in committed_encoded().items():
        if name != "empty_c2":      # there the RIFF header lies over the MD5 sub-block
            assert img[-16:] == md5, name
    src = {c[0]: c for c in cases.cases()}
    _, _, ch, bps, rate, x = src["tone_c2_b8"]
    assert committed_encoded()["tone_c2_b8"][1] == hashlib.md5(port.md5_bytes(x, 8)).digest()


@pytest.mark.parametrize("name", sorted(VECTORS))
def test_new_vectors(name):
    img = new_encoded()[name][0]
    assert len(img) == VECTORS[name]["bytes"]
    assert hashlib.md5(img).hexdigest() == VECTORS[name]["md5"]
    assert img == enc_cases.port_image(name)


MIXED_FMT = (2, 3, 16, 44100)
MIXED_ENC = (56, 16, True, True, True)


def mixed_signals():
    import signals
    t = signals.make("tone", 400, 2, 16, seed=61)
    return [np.zeros(0, dtype=np.int32), np.array([5, -5], dtype=np.int32), t[:2 * 130],
            np.repeat(t[:111], 2), np.zeros(0, dtype=np.int32), t[:2 * 56], t]


def test_mixed_batch_equals_tracks_alone():
    sigs = mixed_signals()
    together, res, sizes = encode_batch(MIXED_FMT, MIXED_ENC, sigs)
    first = 0
    for k, x in enumerate(sigs):
        alone, _, _ = encode_batch(MIXED_FMT, MIXED_ENC, [x])
        assert together[k] == alone[0], k
        assert together[k] == port.encode(x, 2, 3, 16, 44100, 56, 16, True, True, True), k
        n = res[k].n_blocks
        assert res[k].first_block == first and n == (len(x) // 2 + 55) // 56
        first += n
        # the blocks and the 50-byte footer add up to the image
        assert int(sizes[res[k].first_block:first].sum()) + (50 if n else 78) == res[k].bytes
        assert res[k].out_offset % 16 == 0
    assert together[0] == IMAGES["empty_c2"]


def test_capacity():
    from audiotools import _atgpu
    sigs = mixed_signals()
    images, res, _ = encode_batch(MIXED_FMT, MIXED_ENC, sigs)
    needed = res[-1].out_offset + res[-1].bytes
    short = np.full(needed - 1, 0xA5, dtype=np.uint8)
    with pytest.raises(_atgpu.ATGError) as err:
        encode_batch(MIXED_FMT, MIXED_ENC, sigs, out=short)
    assert err.value.status == _atgpu.ATG_ERR_CAPACITY
    assert err.value.needed == needed
    assert (short == 0xA5).all()
    exact = np.full(err.value.needed, 0xA5, dtype=np.uint8)
    again, _, _ = encode_batch(MIXED_FMT, MIXED_ENC, sigs, out=exact)
    assert again == images


def test_device_entry_gives_the_same_bytes():
    import torch
    from audiotools import _atgpu
    sigs = mixed_signals()
    images, res, sizes = encode_batch(MIXED_FMT, MIXED_ENC, sigs)
    needed = res[-1].out_offset + res[-1].bytes
    e = _atgpu.wv_encoder()
    tracks, start = [], 0
    for x in sigs:
        tracks.append((start, len(x) // 2))
        start += len(x) // 2
    for dtype, fmt in ((torch.int16, _atgpu.PCM_S16), (torch.int32, _atgpu.PCM_S32)):
        d_pcm = torch.from_numpy(np.concatenate(sigs).astype(np.int32)).to("cuda").to(dtype)
        d_out = torch.full((needed + 8,), 0x5A, dtype=torch.uint8, device="cuda")
        bsb = np.zeros(len(sizes), dtype=np.uint32)
        with pytest.raises(_atgpu.ATGError) as err:
            e.encode_device(e.options(*MIXED_ENC), d_pcm.data_ptr(), fmt, tracks, 2, 3, 16, 44100,
                            d_out.data_ptr(), needed - 1)
        assert err.value.status == _atgpu.ATG_ERR_CAPACITY and err.value.needed == needed
        torch.cuda.synchronize()
        assert bool((d_out == 0x5A).all())
        dres, need = e.encode_device(e.options(*MIXED_ENC), d_pcm.data_ptr(), fmt, tracks, 2, 3,
                                     16, 44100, d_out.data_ptr(), needed, block_bytes=bsb)
        torch.cuda.synchronize()
        host = d_out.cpu().numpy()
        assert need == needed and (host[needed:] == 0x5A).all()
        assert np.array_equal(bsb, sizes)
        for r, want in zip(dres, images):
            assert host[r.out_offset:r.out_offset + r.bytes].tobytes() == want


def call_host(channels, mask, bps, rate, enc, tracks, n_samples=64, dtype=np.int16):
    """the raw status of atg_wv_encode_host"""
    from audiotools import _atgpu
    e = _atgpu.wv_encoder()
    arr, n, keep = _atgpu._track_array(tracks)
    pcm = np.zeros(n_samples, dtype=dtype)
    out = np.zeros(4096, dtype=np.uint8)
    res = (_atgpu.WvTrackResult * max(1, n))()
    opts = e.options(*enc)
    return e.lib.atg_wv_encode_host(
        e.handle, pcm.ctypes.data_as(ctypes.c_void_p),
        _atgpu.PCM_S16 if dtype == np.int16 else _atgpu.PCM_S32, arr, n, channels, mask, bps,
        rate, ctypes.byref(opts), out.ctypes.data_as(ctypes.c_void_p), len(out), res, None, 0,
        None)


def test_refused_arguments():
    from audiotools import _atgpu
    inv, uns = _atgpu.ATG_ERR_INVALID, _atgpu.ATG_ERR_UNSUPPORTED
    ok = (8, 5, False, False, False)
    one = [(0, 16)]
    assert call_host(2, 3, 16, 44100, ok, one) == 0
    assert call_host(2, 3, 12, 44100, ok, one) == inv
    assert call_host(2, 3, 32, 44100, ok, one, dtype=np.int32) == inv
    assert call_host(0, 0, 16, 44100, ok, one) == inv
    for passes in (3, 4, 6, 15, 17):
        assert call_host(2, 3, 16, 44100, (8, passes, False, False, False), one) == inv
    assert call_host(2, 3, 16, 44100, (0, 5, False, False, False), one) == inv
    # the reference aborts on these: -B 4 -p 16 stereo, -B 2 -p 5 mono
    assert call_host(2, 3, 16, 44100, (4, 16, False, False, False), one) == inv
    assert call_host(1, 4, 16, 44100, (2, 5, False, False, False), one) == inv
    for ch, mask, block, passes, want in ((2, 3, 7, 16, inv), (2, 3, 8, 16, 0), (2, 3, 4, 10, inv),
                                          (2, 3, 5, 10, 0), (2, 3, 2, 5, inv), (2, 3, 3, 5, 0),
                                          (1, 4, 3, 16, 0), (1, 4, 2, 10, inv), (2, 3, 1, 1, inv),
                                          (2, 3, 2, 2, 0), (1, 4, 1, 2, inv), (2, 3, 1, 0, 0),
                                          # 2+1: the mono stream's table is the shallower one
                                          (3, 7, 7, 16, inv), (3, 7, 8, 16, 0)):
        got = call_host(ch, mask, 16, 44100, (block, passes, False, False, False), [(0, 16)])
        assert got == want, (ch, block, passes)
    assert call_host(2, 3, 16, 44100, ok, [(0, 0xFFFFFFFF)]) == inv
    assert call_host(2, 3, 16, 44100, ok, [(0, 16, [8, 8])]) == uns


def test_seeded_random_batches_against_port_and_decoder():
    """12 tracks of 0..300 frames at random legal options, compared with the
    port; every image then goes through the GPU decoder, MD5 checked as the
    encoder hashes (8-bit unsigned)"""
    from audiotools import decoders
    rng = np.random.default_rng(20240917)
    formats = [(1, 4, 16), (2, 3, 16), (2, 3, 24), (2, 3, 8), (3, 7, 16), (6, 0x3F, 24)]
    images, sources = [], []
    for k in range(4):
        ch, mask, bps = formats[int(rng.integers(len(formats)))] if k else (2, 3, 16)
        passes = int(rng.choice([0, 1, 2, 5, 10, 16]))
        block = int(rng.integers(max(1, port.min_block_size(ch, mask, passes)), 90))
        joint, false, wasted = (bool(v) for v in rng.integers(0, 2, 3))
        sigs = []
        for t in range(3):
            n = int(rng.integers(0, 301))
            kind = int(rng.integers(4))
            lim = 1 << (bps - 1)
            if kind == 0:
                x = rng.integers(-lim, lim, n * ch)
            elif kind == 1:
                x = (rng.integers(-lim >> 4, lim >> 4, n * ch) >> 2) << 2
            elif kind == 2:
                x = np.repeat(rng.integers(-lim >> 2, lim >> 2, n), ch)
                x[n * ch // 2:] = 0
            else:
                t0 = np.arange(n)[:, None] + np.arange(ch)[None, :] * 7
                x = np.round((lim >> 2) * np.sin(t0 / 9.0) + rng.normal(0, 3, (n, ch))).reshape(-1)
            sigs.append(np.asarray(x, dtype=np.int32))
        got, res, _ = encode_batch((ch, mask, bps, 44100), (block, passes, false, wasted, joint),
                                   sigs)
        for x, img in zip(sigs, got):
            want = port.encode(x, ch, mask, bps, 44100, block, passes, joint, false, wasted)
            assert img == want, (k, ch, bps, block, passes, joint, false, wasted, len(x))
            images.append(img)
            sources.append(x)
    assert len(images) == 12
    for (status, info, pcm, bad), x in zip(decoders.decode_wavpack_batch(images, md5_mode=2),
                                           sources):
        assert status == 0 and bad is None
        assert np.array_equal(pcm, x)
