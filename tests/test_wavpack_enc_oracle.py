"""CPU: tests/wavpack_enc_port.py, the plain-Python WavPack encoder the GPU
tests compare against, reproduces the reference encoder: the 98 committed
images of tests/golden/wavpack_images.bin byte for byte, and the length and
MD5 that tests/golden/make_wavpack_enc_golden.py recorded for the cases of
tests/wavpack_enc_cases.py."""
import hashlib

import numpy as np
import pytest

import wavpack_cases as cases
import wavpack_enc_cases as enc_cases
import wavpack_enc_port as enc
import wavpack_port as dec

G, IMAGES = cases.load_vectors()
VECTORS = enc_cases.load_vectors()


def port_encode(opts, x, **extra):
    kw = enc.parse_options(opts)
    return enc.encode(x, kw["channels"], kw["mask"], kw["bps"], kw["rate"], kw["block_size"],
                      kw["passes"], kw["joint"], kw["false"], kw["wasted"], **extra)


def test_port_reproduces_the_committed_images():
    all_cases = cases.cases()
    assert len(all_cases) == 98
    for name, opts, ch, bps, rate, x in all_cases:
        assert port_encode(opts, x) == IMAGES[name], name


def test_every_new_case_has_a_vector():
    assert sorted(VECTORS) == sorted(c[0] for c in enc_cases.cases())


@pytest.mark.parametrize("name", sorted(VECTORS))
def test_port_reproduces_the_new_vectors(name):
    img = enc_cases.port_image(name)
    assert len(img) == VECTORS[name]["bytes"]
    assert hashlib.md5(img).hexdigest() == VECTORS[name]["md5"]


@pytest.mark.parametrize("name", sorted(VECTORS))
def test_port_images_decode_to_their_source(name):
    _, opts, ch, bps, rate, x = enc_cases.by_name()[name]
    st, info, pcm, _ = dec.decode(enc_cases.port_image(name))
    # the reference hashes 8-bit samples unsigned when it encodes and signed
    # when its stand-alone decoder checks: its own 8-bit files end so
    assert st == (dec.MD5_MISMATCH if bps == 8 else dec.OK)
    assert (info["channels"], info["bits_per_sample"], info["sample_rate"]) == (ch, bps, rate)
    assert np.array_equal(np.asarray(pcm, dtype=np.int64), x)


def test_total_pcm_frames_equal_to_the_length_changes_nothing():
    for name in ("long_p16_j1", "chan5_37", "one_frame"):
        _, opts, ch, bps, rate, x = enc_cases.by_name()[name]
        assert port_encode(opts, x, total_pcm_frames=len(x) // ch) == enc_cases.port_image(name)


def test_declared_total_is_written_in_every_header():
    """read from the reference's source: its stand-alone encoder always
    passes 0, so no vector covers a declared total that differs"""
    _, opts, ch, bps, rate, x = enc_cases.by_name()["chan4_107"]
    img = port_encode(opts, x, total_pcm_frames=7)
    base = enc_cases.port_image("chan4_107")
    assert len(img) == len(base)
    pos, n = 0, 0
    while pos < len(img):
        st, h = dec.parse_header(img, pos)
        assert st == dec.OK and h["total_samples"] == 7
        assert img[pos + 16:pos + 8 + h["block_size"]] == base[pos + 16:pos + 8 + h["block_size"]]
        pos += 8 + h["block_size"]
        n += 1
    assert n == 3 * 3 + 1


def test_short_blocks_with_passes_are_refused():
    x = np.zeros(64, dtype=np.int32)
    for ch, mask, block, passes in ((2, 3, 4, 16), (2, 3, 7, 16), (2, 3, 4, 10), (2, 3, 2, 5),
                                    (1, 4, 2, 5), (1, 4, 2, 16), (2, 3, 1, 1), (3, 7, 2, 10)):
        with pytest.raises(ValueError):
            enc.encode(x[:ch * 20], ch, mask, 16, 44100, block, passes, False, False, False)
    for ch, mask, block, passes in ((2, 3, 8, 16), (2, 3, 5, 10), (1, 4, 3, 16), (2, 3, 2, 2),
                                    (2, 3, 1, 0)):
        enc.encode(x[:ch * 20], ch, mask, 16, 44100, block, passes, False, False, False)
