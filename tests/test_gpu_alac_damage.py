"""GPU: the ALAC decoder (alac_decode.hip) on damaged streams.  ALAC has no
checksum, so a flipped bit goes straight into the parse, the frameset walk
and the channel restore.  Every single-bit flip of the mdat atom, every
truncation and every header flip that changes the reference decoder's
result (tests/golden/alac_damage_<image>.json, recorded by
tests/golden/make_alac_damage_golden.py) of three small images goes through
the decoder, each kind of case as ONE batch, with clean copies of the image
in between.  Every track of the batch must come out as it does decoded on
its own by the CPU oracle (oracle/alac_port.c) -- a write that strays into a
neighbour's workspace shows as that neighbour differing -- and, where the
reference has a defined result, as the reference recorded.  Every comparison
is exact: status and integers.

The last tests build what the sweep cannot reach from a valid image: a
frameset that carries more channels than any track of the batch declares
(the parse's residual slots are only that wide) and one longer than the
slot."""
import functools
import hashlib

import numpy as np
import pytest

import alac_cases
import oracle_port as op
import signals

pytestmark = pytest.mark.gpu
IMAGES = sorted(alac_cases.DAMAGE_IMAGES)
CLEAN_EVERY = 64


@functools.lru_cache(maxsize=None)
def _image(name):
    rec = alac_cases.damage_load(name)
    img, start, x = alac_cases.damage_image(name)
    assert hashlib.sha256(img).hexdigest() == rec["image_sha256"]
    aside = set()
    for c in alac_cases.DAMAGE_SET_ASIDE:
        aside |= set(rec["set_aside"][c])
    return rec, img, x, alac_cases.damage_cases(name, rec, img), aside


@functools.lru_cache(maxsize=None)
def _port(name, kind):
    """the oracle on every case of a kind, each image on its own; computed
    once and shared by the hints / no hints runs"""
    out = []
    for _, data, _ in _image(name)[3][kind]:
        status, pcm, bps = alac_cases.port_outcome(data)
        pcm.setflags(write=False)
        out.append((status, pcm, bps))
    return out


def _decode(images, hints):
    """one decode call over `images` -> per image (header status, info,
    status, int32 PCM); status and PCM are None where the header is refused
    (such an image is not part of the batch)"""
    from audiotools import _atgpu
    tracks, parts, heads, pos = [], [], [], 0
    for img in images:
        st, info, _, sizes = _atgpu.alac_read_info(img, sp_cap=16)
        heads.append((st, info))
        if st:
            continue
        pad = (-len(img)) % 4
        tracks.append(_atgpu.alac_dec_track(pos, len(img), info,
                                            frameset_bytes=sizes if hints else None))
        parts.append(img + b"\0" * pad)
        pos += len(img) + pad
    pcm, res, _, _ = _atgpu.alac_decoder().decode(b"".join(parts), tracks)
    out, k = [], 0
    for st, info in heads:
        if st:
            out.append((st, info, None, None))
            continue
        r = res[k]
        k += 1
        out.append((st, info, r.status,
                    pcm[r.sample_offset:r.sample_offset + r.pcm_frames * info.channels]))
    return out


def _with_clean_copies(cases, img):
    """the cases with a clean copy of the image before every CLEAN_EVERY-th
    and one at the end -> (images, positions of the clean copies)"""
    images, clean = [], []
    for i, c in enumerate(cases):
        if i % CLEAN_EVERY == 0:
            clean.append(len(images))
            images.append(img)
        images.append(c[1])
    clean.append(len(images))
    images.append(img)
    return images, clean


def _sweep(name, cases, port, hints, same_channels):
    """`cases` of an image (and the oracle's results `port` on them) as one
    batch -> how many the reference comparison skipped as channel mismatches"""
    from audiotools import _atgpu
    rec, img, x, _, aside = _image(name)
    n = rec["counts"]
    # the caps on what the reference comparison leaves out, from the record's
    # own counts: the reference dies on at most 0.5 % of an image's cases, and
    # at most 10 % of its mdat flips are channel mismatches
    assert 200 * len(rec["set_aside"]["reference_died"]) <= n["cases"]
    assert 10 * n["channel_mismatch_mdat_flips"] <= n["mdat_flips"]
    images, clean = _with_clean_copies(cases, img)
    got = _decode(images, hints)
    channels = alac_cases.DAMAGE_IMAGES[name]["channels"]
    for k in clean:
        st, info, status, pcm = got[k]
        assert st == 0 and status == 0 and np.array_equal(pcm, x), "clean copy at %d" % k
    cs = set(clean)
    mine = [g for k, g in enumerate(got) if k not in cs]
    assert len(mine) == len(cases) == len(port)
    skipped = 0
    for (key, data, outcome), (pstatus, ppcm, bps), (st, info, status, pcm) in \
            zip(cases, port, mine):
        # on its own in the oracle and in the batch on the GPU: the same
        if st:
            assert pstatus == 100 + st, (key, st, pstatus)
            status, pcm = 100 + st, ppcm
        else:
            if same_channels:  # the residual slots are as wide as the image's channels
                assert info.channels == channels, key
            assert status == pstatus and np.array_equal(pcm, ppcm), (key, status, pstatus)
        if key in aside:
            continue
        if status == _atgpu.AD_CHANNEL_MISMATCH:
            skipped += 1  # the Python path raises; the standalone has no check
            continue
        assert alac_cases.matches_reference(status, pcm, bps, outcome), (key, status, outcome)
    return skipped


@pytest.mark.parametrize("hints", [True, False], ids=["hints", "inline"])
@pytest.mark.parametrize("name", IMAGES)
def test_all_mdat_flips_one_batch(name, hints):
    """every single-bit flip of the mdat atom (hints: the stsz sizes, so the
    framesets go through k_adec_parse and its residual slots; without, the
    walk parses inline)"""
    skipped = _sweep(name, _image(name)[3]["mdat"], _port(name, "mdat"), hints, True)
    n = _image(name)[0]["counts"]
    assert skipped <= n["channel_mismatch_mdat_flips"] and 10 * skipped <= n["mdat_flips"]


@pytest.mark.parametrize("hints", [True, False], ids=["hints", "inline"])
@pytest.mark.parametrize("name", IMAGES)
def test_all_truncations_one_batch(name, hints):
    _sweep(name, _image(name)[3]["cut"], _port(name, "cut"), hints, True)


@pytest.mark.parametrize("hints", [True, False], ids=["hints", "inline"])
@pytest.mark.parametrize("name", [n for n in IMAGES if n != "three16"])
def test_header_flips_one_batch(name, hints):
    """every header flip on which the reference's result differs from the
    clean image's, in a batch of their own: a flipped channel count widens
    every residual slot of its batch.  A header whose channel count or
    sample size the decoder's interface refuses for the whole call
    (channels 1..8, bits per sample 1..32) cannot be part of a batch: those
    flips are left out here.  They are flips of those two bytes, 16 bits."""
    from audiotools import _atgpu
    cases, port, out = [], [], 0
    for c, p in zip(_image(name)[3]["header"], _port(name, "header")):
        st, info, _, _ = _atgpu.alac_read_info(c[1], sp_cap=16)
        if not st and not (1 <= info.channels <= 8 and 1 <= info.bits_per_sample <= 32):
            out += 1
            continue
        cases.append(c)
        port.append(p)
    assert out <= 16
    _sweep(name, cases, port, hints, False)


def _track(frames, channels, block, seed, declared=None, max_frame=None):
    """-> (m4a image, source PCM): `channels` in the mdat, `declared` in the
    container"""
    from audiotools import m4a
    x = signals.make("tone", frames, channels, 16, seed=seed)
    mdat, fs = op.alac_encode(x, channels, 16, block_size=block)
    return m4a.m4a_file(declared or channels, 16, 44100, max_frame or block, frames, mdat, fs,
                        create_date=1), x


@pytest.mark.parametrize("hints", [True, False], ids=["hints", "inline"])
@pytest.mark.parametrize("declared,carried", [(1, 2), (1, 8), (2, 6)])
def test_overdeclared_channels_leave_neighbours_alone(declared, carried, hints):
    """a frameset that carries more channels than its container, and every
    other track of the batch, declares: the parse's residual slots are
    `declared` channels wide, and the frameset's further channels must not
    be stored into the slots that follow (they belong to the valid tracks
    behind it).  Two valid tracks of five framesets each follow every bad
    one, so the 7 slots a frameset of 8 channels could reach all exist."""
    from audiotools import _atgpu
    valid = [_track(64 * 4 + 20, declared, 64, 40 + i) for i in range(7)]
    bad = [_track(64 * 2 + 5, carried, 64, 50 + i, declared=declared) for i in range(2)]
    order = [valid[0], bad[0], valid[1], valid[2], bad[1], valid[3], valid[4], valid[5],
             valid[6]]
    got = _decode([t[0] for t in order], hints)
    for i, ((img, x), (st, info, status, pcm)) in enumerate(zip(order, got)):
        assert st == 0 and info.channels == declared
        want = op.alac_decode(img)
        assert status == want["code"] and np.array_equal(pcm, want["pcm"]), i
        if any(img is b[0] for b in bad):
            assert status == _atgpu.AD_CHANNEL_MISMATCH, i
        else:
            assert status == 0 and np.array_equal(pcm, x), i


def test_frameset_longer_than_slot():
    """one frameset that states its own length, 200 samples, under a
    container whose max_samples_per_frame (the residual slot's length) is
    64: its residuals are not stored and the restore decodes them again"""
    long_img, long_x = _track(200, 1, 256, 60, max_frame=64)
    assert op.alac_read_info(long_img)[1].max_samples_per_frame == 64
    others = [_track(64 * 3 + 9, 1, 64, 61 + i) for i in range(4)]
    order = [others[0], (long_img, long_x), others[1], others[2], others[3]]
    got = _decode([t[0] for t in order], True)
    for i, ((img, x), (st, info, status, pcm)) in enumerate(zip(order, got)):
        want = op.alac_decode(img)
        assert st == 0 and status == want["code"] == 0, i
        assert np.array_equal(pcm, want["pcm"]) and np.array_equal(pcm, x), i
