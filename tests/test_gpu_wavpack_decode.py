"""GPU parity: libatgpu's WavPack decoder (wavpack_decode.hip) against the
reference decoder's recorded outcomes (tests/golden/wavpack_vectors.json:
status, md5 and length of the PCM oracle/_ref/wvdec wrote) over the good
images, the single-bit flips and the truncations, many images per call."""
import functools
import hashlib

import numpy as np
import pytest

import wavpack_cases as cases
import wavpack_port as port

pytestmark = pytest.mark.gpu
G, IMAGES = cases.load_vectors()


def file_bytes(pcm, bits):
    """the byte form wvdec writes: clamped to the width, little endian"""
    hi = (1 << (bits - 1)) - 1
    return cases.pcm_bytes(np.clip(np.asarray(pcm, dtype=np.int64), -hi - 1, hi), bits)


@functools.lru_cache(maxsize=None)
def damage():
    return cases.damage_cases(G, IMAGES)


@functools.lru_cache(maxsize=None)
def good_batch():
    """every good image in one call (1, 2, 3, 6 and 8 channels, 8, 16 and 24
    bits mixed)"""
    from audiotools import decoders
    names = sorted(IMAGES)
    return names, decoders.decode_wavpack_batch([IMAGES[n] for n in names])


def test_good_vectors_status_pcm_md5():
    names, got = good_batch()
    src = {c[0]: c for c in cases.cases()}
    formats = set()
    for name, (status, info, pcm, bad) in zip(names, got):
        v = G["images"][name]
        assert status == v["status"], name
        assert bad is None, name
        raw = file_bytes(pcm, info.bits_per_sample)
        assert len(raw) == v["bytes"], name
        assert hashlib.md5(raw).hexdigest() == v["md5"], name
        if v["source"]:
            assert np.array_equal(pcm, src[name][5]), name
        formats.add((info.channels, info.bits_per_sample))
    assert {(1, 8), (2, 16), (6, 24), (3, 16), (8, 16)} <= formats


def test_fixtures_decode_to_the_recorded_pcm():
    names, got = good_batch()
    for name, md5, nbytes in (("silence.wv", "9b1be87c", 882000),
                              ("wavpack-combo.wv", "0029a4d0", 176800)):
        status, info, pcm, bad = got[names.index(name)]
        raw = file_bytes(pcm, info.bits_per_sample)
        assert status == 0 and len(raw) == nbytes, name
        assert hashlib.md5(raw).hexdigest().startswith(md5), name


def test_eight_bit_md5_unsigned_mode():
    """the 8-bit images' MD5 was taken over unsigned bytes: mode 2 accepts
    them, mode 1 reports what wvdec reports"""
    from audiotools import decoders
    names = [n for n in sorted(IMAGES) if n.endswith("_b8")]
    for md5_mode, want in ((2, 0), (1, port.MD5_MISMATCH), (0, 0)):
        got = decoders.decode_wavpack_batch([IMAGES[n] for n in names], md5_mode=md5_mode)
        for name, (status, info, pcm, bad) in zip(names, got):
            assert status == want and bad is None, (name, md5_mode)
            assert len(pcm) == G["images"][name]["bytes"], name


def test_damage_vectors():
    """every recorded flip and cut, in one batch: the reference's status
    and the PCM it wrote before it; where the host's layout checks apply,
    any failure with exactly the PCM before the refused set"""
    from audiotools import decoders
    rows = damage()
    got = decoders.decode_wavpack_batch([r[1] for r in rows])
    flagged_seen = 0
    for (label, img, status, nbytes, md5, flagged), (st, info, pcm, bad) in zip(rows, got):
        raw = file_bytes(pcm, info.bits_per_sample) if info is not None else b""
        assert len(raw) == nbytes, label
        assert hashlib.md5(raw).hexdigest() == md5, label
        if flagged:
            assert st != 0, label
            flagged_seen += 1
        else:
            assert st == status, label
    assert 0 < flagged_seen * 10 < len(rows)


def patched(img, byte, mask):
    d = bytearray(img)
    d[byte] ^= mask
    return bytes(d)


def test_neighbours_and_guard():
    """a valid track between damaged ones keeps its PCM, and nothing is
    written past the batch's last sample"""
    from audiotools import _atgpu
    good = IMAGES[cases.DAMAGE_STEREO]
    three = IMAGES[cases.DAMAGE_3CH]
    last_of_set = _atgpu.wv_read_info(three)[2][1].offset
    bad = [patched(good, 24, 0x04),             # mono flag of the first block
           patched(three, 25, 0x10),            # final flag set early: the set shrinks
           patched(three, last_of_set + 25, 0x10),  # final flag cleared: the set stretches
           patched(good, 20, 0x08),             # block_samples 200 -> 208
           good[:len(good) - 300]]              # cut inside the last bitstream
    order = [bad[0], good, bad[1], three, bad[2], good, bad[3], three, bad[4]]
    parts, tracks, pos = [], [], 0
    for img in order:
        st, info, blocks = _atgpu.wv_read_info(img)
        assert st == 0
        pad = (-len(img)) % 4
        tracks.append(_atgpu.wv_dec_track(pos, len(img), info, blocks))
        parts.append(img + b"\0" * pad)
        pos += len(img) + pad
    dec = _atgpu.wv_decoder()
    pcm, res = dec.decode(b"".join(parts), tracks)
    guard = np.full(len(pcm) + 64, 0x5A5A5A5A, dtype=np.int32)
    pcm2, res2 = dec.decode(b"".join(parts), tracks, pcm_out=guard)
    assert np.array_equal(pcm, pcm2)
    assert np.all(guard[len(pcm):] == 0x5A5A5A5A)
    src = {c[0]: c[5] for c in cases.cases()}
    for k, r in enumerate(res):
        img = order[k]
        if img is good or img is three:
            want = src[cases.DAMAGE_STEREO if img is good else cases.DAMAGE_3CH]
            assert r.status == 0, k
            assert np.array_equal(pcm[r.sample_offset:r.sample_offset + len(want)], want), k
        else:
            st, info, ppcm, _ = port.decode(img)
            assert r.status != 0 and (r.status == st or st == port.INCONSISTENT_BLOCK), k
            assert np.array_equal(
                pcm[r.sample_offset:r.sample_offset + r.pcm_frames * r.channels],
                np.asarray(ppcm, dtype=np.int32)), k


def test_hostile_headers_between_valid_tracks(tmp_path):
    """images that no single-bit flip reaches end as tracks with a status;
    the batch goes on and their neighbours decode"""
    from audiotools import InvalidFile, InvalidWavPack, WavPackAudio, decoders
    (l0, zero), (l1, big) = cases.hostile_images(IMAGES)
    good, three = IMAGES[cases.DAMAGE_STEREO], IMAGES[cases.DAMAGE_3CH]
    src = {c[0]: c[5] for c in cases.cases()}
    got = decoders.decode_wavpack_batch([good, zero, three, big, good])
    for k, name in ((0, cases.DAMAGE_STEREO), (2, cases.DAMAGE_3CH), (4, cases.DAMAGE_STEREO)):
        assert got[k][0] == 0 and np.array_equal(got[k][2], src[name]), k
    assert got[1][0] == port.CHANNELS_UNDEFINED and got[1][1] is None and len(got[1][2]) == 0
    assert got[3][0] == port.INCONSISTENT_BLOCK and len(got[3][2]) == 0 and got[3][3] == 0
    with pytest.raises(ValueError, match="channel count/mask undefined"):
        decoders.WavPackDecoder(zero)
    d = decoders.WavPackDecoder(big)
    with pytest.raises(ValueError, match="inconsistent block header"):
        d.read(4096)
    for name, data in (("zero.wv", zero), ("big.wv", big)):
        fn = str(tmp_path / name)
        with open(fn, "wb") as f:
            f.write(data)
    with pytest.raises(InvalidWavPack):
        WavPackAudio(str(tmp_path / "zero.wv"))
    with pytest.raises(InvalidFile):
        WavPackAudio(str(tmp_path / "big.wv")).verify()


def test_device_entry_matches_host_entry():
    import torch
    from audiotools import _atgpu
    names = ["chan6", "tone_c1_b8", "noise_p16_j_b24", "wavpack-combo.wv", "len7_c2_p16"]
    parts, tracks, pos = [], [], 0
    for n in names:
        img = IMAGES[n]
        st, info, blocks = _atgpu.wv_read_info(img)
        pad = (-len(img)) % 4
        tracks.append(_atgpu.wv_dec_track(pos, len(img), info, blocks))
        parts.append(img + b"\0" * pad)
        pos += len(img) + pad
    blob = b"".join(parts)
    dec = _atgpu.wv_decoder()
    pcm, res = dec.decode(blob, tracks)
    pcm = pcm.copy()
    d = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    dres, d_pcm, ns = dec.decode_device(d.data_ptr(), len(blob), tracks)
    assert ns == len(pcm) and d_pcm
    assert np.array_equal(dec.fetch(ns), pcm)
    for a, b in zip(res, dres):
        assert (a.status, a.n_sets, a.pcm_frames, a.sample_offset, a.channels) == \
            (b.status, b.n_sets, b.pcm_frames, b.sample_offset, b.channels)


def test_contradictory_table_is_refused():
    """the decoder checks the table again: blocks of a set that disagree on
    block_samples are an error, not a launch"""
    from audiotools import _atgpu
    img = IMAGES[cases.DAMAGE_3CH]
    st, info, blocks = _atgpu.wv_read_info(img)
    blocks[1].block_samples += 1
    track = _atgpu.wv_dec_track(0, len(img), info, blocks)
    with pytest.raises(_atgpu.ATGError):
        _atgpu.wv_decoder().decode(img + b"\0" * ((-len(img)) % 4), [track])
    st, info, blocks = _atgpu.wv_read_info(img)
    track = _atgpu.wv_dec_track(0, len(img), info, blocks)
    track.bits_per_sample = 12
    with pytest.raises(_atgpu.ATGError, match="bits per sample"):
        _atgpu.wv_decoder().decode(img + b"\0" * ((-len(img)) % 4), [track])
