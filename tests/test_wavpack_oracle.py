"""CPU: the WavPack checker (tests/wavpack_port.py) against the reference
decoder's recorded outcomes (tests/golden/wavpack_vectors.json, made by
tests/golden/make_wavpack_golden.py), and libatgpu's host-side stream reader
(atg_wv_read_info) against the checker, the reference's fixtures, damaged
headers and cuts.  No kernel is launched."""
import functools
import hashlib
import os
import subprocess

import pytest

import wavpack_cases as cases
import wavpack_port as port

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WVDEC = os.path.join(ROOT, "oracle", "_ref", "wvdec")
G, IMAGES = cases.load_vectors()


@functools.lru_cache(maxsize=None)
def damage():
    return cases.damage_cases(G, IMAGES)


def outcome(image):
    st, info, pcm, _ = port.decode(image)
    raw = port.pcm_bytes(pcm, info["bits_per_sample"]) if info else b""
    return st, raw


def test_vector_set_matches_cases():
    want = [c[0] for c in cases.cases()] + [p[0] for p in cases.PATCHED] + list(cases.FIXTURES)
    assert sorted(G["images"]) == sorted(want)
    d = G["damage"]
    assert d["left_out_count"] == len(d["left_out"])
    assert d["left_out_count"] * 50 <= d["cases"]
    assert all(e["reason"] for e in d["left_out"])
    assert len(damage()) + d["left_out_count"] == d["cases"]
    flips = cases.flip_cases(len(IMAGES[cases.DAMAGE_STEREO]))
    got = [r for r in damage() if r[0].startswith(cases.DAMAGE_STEREO + " flip")]
    assert len(got) >= len(flips) - d["left_out_count"]


def test_exp2_table_is_generated():
    """the 256-entry table is floor(256 * 2**(i/256) + 0.5); its ends and the
    entries next to a rounding boundary"""
    assert port.EXP2[0] == 0x100 and port.EXP2[255] == 0x1FF and port.EXP2[128] == 0x16A
    assert all(a <= b for a, b in zip(port.EXP2, port.EXP2[1:]))


def test_port_reproduces_good_vectors():
    src = {c[0]: c for c in cases.cases()}
    for name, v in sorted(G["images"].items()):
        st, raw = outcome(IMAGES[name])
        # wvdec hashes 8-bit samples signed where the encoder hashed them
        # unsigned: its own 8-bit files end with an MD5 mismatch, all PCM out
        want = port.MD5_MISMATCH if (v["bytes"] and name.endswith("_b8")) else 0
        assert st == v["status"] == want and (v["returncode"] == 0) == (st == 0), name
        assert len(raw) == v["bytes"], name
        assert hashlib.md5(raw).hexdigest() == v["md5"], name
        if v["source"]:
            _, _, ch, bps, rate, x = src[name]
            assert raw == cases.pcm_bytes(x, bps), name


def test_fixture_md5s():
    assert G["images"]["silence.wv"]["md5"].startswith("9b1be87c")
    assert G["images"]["silence.wv"]["bytes"] == 882000
    assert G["images"]["wavpack-combo.wv"]["md5"].startswith("0029a4d0")
    assert G["images"]["wavpack-combo.wv"]["bytes"] == 176800


def test_port_reproduces_damage_vectors():
    """every third recorded flip and cut (the golden script runs them all)"""
    for label, img, status, nbytes, md5, flagged in damage()[::3]:
        st, raw = outcome(img)
        assert st == status, label
        assert len(raw) == nbytes and hashlib.md5(raw).hexdigest() == md5, label
        assert bool(flagged) == (st == port.INCONSISTENT_BLOCK), label


def _table(image):
    from audiotools import _atgpu
    st, info, blocks = _atgpu.wv_read_info(image)
    return st, info, blocks


def check_read_info(label, image):
    """atg_wv_read_info against the port's read_info, field for field"""
    st, info, blocks = _table(image)
    pst, pinfo, psets, pend = port.read_info(image)
    assert st == pst, label
    if st:
        return
    for f in ("sample_rate", "bits_per_sample", "channels", "channel_mask", "total_pcm_frames"):
        assert getattr(info, f) == pinfo[f], (label, f)
    assert info.end_status == pend, label
    assert info.n_sets == len(psets), label
    want = [(k, h) for k, s in enumerate(psets) for h in s] + \
        [(len(psets), h) for h in pinfo["end_blocks"]]
    assert info.n_blocks == len(want) and info.tail_blocks == len(pinfo["end_blocks"]), label
    for b, (k, h) in zip(blocks, want):
        assert (b.offset, b.size) == (h["offset"], h["data"][1]), label
        assert (b.block_index, b.block_samples, b.flags, b.crc) == \
            (h["block_index"], h["block_samples"], h["flags"], h["crc"]), label
        assert (b.set, b.first_channel) == (k, h["first_channel"]), label
    assert bool(info.has_md5) == (pinfo["md5"] is not None), label
    if pinfo["md5"] is not None:
        assert bytes(info.md5) == pinfo["md5"], label
    assert info.end_offset == pinfo["end_offset"], label


def test_read_info_good_vectors_and_fixtures():
    for name in sorted(IMAGES):
        check_read_info(name, IMAGES[name])
    st, info, blocks = _table(IMAGES["wavpack-combo.wv"])
    assert (info.sample_rate, info.bits_per_sample, info.channels, info.channel_mask,
            info.total_pcm_frames, info.n_sets) == (44100, 16, 2, 3, 44200, 3)
    assert bytes(info.md5).hex() == G["images"]["wavpack-combo.wv"]["md5"]
    assert [b.block_samples for b in blocks] == [22050, 11075, 11075]
    st, info, blocks = _table(IMAGES["silence.wv"])
    assert (info.total_pcm_frames, info.n_sets, info.has_md5) == (220500, 10, 0)
    st, info, _ = _table(IMAGES["rate12345_c3"])
    assert (info.sample_rate, info.channels, info.channel_mask) == (12345, 3, 7)
    st, info, _ = _table(IMAGES["chan6"])
    assert (info.channels, info.channel_mask) == (6, 0x3F)


def test_read_info_damaged_headers_and_cuts():
    """status for status: every recorded flip in the dense header region and
    every recorded cut, and the rest thinned"""
    rows = damage()
    picked = [r for r in rows if " cut " in r[0]] + \
        [r for r in rows if " flip " in r[0]][:cases.DENSE_BYTES * 8] + rows[::5]
    for label, img, status, nbytes, md5, flagged in picked:
        check_read_info(label, img)
        st, info, _ = _table(img)
        if st:
            assert status == st and nbytes == 0, label
        elif flagged:
            assert info.end_status == port.INCONSISTENT_BLOCK, label


def test_read_info_initialisation_statuses():
    img = IMAGES["chan3"]
    assert _table(img[:31])[0] == port.IO_ERROR
    assert _table(b"xvpk" + img[4:])[0] == port.INVALID_BLOCK_ID
    d = bytearray(img)
    d[27] |= 0x80
    assert _table(bytes(d))[0] == port.INVALID_RESERVED_BIT
    # a first block that is not final and carries no channel info
    st, info, blocks = _table(IMAGES["tone_c2_b16"])
    d = bytearray(IMAGES["tone_c2_b16"])
    d[25] &= ~0x10 & 0xFF
    assert _table(bytes(d))[0] == port.CHANNELS_UNDEFINED
    # rate code 15 without a sample-rate sub-block
    d = bytearray(IMAGES["tone_c2_b16"])
    d[26] |= 0x80
    d[27] |= 0x07
    assert _table(bytes(d))[0] == port.SAMPLE_RATE_UNDEFINED


def test_layout_checks():
    """the four layout checks end the table before the set they refuse"""
    img = IMAGES[cases.DAMAGE_3CH]
    st, info, blocks = _table(img)
    assert st == 0 and info.n_sets == 2 and info.end_status == 0
    second = blocks[2].offset                   # first block of the second set

    def patched(offset, value):
        d = bytearray(img)
        d[offset:offset + 4] = value.to_bytes(4, "little")
        return bytes(d)
    for label, bad in (
            ("block_index does not continue", patched(second + 16, 199)),
            ("more samples than are left", patched(second + 20, 201)),
            ("blocks disagree on block_samples", patched(blocks[3].offset + 20, 199)),
            ("final block too early", patched(second + 24, blocks[2].flags | (1 << 12)))):
        st, info, _ = _table(bad)
        assert st == 0 and info.n_sets == 1 and info.tail_blocks == 0, label
        assert info.end_status == port.INCONSISTENT_BLOCK, label


def test_hostile_headers_are_refused_by_the_reader():
    """the reader hands the decoder no table that the decoder would turn
    down: 0 channels is not opened, a block of 2^31 frames ends the table"""
    (l0, zero), (l1, big) = cases.hostile_images(IMAGES)
    check_read_info(l0, zero)
    assert _table(zero)[0] == port.CHANNELS_UNDEFINED
    assert port.decode(zero)[0] == port.CHANNELS_UNDEFINED
    check_read_info(l1, big)
    st, info, _ = _table(big)
    assert (st, info.n_sets, info.n_blocks, info.end_status) == \
        (0, 0, 0, port.INCONSISTENT_BLOCK)
    assert port.decode(big)[0] == port.INCONSISTENT_BLOCK and port.decode(big)[2] == []


@pytest.mark.skipif(not os.path.exists(WVDEC), reason="oracle/_ref/wvdec not built")
def test_live_reference(tmp_path):
    for name in ("wavpack-combo.wv", "chan6", "wasted5_c2_dupbits", "impulse_c2_b24"):
        p = tmp_path / "x.wv"
        p.write_bytes(IMAGES[name])
        r = subprocess.run([WVDEC, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        st, raw = outcome(IMAGES[name])
        assert r.returncode == 0 and st == 0 and r.stdout == raw, name
