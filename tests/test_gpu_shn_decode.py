"""GPU parity: libatgpu's Shorten decoder (shn_decode.hip) against what the
reference's shndec made of the same streams (tests/golden/shn_vectors.json:
return code, md5 and length of its output, which clamps to the sample width)
and, in full int32, against tests/shn_port.py.  Both index walks are held to
the same record."""
import hashlib
import json
import os

import numpy as np
import pytest

import shn_cases
import shn_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "shn_vectors.json")))


def fixture(name):
    with open(os.path.join(HERE, "golden", "fixtures", name), "rb") as f:
        return f.read()


def gpu_decode(images, cooperative=True):
    """-> per image (status, pcm int32, header bytes, footer bytes); a header
    error is the status atg_shn_read_info gave"""
    from audiotools import _atgpu
    dec = _atgpu.shn_decoder()
    dec.set_index_walk(cooperative)
    buf = bytearray()
    tracks, slot = [], []
    for img in images:
        st, info = _atgpu.shn_read_info(img)
        if st != _atgpu.SHN_OK:
            slot.append(st)
            continue
        while len(buf) % 4:
            buf.append(0)
        slot.append(None)
        tracks.append(_atgpu.shn_dec_track(len(buf), len(img), info))
        buf += img
    try:
        pcm, res, verb = dec.decode(bytes(buf), tracks)
    finally:
        dec.set_index_walk(True)
    out, k = [], 0
    for s in slot:
        if s is not None:
            out.append((s, np.zeros(0, np.int32), b"", b""))
            continue
        r, t = res[k], tracks[k]
        k += 1
        v = verb[r.verbatim_offset:r.verbatim_offset + r.header_bytes + r.footer_bytes].tobytes()
        out.append((r.status, pcm[r.pcm_offset:r.pcm_offset + r.pcm_frames * t.channels],
                    v[:r.header_bytes], v[r.header_bytes:]))
    return out


_PORT = {}


def port_decode(img):
    """shn_port's answer, computed once per image"""
    if img not in _PORT:
        _PORT[img] = shn_port.decode(img)
    return _PORT[img]


def check_against_port(images, names, cooperative=True, verbatim=True):
    got = gpu_decode(images, cooperative)
    for name, img, (st, pcm, head, foot) in zip(names, images, got):
        wst, wpcm, _, whead, wfoot = port_decode(img)
        assert st == wst, name
        assert np.array_equal(pcm, wpcm), name
        if verbatim and wst == shn_port.END_OF_STREAM:
            assert (head, foot) == (whead, wfoot), name
    return got


def check_record(name, got, bps):
    """shndec's return code and output"""
    st, pcm = got[0], got[1]
    v = G["decoder"][name]
    assert (0 if st == shn_port.END_OF_STREAM else 1) == v["returncode"], name
    raw = shn_cases.pcm_bytes(pcm, bps)
    assert len(raw) == v["bytes"] and hashlib.md5(raw).hexdigest() == v["md5"], name


@pytest.mark.parametrize("cooperative", [True, False], ids=["cooperative", "serial"])
def test_encoder_images_round_trip(cooperative):
    """every image the encoders made decodes to its source, to shndec's
    record and with the header and footer bytes it was given"""
    cases = shn_cases.encoder_cases()
    images = [shn_port.encode(c[4], c[1], c[2], c[3], False, True, c[5], c[6]) for c in cases]
    got = check_against_port(images, [c[0] for c in cases], cooperative)
    for c, g in zip(cases, got):
        assert g[0] == shn_port.END_OF_STREAM
        assert np.array_equal(g[1], c[4]), c[0]
        assert (g[2], g[3]) == (c[5], c[6]), c[0]
        check_record("enc:" + c[0], g, c[2])


def test_port_images_round_trip():
    cases = shn_cases.port_cases()
    images = [shn_port.encode(c[4], c[1], c[2], c[3], c[7], c[8], c[5], c[6], c[9])
              for c in cases]
    got = check_against_port(images, [c[0] for c in cases])
    for c, g in zip(cases, got):
        assert np.array_equal(g[1], c[4]), c[0]
        check_record("port:" + c[0], g, c[2])


def test_gpu_encoder_to_gpu_decoder():
    from test_gpu_shn_encode import gpu_encode
    pcms = shn_cases.mixed_batch()
    images = gpu_encode(pcms, 2, 16, 256, headers=[b"hd"] * len(pcms))
    for p, g in zip(pcms, gpu_decode(images)):
        assert g[0] == shn_port.END_OF_STREAM and np.array_equal(g[1], p) and g[2] == b"hd"


@pytest.mark.parametrize("cooperative", [True, False], ids=["cooperative", "serial"])
def test_fixtures(cooperative):
    images = [fixture(n) for n in shn_cases.FIXTURES]
    got = check_against_port(images, shn_cases.FIXTURES, cooperative)
    for n, g in zip(shn_cases.FIXTURES, got):
        assert g[0] == shn_port.END_OF_STREAM and len(g[1]) == 100
        check_record(n, g, 16)


@pytest.mark.parametrize("cooperative", [True, False], ids=["cooperative", "serial"])
def test_builder_streams(cooperative):
    """DIFF0 with mean counts 1 and 4, QLPC of orders 0, 1, 3 and 8, blocks of
    1 and 2 before DIFF3 (the short-history rule), shift changes, VERBATIM
    between blocks, a 10000-bit zero run, energies 0 and 20, and the ends a
    stream can come to"""
    streams = sorted(shn_cases.builder_streams().items())
    got = check_against_port([s[1] for s in streams], [s[0] for s in streams], cooperative)
    for (name, img), g in zip(streams, got):
        check_record("built:" + name, g, shn_port.read_info(img)[1]["bits_per_sample"])
    by = dict(zip([s[0] for s in streams], got))
    assert by["no_quit"][0] == shn_port.IOERROR and len(by["no_quit"][1]) == 10
    assert by["unknown_command"][0] == shn_port.UNKNOWN_COMMAND
    assert by["incomplete_set"][0] == shn_port.END_OF_STREAM and len(by["incomplete_set"][1]) == 20
    late = by["incomplete_set_then_verbatim"]
    assert late[0] == shn_port.END_OF_STREAM and len(late[1]) == 20
    assert (late[2], late[3]) == (b"front", b"late")


def test_limits_refused():
    streams = sorted(shn_cases.unsupported_streams().items())
    for (name, img), g in zip(streams, gpu_decode([s[1] for s in streams])):
        assert g[0] == shn_port.UNSUPPORTED, name
        assert np.array_equal(g[1], port_decode(img)[1]), name


def test_many_commands_rerun_index():
    """more commands than the first guess allows for (ZERO commands are five
    bits): the index pass runs again with the count it reported"""
    b = shn_port.Builder(5, 1, 256)
    for k in range(2000):
        b.zero() if k % 50 else b.diff(1, 1, [k % 3 - 1] * 256)
    img = b.quit()
    g = check_against_port([img], ["zeros"])[0]
    assert g[0] == shn_port.END_OF_STREAM and len(g[1]) == 2000 * 256


@pytest.mark.parametrize("cooperative", [True, False], ids=["cooperative", "serial"])
def test_all_truncations_one_batch(cooperative):
    """all 310 truncations of the two fixtures"""
    images, names, want = [], [], []
    for n in shn_cases.FIXTURES:
        img = fixture(n)
        for k in range(len(img)):
            images.append(img[:k])
            names.append("%s[:%d]" % (n, k))
            want.append(G["damaged"][n]["truncations"][k])
    assert len(images) == 310
    got = check_against_port(images, names, cooperative, verbatim=False)
    for name, g, (rc, md5, nbytes) in zip(names, got, want):
        raw = shn_cases.pcm_bytes(g[1], 16)
        assert (0 if g[0] == shn_port.END_OF_STREAM else 1) == rc, name
        assert len(raw) == nbytes and hashlib.md5(raw).hexdigest()[:16] == md5, name


@pytest.mark.parametrize("cooperative", [True, False], ids=["cooperative", "serial"])
def test_all_bit_flips_one_batch(cooperative):
    """all 2,480 single-bit flips of the two fixtures: shn_port's status and
    int32 PCM on every one; shndec's record on all but those set aside, of
    which the ones only the limits refuse are ATG_SHN_UNSUPPORTED"""
    images, names, want = [], [], []
    for n in shn_cases.FIXTURES:
        img = fixture(n)
        rec = G["damaged"][n]
        for bit in range(8 * len(img)):
            b = bytearray(img)
            b[bit >> 3] ^= 0x80 >> (bit & 7)
            images.append(bytes(b))
            names.append("%s^%d" % (n, bit))
            want.append((rec["flips"][bit], rec["set_aside"].get(str(bit))))
    assert len(images) == 2480
    assert G["counts"]["set_aside"] * 20 <= 2480
    got = check_against_port(images, names, cooperative, verbatim=False)
    for name, img, g, ((rc, md5, nbytes), aside) in zip(names, images, got, want):
        if aside == "limits":
            assert g[0] == shn_port.UNSUPPORTED, name
        if aside is not None:
            continue
        info = port_decode(img)[2]
        raw = shn_cases.pcm_bytes(g[1], info["bits_per_sample"] if info else 16)
        assert (0 if g[0] == shn_port.END_OF_STREAM else 1) == rc, name
        assert len(raw) == nbytes and hashlib.md5(raw).hexdigest()[:16] == md5, name


def test_kernel_times_and_device_path():
    import torch
    from audiotools import _atgpu
    dec = _atgpu.shn_decoder()
    img = fixture("shorten-lpc.shn")
    st, info = _atgpu.shn_read_info(img)
    pad = img + b"\0" * (-len(img) % 4)
    d = torch.from_numpy(np.frombuffer(pad + pad, dtype=np.uint8).copy()).cuda()
    tracks = [_atgpu.shn_dec_track(0, len(img), info),
              _atgpu.shn_dec_track(len(pad), len(img), info)]
    res, dp, ns = dec.decode_device(d.data_ptr(), len(pad) * 2, tracks)
    assert dp and ns == 200
    pcm = dec.fetch(ns)
    want = shn_port.decode(img)[1]
    assert np.array_equal(pcm[:100], want) and np.array_equal(pcm[100:], want)
    assert list(dec.kernel_times()) == ["shnd_index", "shnd_layout", "shnd_parse", "shnd_recon",
                                        "shnd_total"]
