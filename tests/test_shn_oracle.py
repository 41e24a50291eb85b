"""CPU: tests/shn_port.py, the checker the GPU Shorten codec is held to,
against the record of the reference's shnenc and shndec
(tests/golden/shn_vectors.json) and, where oracle/_ref has them, against the
tools themselves; libatgpu's host-side atg_shn_read_info against the port;
and the ABI checks of the two Shorten handles."""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import shn_cases
import shn_port
from audiotools import _atgpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = json.load(open(os.path.join(HERE, "golden", "shn_vectors.json")))
SHNENC = os.path.join(ROOT, "oracle", "_ref", "shnenc")
SHNDEC = os.path.join(ROOT, "oracle", "_ref", "shndec")
have_ref = pytest.mark.skipif(not (os.path.exists(SHNENC) and os.path.exists(SHNDEC)),
                              reason="oracle/_ref/shnenc and shndec are not built")


def fixture(name):
    with open(os.path.join(HERE, "golden", "fixtures", name), "rb") as f:
        return f.read()


def as_shndec(image):
    status, pcm, info, _, _ = shn_port.decode(image)
    raw = shn_cases.pcm_bytes(pcm, info["bits_per_sample"]) if info else b""
    return status, 0 if status == shn_port.END_OF_STREAM else 1, raw


def test_port_reproduces_encoder_vectors():
    cases = shn_cases.encoder_cases()
    assert set(c[0] for c in cases) == set(G["encoder"])
    for name, ch, bps, block, x, header, footer in cases:
        img = shn_port.encode(x, ch, bps, block, False, True, header, footer)
        assert len(img) % 4 == 1, name
        assert len(img) == G["encoder"][name]["bytes"], name
        assert hashlib.sha256(img).hexdigest() == G["encoder"][name]["sha256"], name


def test_port_reproduces_decoder_vectors():
    todo = [("enc:" + c[0], shn_port.encode(c[4], c[1], c[2], c[3], False, True, c[5], c[6]))
            for c in shn_cases.encoder_cases()]
    todo += [("port:" + c[0], shn_port.encode(c[4], c[1], c[2], c[3], c[7], c[8], c[5], c[6],
                                              c[9])) for c in shn_cases.port_cases()]
    todo += [(n, fixture(n)) for n in shn_cases.FIXTURES]
    todo += [("built:" + n, d) for n, d in shn_cases.builder_streams().items()]
    assert set(t[0] for t in todo) == set(G["decoder"])
    for name, img in todo:
        _, rc, raw = as_shndec(img)
        v = G["decoder"][name]
        assert rc == v["returncode"], name
        assert len(raw) == v["bytes"] and hashlib.md5(raw).hexdigest() == v["md5"], name


def test_port_round_trips_its_own_files():
    for c in shn_cases.port_cases():
        img = shn_port.encode(c[4], c[1], c[2], c[3], c[7], c[8], c[5], c[6], c[9])
        status, pcm, info, head, foot = shn_port.decode(img)
        assert status == shn_port.END_OF_STREAM and np.array_equal(pcm, c[4]), c[0]
        assert (head, foot) == (c[5], c[6]), c[0]
        assert info["file_type"] == shn_port.file_type(c[2], c[7], c[8])


def test_short_mid_stream_blocks_do_not_round_trip():
    """the two history rules: the encoder's accumulates, the decoder's is the
    last block alone, so a mid-stream block shorter than 3 breaks the chain
    (shnenc -B 1 and -B 2 files do not decode to their source with shndec)"""
    # smooth and odd throughout: DIFF3 wins the early blocks and nothing shifts
    x = (np.arange(40, dtype=np.int32) ** 2) * 2 + 1
    for block, same in ((1, False), (2, False), (3, True)):
        pcm = shn_port.decode(shn_port.encode(x, 1, 16, block))[1]
        assert np.array_equal(pcm, x) == same, block


def test_port_on_damaged_fixtures():
    """every truncation, and every single-bit flip that is not set aside"""
    c = G["counts"]
    assert c["flips"] == 2480 and c["set_aside"] * 20 <= c["flips"]
    assert c["set_aside"] == c["reference_died"] + c["reference_limits"] + \
        c["limits_only"] + c["reference_overflow"]
    for n in shn_cases.FIXTURES:
        img, rec = fixture(n), G["damaged"][n]
        for k in range(len(img)):
            _, rc, raw = as_shndec(img[:k])
            assert [rc, hashlib.md5(raw).hexdigest()[:16], len(raw)] == rec["truncations"][k]
        for bit in range(8 * len(img)):
            b = bytearray(img)
            b[bit >> 3] ^= 0x80 >> (bit & 7)
            status, rc, raw = as_shndec(bytes(b))
            aside = rec["set_aside"].get(str(bit))
            if aside == "limits":
                assert status == shn_port.UNSUPPORTED, (n, bit)
            if aside is None:
                assert [rc, hashlib.md5(raw).hexdigest()[:16], len(raw)] == rec["flips"][bit], \
                    (n, bit)


def test_limits_refused_by_port():
    for name, img in shn_cases.unsupported_streams().items():
        assert shn_port.decode(img)[0] == shn_port.UNSUPPORTED, name


# ------------------------------------------------------------- read_info
def info_dict(info):
    return {k: getattr(info, k) for k, _ in info._fields_}


def check_read_info(img):
    st, info = _atgpu.shn_read_info(img)
    wst, winfo = shn_port.read_info(img)
    assert st == wst
    if wst == shn_port.OK:
        assert info_dict(info) == winfo
    return st, info


def aiff_header(channels, rate_bytes, n_frames):
    comm = struct.pack(">HIH", channels, n_frames, 16) + rate_bytes
    ssnd = 8 + n_frames * channels * 2
    body = b"AIFF" + b"COMM" + struct.pack(">I", 18) + comm + b"SSND" + \
        struct.pack(">III", ssnd, 0, 0)
    return b"FORM" + struct.pack(">I", len(body) + ssnd - 8) + body


RATE_48000 = b"\x40\x0e\xbb\x80\x00\x00\x00\x00\x00\x00"


def extensible_header(channels, mask, n_bytes):
    fmt = struct.pack("<HHIIHH", 0xFFFE, channels, 96000, 96000 * channels * 2, channels * 2,
                      16) + struct.pack("<HHI", 22, 16, mask) + shn_port.SUBFORMAT_PCM
    return (b"RIFF" + struct.pack("<I", 20 + len(fmt) + n_bytes) + b"WAVE" + b"LIST" +
            struct.pack("<I", 3) + b"odd\x00" + b"fmt " + struct.pack("<I", len(fmt)) + fmt +
            b"data" + struct.pack("<I", n_bytes))


def test_read_info_fixtures_and_headers():
    for n in shn_cases.FIXTURES:
        st, info = check_read_info(fixture(n))
        assert st == 0 and (info.sample_rate, info.channel_mask, info.total_pcm_frames) == \
            (44100, 0x4, 100)
    x = np.arange(40, dtype=np.int32)
    for ch, header, want in (
            (2, shn_cases.wave_header(80), (44100, 0x3, 20)),
            (4, extensible_header(4, 0x33, 80), (96000, 0x33, 10)),
            (2, aiff_header(2, RATE_48000, 20), (48000, 0x3, 20)),
            (1, aiff_header(1, RATE_48000, 40), (48000, 0x4, 40)),
            (2, b"not a header at all", (44100, 0, 0)),
            (2, b"", (44100, 0, 0)),
            (2, shn_cases.wave_header(80)[:30], (44100, 0, 0))):
        img = shn_port.encode(x, ch, 16, 256, header[:4] == b"FORM", True, header)
        st, info = check_read_info(img)
        assert st == 0 and (info.sample_rate, info.channel_mask, info.total_pcm_frames) == want
        assert info.channels == ch and info.block_length == 256
    # no VERBATIM in front
    img = shn_port.Builder(2, 3, 7, 2, 1, 5).diff(1, 1, [0] * 7).quit()
    st, info = check_read_info(img)
    assert st == 0 and (info.bits_per_sample, info.signed_samples, info.bytes_to_skip) == (8, 0, 5)


def test_read_info_every_truncation_of_a_header():
    img = shn_port.encode(np.arange(8), 2, 16, 256, False, True, shn_cases.wave_header(16))
    first_audio = shn_port.read_info(img)[1]["first_command_bit"] // 8 + 50
    seen = set()
    for k in range(first_audio + 8):
        seen.add(check_read_info(img[:k])[0])
    assert seen == {shn_port.IOERROR, shn_port.OK}
    for n in shn_cases.FIXTURES:
        for k in range(0, 40):
            check_read_info(fixture(n)[:k])


def test_read_info_refusals():
    img = fixture("shorten-frames.shn")
    assert check_read_info(b"ajkx" + img[4:])[0] == shn_port.INVALID_MAGIC_NUMBER
    assert check_read_info(img[:4] + b"\x01" + img[5:])[0] == shn_port.INVALID_SHORTEN_VERSION
    for ftype in (0, 7):
        bad = shn_port.Builder(ftype, 1, 4).diff(1, 1, [0] * 4).quit()
        assert check_read_info(bad)[0] == shn_port.UNSUPPORTED_FILE_TYPE
    for ftype in range(1, 7):
        ok = shn_port.Builder(ftype, 1, 4).diff(1, 1, [0] * 4).quit()
        assert check_read_info(ok)[0] == shn_port.OK
    lib = _atgpu.load_library()
    assert lib.atg_shn_read_info(None, 0, None) == shn_port.IOERROR


# ------------------------------------------------------- the reference, live
def run_shndec(image, tmp_path):
    p = tmp_path / "d.shn"
    p.write_bytes(image)
    r = subprocess.run([SHNDEC, str(p)], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                       timeout=20)
    return r.returncode, r.stdout


@have_ref
def test_live_shnenc_matches_port(tmp_path):
    for name, ch, bps, block, x, header, footer in shn_cases.encoder_cases()[::5]:
        out = tmp_path / "e.shn"
        cmd = [SHNENC, "-c", str(ch), "-b", str(bps), "-B", str(block)]
        for flag, data in (("-H", header), ("-F", footer)):
            if data:
                (tmp_path / flag).write_bytes(data)
                cmd += [flag, str(tmp_path / flag)]
        subprocess.run(cmd + [str(out)], input=shn_cases.pcm_bytes(x, bps),
                       stdout=subprocess.DEVNULL, check=True, timeout=20)
        assert out.read_bytes() == shn_port.encode(x, ch, bps, block, False, True, header,
                                                   footer), name


@have_ref
def test_live_shndec_decodes_port_files(tmp_path):
    """unsigned and big-endian types and explicit frame sizes, which shnenc
    cannot write, and the builder's streams"""
    for c in shn_cases.port_cases():
        img = shn_port.encode(c[4], c[1], c[2], c[3], c[7], c[8], c[5], c[6], c[9])
        assert run_shndec(img, tmp_path) == (0, shn_cases.pcm_bytes(c[4], c[2])), c[0]
    for name, img in shn_cases.builder_streams().items():
        _, rc, raw = as_shndec(img)
        assert run_shndec(img, tmp_path) == (rc, raw), name


# ------------------------------------------------------------------- the ABI
HANDLES = [(_atgpu.ShnEncoder, "atg_shn_encoder", "atg_shn_encoder_last_error"),
           (_atgpu.ShnDecoder, "atg_shn_decoder", "atg_shn_decoder_last_error")]
OTHERS = ["atg_last_error", "atg_decoder_last_error", "atg_alac_last_error",
          "atg_alac_decoder_last_error", "atg_tta_last_error", "atg_tta_decoder_last_error",
          "atg_wv_decoder_last_error", "atg_wv_encoder_last_error"]


def gpu_visible():
    return os.path.exists("/dev/kfd") and os.environ.get("HIP_VISIBLE_DEVICES", "x") != ""


@pytest.mark.skipif(gpu_visible(), reason="a GPU is visible: covered by -m gpu tests")
@pytest.mark.parametrize("cls", [h[0] for h in HANDLES], ids=lambda c: c.__name__)
def test_handle_create_fails_loudly_without_gpu(cls):
    with pytest.raises(_atgpu.ATGError) as e:
        cls(0)
    assert e.value.status == _atgpu.ATG_ERR_DEVICE
    assert e.value.args[0] and str(e.value)


@pytest.mark.skipif(gpu_visible(), reason="a GPU is visible: covered by -m gpu tests")
def test_error_slots_stay_separate():
    """a failed Shorten create writes that component's slot and no other's"""
    lib = _atgpu.load_library()
    for cls, _, own in HANDLES:
        names = OTHERS + [h[2] for h in HANDLES if h[2] != own]
        before = {err: getattr(lib, err)() for err in names}
        with pytest.raises(_atgpu.ATGError):
            cls(0)
        assert getattr(lib, own)()
        assert {err: getattr(lib, err)() for err in names} == before


@pytest.mark.parametrize("prefix", [h[1] for h in HANDLES])
def test_handle_null_arguments(prefix):
    lib = _atgpu.load_library()
    assert getattr(lib, prefix + "_create")(0, None) == _atgpu.ATG_ERR_INVALID
    getattr(lib, prefix + "_destroy")(None)  # no-op
    assert getattr(lib, prefix + "_kernel_times")(None, None, None, 0) == 0
    assert lib.atg_shn_decoder_set_index_walk(None, 1) == _atgpu.ATG_ERR_INVALID
    assert lib.atg_shn_decode_fetch(None, None, 0) == _atgpu.ATG_ERR_INVALID
    assert lib.atg_shn_decode_fetch_verbatim(None, None, 0) == _atgpu.ATG_ERR_INVALID
    assert lib.atg_shn_decode_fetch_blocks(None, 0, None, 0, None) == _atgpu.ATG_ERR_INVALID
    assert lib.atg_shn_encode_host(None, None, 0, None, None, 0, 2, 16, None, None, 0, None,
                                   None) == _atgpu.ATG_ERR_INVALID
    assert lib.atg_shn_decode_host(None, None, 0, None, 0, None, None) == _atgpu.ATG_ERR_INVALID
