"""CPU: the MLP port (mlp_port.py) against the reference's vectors
(golden/mlp_vectors.json), the stream writer's round trip, and the C ABI's
prototypes and argument checks."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest

import bad_device
import dvda_build
import mlp_build
import mlp_cases as cases
import mlp_port as port
from audiotools import _atgpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "mlp_vectors.json")
HEADER = os.path.join(ROOT, "include", "atgpu_mlp.h")
FIELDS = ["status", "stop_sector", "stop_unit", "access_units", "sample_rate", "bits_per_sample",
          "channels", "channel_mask", "channel_assignment", "substreams", "good_frames"]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def check_record(img, first, rec, name):
    """the port on one vector: its own recorded answer, and the reference's
    where the vector is not set aside"""
    res, x, _ = port.decode(img, first)
    p = rec["port"]         # cases.PORT_KEYS' values, clip, the samples' MD5
    assert [res[k] for k in cases.PORT_KEYS] == p[:-2], name
    assert hashlib.md5(x.astype("<i4").tobytes()).hexdigest()[:16] == p[-1], name
    if rec.get("set_aside"):
        return 0
    rc, err, md5, size = rec["ref"]
    raw, text = port.answer_from(res, x, cases.ask_pts(res))
    assert rc == 0 and text == err and len(raw) == size, name
    assert hashlib.md5(raw).hexdigest()[:16] == md5, name
    return 1


def test_port_against_the_title_vectors(golden):
    specs = cases.title_cases()
    assert sorted(s["name"] for s in specs) == sorted(golden["titles"])
    compared, statuses = 0, set()
    for s in specs:
        rec = golden["titles"][s["name"]]
        assert rec["spec"] == cases.spec_digest(s), s["name"]
        img, first = cases.image_of(s)
        compared += check_record(img, first, rec, s["name"])
        statuses.add(rec["port"][0])
    assert compared >= len(specs) - 6
    # every status but the three a title case cannot reach, each of them
    # confirmed by the reference's own message
    assert statuses == set(range(17)) - {port.NOT_MLP, port.NO_MAJOR_SYNC, port.EOF}
    res = [port.decode(*cases.image_of(s))[0]["status"] for s in cases.other_cases()]
    assert res == [port.NOT_MLP, port.NO_MAJOR_SYNC]
    assert port.decode(b"")[0]["status"] == port.EOF


@pytest.mark.parametrize("name", sorted(cases.flip_specs()))
def test_port_against_the_damage_sweeps(golden, name):
    sweep = golden["sweeps"][name]
    spec = cases.flip_specs()[name]
    assert sweep["spec"] == cases.spec_digest(spec)
    img, _ = cases.image_of(spec)
    bits = cases.flip_bits(spec)
    assert len(bits) == sweep["n_bits"] >= 3000
    assert sweep["counts"]["set_aside"] * 50 <= len(bits)
    rows = cases.unpack_flips(sweep)
    assert len(rows) == len(bits)
    # most flips still decode, to other PCM: that is what pins the arithmetic
    assert sweep["counts"]["changed_pcm"] >= len(bits) // 2
    compared = 0
    for k, bit in enumerate(bits):
        # the digest covers the result, the samples and, for flag "p", the
        # reference's stderr and PCM bytes (cases.outcome)
        flag = rows[k][0]
        res, x, _ = port.decode(dvda_build.flip(img, bit))
        answer = port.answer_from(res, x, cases.ask_pts(res)) if flag == "p" else None
        assert cases.outcome(res, x, flag, answer) == rows[k], (name, bit)
        compared += flag == "p"
    assert sum(r[0] == "a" for r in rows) == sweep["counts"]["set_aside"]
    assert compared >= len(bits) * 0.95


def test_builder_round_trip():
    """the signal the writer chose comes back out of the port"""
    for s in cases.title_cases():
        if s["plan"] not in ("plain", "filters", "fir-restart", "codebooks") or s.get("bad") or \
                s.get("partial") or s.get("bad_sector") is not None:
            continue
        title, stream = cases.expand(s)
        img, first = cases.image_of(s)
        res, x, units = port.decode(img, first)
        assert res["status"] == port.OK and len(units) == s["units"], s["name"]
        assert res["good_frames"] == s["units"] * s["frames"], s["name"]
        ch = res["channels"]
        full = res["full"].reshape(-1, ch)
        for k, (lo, hi, _) in enumerate(cases.ranges(s)):
            for c in range(lo, hi + 1):
                want = title["signal"][k][c]
                wave = port.WAVE_CHANNEL[res["channel_assignment"]][c]
                assert list(full[:, wave]) == want, (s["name"], c)
    # the codebooks of the writer and the reader are each other's inverse
    for k in (1, 2, 3):
        codes = port.codebook(k)
        assert len(codes) == {1: 20, 2: 18, 3: 17}[k]
        for bits_, value in codes:
            b = port.Bits(int(bits_ + "1" * (16 - len(bits_)), 2).to_bytes(2, "big"))
            assert b.huffman(k) == value and b.pos == len(bits_)
    assert port.CRC8[:5] == [0x00, 0x63, 0xC6, 0xA5, 0xEF]


# ------------------------------------------------------------------ the ABI
def prototypes():
    from test_signatures import c_kind
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    out = {}
    for result, name, args in re.findall(
            r"([A-Za-z_][\w\s\*]*?)\b(atg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        args = " ".join(args.split())
        out[name] = (c_kind(result, False),
                     [] if args == "void" else [c_kind(a, True) for a in args.split(",")])
    return out


def test_signature_table_agrees_with_the_header():
    from test_signatures import ctypes_kind
    protos = prototypes()
    assert sorted(protos) == sorted(_atgpu.MLP_SIGNATURES) and len(protos) == 5
    lib = _atgpu.load_library()
    for name, (result, params) in protos.items():
        restype, argtypes = _atgpu.MLP_SIGNATURES[name]
        assert (ctypes_kind(restype), [ctypes_kind(t) for t in argtypes]) == (result, params), name
        assert getattr(lib, name).argtypes is not None or not params
    assert not set(protos) & (set(_atgpu.SIGNATURES) | set(_atgpu.DVDA_SIGNATURES))
    assert ctypes.sizeof(_atgpu.MlpResult) == 56 and ctypes.sizeof(_atgpu.MlpUnit) == 32
    text = open(HEADER).read()
    assert int(re.search(r"ATG_MLP_MAX_UNIT_FRAMES (\d+)u", text).group(1)) == \
        _atgpu.MLP_MAX_UNIT_FRAMES == port.MAX_UNIT_FRAMES
    names = re.findall(r"\bATG_MLP_([A-Z0-9_]+) = (\d+)", text)
    assert [int(v) for _, v in names] == list(range(17))
    for n, v in names:
        assert getattr(_atgpu, "MLP_" + n) == int(v) == getattr(port, n, int(v))


def test_argument_checks_need_no_device():
    lib = _atgpu.load_library()
    res = (_atgpu.MlpResult * 2)()
    total = ctypes.c_uint64(7)
    buf = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(buf) + 15) & ~15

    def scan(ptr, cap, titles, fmt=_atgpu.PCM_S32, results=res, n=None):
        arr, k = _atgpu.aob_titles(titles)
        return lib.atg_mlp_scan_device(ctypes.c_void_p(ptr), cap, arr, k if n is None else n, fmt,
                                       results, ctypes.byref(total), None, 0, None)

    def decode(ptr, cap, titles, pcm, fmt=_atgpu.PCM_S32):
        arr, k = _atgpu.aob_titles(titles)
        return lib.atg_mlp_decode_device(ctypes.c_void_p(ptr), cap, arr, k, ctypes.c_void_p(pcm),
                                         fmt, 1 << 20, res, None)

    assert scan(None, 0, []) == _atgpu.ATG_OK and total.value == 0
    assert decode(None, 0, [], None) == _atgpu.ATG_OK
    assert lib.atg_mlp_decode_host(0, None, 0, None, 0, None, _atgpu.PCM_S32, 0, None) == \
        _atgpu.ATG_OK
    assert lib.atg_mlp_kernel_times(None, None, 10) == 0
    for call, status, words in [
            (lambda: scan(None, 4096, [(0, 2)]), _atgpu.ATG_ERR_INVALID, "NULL"),
            (lambda: scan(base, 4096, [(0, 2)], results=None), _atgpu.ATG_ERR_INVALID, "NULL"),
            (lambda: scan(base, 4096, [(0, 2)], fmt=5), _atgpu.ATG_ERR_INVALID, "format"),
            (lambda: scan(base + 4, 4096, [(0, 1)]), _atgpu.ATG_ERR_INVALID, "16-byte aligned"),
            (lambda: scan(base, 4096, [(8, 1)]), _atgpu.ATG_ERR_INVALID, "multiple of 16"),
            (lambda: scan(base, 4096, [(0, 3)]), _atgpu.ATG_ERR_CAPACITY, "bytes_cap"),
            (lambda: scan(base, 4096, [(2064, 1)]), _atgpu.ATG_ERR_CAPACITY, "bytes_cap"),
            (lambda: scan(base, 4096, [(0, (1 << 23) + 1)]), _atgpu.ATG_ERR_UNSUPPORTED,
             "ATG_AOB_MAX_TITLE_SECTORS"),
            (lambda: scan(base, (1 << 38) + 16, [(0, 1)]), _atgpu.ATG_ERR_UNSUPPORTED,
             "ATG_AOB_MAX_BATCH_BYTES"),
            (lambda: scan(base, 4096, [(0, 1)], n=(1 << 20) + 1), _atgpu.ATG_ERR_UNSUPPORTED,
             "ATG_AOB_MAX_TITLES"),
            (lambda: decode(base, 4096, [(0, 2)], None), _atgpu.ATG_ERR_INVALID, "NULL"),
            (lambda: decode(base, 4096, [(0, 2)], base + 8), _atgpu.ATG_ERR_INVALID, "d_pcm"),
            (lambda: lib.atg_mlp_decode_host(0, None, 4096, _atgpu.aob_titles([(0, 1)])[0], 1,
                                             None, _atgpu.PCM_S32, 0, res),
             _atgpu.ATG_ERR_INVALID, "NULL")]:
        assert call() == status, words
        assert words in lib.atg_mlp_last_error().decode(), words
    # a sound call on device -1: one whole sector in, room for its samples out
    sector = np.zeros(2048, dtype=np.uint8)
    pcm = np.zeros(1024, dtype=np.int32)
    bad_device.check_refused(lib.atg_mlp_decode_host(
        -1, sector.ctypes.data_as(ctypes.c_void_p), 2048, _atgpu.aob_titles([(0, 1)])[0], 1,
        pcm.ctypes.data_as(ctypes.c_void_p), _atgpu.PCM_S32, 1024, res), "mlp")
