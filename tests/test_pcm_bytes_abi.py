"""CPU: the packed-PCM entry points' argument checks, all made before any GPU
call (so they run without one), and libatgpu's AIFF / Sun AU header parsers
against the Python walkers over every truncation and every single-byte
change of a file of each kind."""
import ctypes
import os

import numpy as np
import pytest

import bad_device
from audiotools import _atgpu, aiff, au

HERE = os.path.dirname(os.path.abspath(__file__))
AIFF_2CH = os.path.join(HERE, "golden", "fixtures", "aiff-2ch.aiff")


def _buf(nbytes, shift=0):
    """a host buffer whose address is 16-byte aligned plus `shift`"""
    a = np.zeros(nbytes + 32, dtype=np.uint8)
    off = (-a.ctypes.data) % 16 + shift
    return a[off:off + nbytes]


def _call(which, layout=(2, True, True), fmt=_atgpu.PCM_S32, runs=((0, 8, 0),), bytes_cap=64,
          pcm_cap=64, d_bytes="buf", d_pcm="buf", n_runs=None, null_runs=False, shift_bytes=0,
          shift_pcm=0):
    """the device entry with host pointers: every case here is refused (or is
    empty) before the pointers are used"""
    lib = _atgpu.load_library()
    keep_b, keep_p = _buf(256, shift_bytes), _buf(1024, shift_pcm)
    pb = keep_b.ctypes.data if d_bytes == "buf" else None
    pp = keep_p.ctypes.data if d_pcm == "buf" else None
    arr, n = _atgpu.pcm_runs(runs)
    n = n if n_runs is None else n_runs
    lay = _atgpu.pcm_layout(*layout)
    ra = None if null_runs else arr
    if which == "unpack":
        return lib.atg_pcm_unpack_device(pb, bytes_cap, lay, ra, n, pp, fmt, pcm_cap, None)
    return lib.atg_pcm_pack_device(pp, fmt, pcm_cap, lay, ra, n, pb, bytes_cap, None)


BOTH = ["unpack", "pack"]


@pytest.mark.parametrize("which", BOTH)
def test_invalid_arguments(which):
    inv = _atgpu.ATG_ERR_INVALID
    lib = _atgpu.load_library()
    assert _call(which, d_bytes=None) == inv
    assert lib.atg_pcm_bytes_last_error()
    assert _call(which, d_pcm=None) == inv
    assert _call(which, null_runs=True) == inv
    assert _call(which, layout=(0, True, True)) == inv
    assert _call(which, layout=(4, True, True)) == inv
    assert _call(which, layout=(3, True, True), fmt=_atgpu.PCM_S16) == inv
    assert _call(which, fmt=2) == inv
    assert _call(which, fmt=-1) == inv
    assert _call(which, shift_bytes=4) == inv          # packed buffer off a 16-byte boundary
    assert _call(which, shift_pcm=2) == inv            # integer buffer off its boundary
    # the format and layout are checked even with nothing to do
    assert _call(which, layout=(5, False, False), runs=()) == inv
    assert _call(which, fmt=7, runs=()) == inv


def test_unpack_alignment_rules():
    inv = _atgpu.ATG_ERR_INVALID
    assert _call("unpack", bytes_cap=60) == inv                      # capacity not whole units
    assert _call("unpack", shift_pcm=4) == inv                       # d_pcm needs 16 bytes
    assert _call("unpack", runs=((0, 8, 2),)) == inv                 # int32: multiples of 4
    assert _call("unpack", runs=((0, 8, 4),), fmt=_atgpu.PCM_S16) == inv   # int16: of 8
    assert _call("unpack", runs=((0, 0, 3),)) == _atgpu.ATG_OK       # an empty run is not placed
    # pack takes any sample_offset and any capacity, and int32 on 4 bytes
    assert _call("pack", runs=((0, 0, 3),), bytes_cap=61, shift_pcm=4) == _atgpu.ATG_OK


@pytest.mark.parametrize("which", BOTH)
def test_capacity(which):
    cap = _atgpu.ATG_ERR_CAPACITY
    assert _call(which, runs=((0, 33, 0),), bytes_cap=64, pcm_cap=64) == cap      # 66 bytes
    assert _call(which, runs=((63, 1, 0),), bytes_cap=64) == cap
    assert _call(which, runs=((80, 0, 0),), bytes_cap=64) == cap
    assert _call(which, runs=((0, 8, 60),), pcm_cap=64) == cap
    assert _call(which, runs=((0, 0, 68),), pcm_cap=64) == cap
    assert _call(which, runs=((0, 0, 0), (0, 1 << 63, 0))) == cap                  # no overflow
    assert _call(which, runs=((0, 4, 0), ((1 << 64) - 2, 4, 0))) == cap
    assert _call(which, runs=((0, 4, (1 << 64) - 4),)) == cap
    assert _atgpu.load_library().atg_pcm_bytes_last_error()


@pytest.mark.parametrize("which", BOTH)
def test_nothing_to_do_is_ok(which):
    assert _call(which, runs=()) == _atgpu.ATG_OK
    assert _call(which, runs=(), d_bytes=None, d_pcm=None, null_runs=True) == _atgpu.ATG_OK
    assert _call(which, runs=((0, 0, 0), (64, 0, 64), (7, 0, 8))) == _atgpu.ATG_OK


def test_host_entries_check_before_staging():
    lib = _atgpu.load_library()
    arr, n = _atgpu.pcm_runs([(0, 8, 0)])
    b, p = _buf(16), _buf(64)
    lay = _atgpu.pcm_layout(3, True, True)
    assert lib.atg_pcm_unpack_host(0, b.ctypes.data, 16, lay, arr, n, p.ctypes.data,
                                   _atgpu.PCM_S32, 16) == _atgpu.ATG_ERR_CAPACITY   # 24 bytes
    assert lib.atg_pcm_pack_host(0, p.ctypes.data, _atgpu.PCM_S16, 16, lay, arr, n,
                                 b.ctypes.data, 16) == _atgpu.ATG_ERR_INVALID
    assert lib.atg_pcm_unpack_host(0, None, 0, lay, None, 0, None, _atgpu.PCM_S32,
                                   0) == _atgpu.ATG_OK
    assert _atgpu.pcm_bytes_tile_samples() % 8 == 0
    assert lib.atg_pcm_bytes_kernel_times(None, None, 0) == 0


def test_host_entries_refuse_device_minus_1():
    lib = _atgpu.load_library()
    arr, n = _atgpu.pcm_runs([(0, 8, 0)])
    b, p = _buf(16), _buf(64)
    lay = _atgpu.pcm_layout(2, True, True)
    bad_device.check_refused(lib.atg_pcm_unpack_host(
        -1, b.ctypes.data, 16, lay, arr, n, p.ctypes.data, _atgpu.PCM_S32, 16), "pcm_bytes")
    bad_device.check_refused(lib.atg_pcm_pack_host(
        -1, p.ctypes.data, _atgpu.PCM_S16, 16, lay, arr, n, b.ctypes.data, 16), "pcm_bytes")
    # nothing to do comes first: no device is asked for
    assert lib.atg_pcm_unpack_host(-1, None, 0, lay, None, 0, None, _atgpu.PCM_S32,
                                   0) == _atgpu.ATG_OK


# ------------------------------------------------------------------ parsers
def variants(image):
    for cut in range(len(image) + 1):
        yield image[:cut]
    for i in range(len(image)):
        for v in (0x00, 0xFF, (image[i] + 1) & 0xFF, image[i] ^ 0x80, 0x20, 0x7E):
            if v != image[i]:
                yield image[:i] + bytes([v]) + image[i + 1:]


AIFF_STATUS = {"not an AIFF file": _atgpu.AIFF_NOT_AIFF,
               "invalid AIFF file": _atgpu.AIFF_INVALID_AIFF,
               "invalid AIFF chunk ID": _atgpu.AIFF_INVALID_CHUNK_ID,
               "invalid AIFF chunk": _atgpu.AIFF_INVALID_CHUNK,
               "SSND chunk found before fmt": _atgpu.AIFF_PREMATURE_SSND,
               "SSND chunk not found": _atgpu.AIFF_NO_SSND}


def aiff_walk(path, image):
    """(status, reader fields) of the Python walker, with the C parser's
    support rule applied to what it parsed"""
    with open(path, "wb") as f:
        f.write(image)
    try:
        r = aiff.AiffReader(path)
    except IOError:
        return _atgpu.AIFF_IOERROR, None
    except (ValueError, aiff.InvalidAIFF) as err:
        return AIFF_STATUS[str(err)], None
    r.close()
    fields = (r.channels, r.total_pcm_frames, r.bits_per_sample, r.sample_rate, r.channel_mask,
              r.ssnd_chunk_offset)
    if r.bits_per_sample not in (8, 16, 24) or not 0 <= r.sample_rate < (1 << 32):
        return _atgpu.ATG_ERR_UNSUPPORTED, fields
    return _atgpu.AIFF_OK, fields


@pytest.mark.parametrize("name", ["aiff-2ch", "aiff-misordered"])
def test_aiff_parser_against_the_python_walker(tmp_path, name):
    image = open(AIFF_2CH.replace("aiff-2ch", name), "rb").read()
    path = str(tmp_path / "v.aiff")
    seen = set()
    for v in variants(image):
        want, fields = aiff_walk(path, v)
        st, info = _atgpu.aiff_read_info(v)
        assert st == want, (len(v), v[:64])
        assert info.ssnd_data_offset + info.ssnd_data_bytes <= len(v)
        if fields is not None:
            assert (info.channels, info.total_pcm_frames, info.bits_per_sample,
                    info.sample_rate if st == 0 else fields[3], info.channel_mask,
                    info.ssnd_data_offset) == fields
        seen.add(st)
    assert seen >= {0, _atgpu.AIFF_NOT_AIFF, _atgpu.AIFF_INVALID_AIFF,
                    _atgpu.AIFF_INVALID_CHUNK_ID, _atgpu.AIFF_NO_SSND, _atgpu.AIFF_IOERROR,
                    _atgpu.ATG_ERR_UNSUPPORTED}
    lib = _atgpu.load_library()
    assert lib.atg_aiff_read_info(None, 0, None) == _atgpu.ATG_ERR_INVALID
    assert lib.atg_aiff_read_info(None, 5, ctypes.byref(_atgpu.AiffInfo())) == _atgpu.ATG_ERR_INVALID


def test_aiff_parser_other_statuses():
    """the two statuses one changed byte of aiff-2ch.aiff does not reach"""
    image = open(AIFF_2CH, "rb").read()
    comm, ssnd = image[12:38], image[38:]
    only_ssnd = b"FORM" + (len(ssnd) + 4).to_bytes(4, "big") + b"AIFF" + ssnd
    assert _atgpu.aiff_read_info(only_ssnd)[0] == _atgpu.AIFF_PREMATURE_SSND
    # SSND first, COMM after it: the sound data met first is reported
    st, info = _atgpu.aiff_read_info(image[:12] + ssnd + comm)
    assert st == 0 and (info.ssnd_data_offset, info.ssnd_data_bytes, info.channels) == (28, 80, 2)
    odd = b"NAME\x00\x00\x00\x03abc"
    assert _atgpu.aiff_read_info(image[:12] + comm + odd)[0] == _atgpu.AIFF_INVALID_CHUNK
    st, info = _atgpu.aiff_read_info(image[:12] + comm + odd + b"\0" + ssnd)
    assert st == 0 and info.ssnd_data_offset == 54 + 12 and info.ssnd_data_bytes == 80
    # the 80-bit rate: infinity, a negative rate and 2^32 do not fit; 2^32 - 1 does
    for rate, want in ((bytes.fromhex("7FFF0000000000000000"), _atgpu.ATG_ERR_UNSUPPORTED),
                       (bytes.fromhex("C00EAC44000000000000"), _atgpu.ATG_ERR_UNSUPPORTED),
                       (aiff.build_ieee_extended(float(1 << 32)), _atgpu.ATG_ERR_UNSUPPORTED),
                       (aiff.build_ieee_extended(float((1 << 32) - 1)), 0),
                       (bytes.fromhex("3FFE8000000000000000"), 0)):          # 0.5 -> 0
        st, info = _atgpu.aiff_read_info(image[:28] + rate + image[38:])
        assert st == want
        if st == 0:
            assert info.sample_rate == int(aiff.parse_ieee_extended(rate))


def au_walk(path, image):
    with open(path, "wb") as f:
        f.write(image)
    try:
        r = au.AuReader(path)
    except IOError:
        return _atgpu.AU_IOERROR, None
    except ZeroDivisionError:
        return _atgpu.ATG_ERR_UNSUPPORTED, None
    except ValueError as err:
        return {"invalid Sun AU header": _atgpu.AU_INVALID_HEADER,
                "unsupported Sun AU format": _atgpu.AU_UNSUPPORTED_FORMAT}[str(err)], None
    r.close()
    return _atgpu.AU_OK, (r.channels, r.bits_per_sample, r.sample_rate, r.channel_mask,
                          r.total_pcm_frames, r.data_offset)


def test_au_parser_against_the_python_walker(tmp_path):
    image = (b".snd" + (28).to_bytes(4, "big") + (12).to_bytes(4, "big") + (3).to_bytes(4, "big") +
             (44100).to_bytes(4, "big") + (2).to_bytes(4, "big") + b"note" + bytes(range(12)))
    assert len(image) == 40
    path = str(tmp_path / "v.au")
    seen = set()
    for v in variants(image):
        want, fields = au_walk(path, v)
        st, info = _atgpu.au_read_info(v)
        assert st == want, (len(v), v[:24])
        if fields is not None:
            assert (info.channels, info.bits_per_sample, info.sample_rate, info.channel_mask,
                    info.total_pcm_frames, info.data_offset) == fields
            assert info.data_bytes == min(info.data_size, max(0, len(v) - info.data_offset))
        seen.add(st)
    assert seen == {0, _atgpu.AU_INVALID_HEADER, _atgpu.AU_UNSUPPORTED_FORMAT, _atgpu.AU_IOERROR,
                    _atgpu.ATG_ERR_UNSUPPORTED}
    assert _atgpu.load_library().atg_au_read_info(None, 0, None) == _atgpu.ATG_ERR_INVALID
