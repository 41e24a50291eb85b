"""CPU: the dither block of the C ABI (include/atgpu_dither.h).  Its table in
_atgpu agrees with the header, the library exports it, and every argument
check of atg_dither_fill_device comes before any GPU call: on a machine
without a GPU each refusal still gives its own status and message, with a
device pointer that is never dereferenced."""
import ctypes
import os
import threading

import pytest

import test_signatures
import audiotools
from audiotools import _atgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "atgpu_dither.h")

OK, INVALID, CAPACITY = _atgpu.ATG_OK, _atgpu.ATG_ERR_INVALID, _atgpu.ATG_ERR_CAPACITY
OUT = 0x200000  # never written

OTHER_SLOTS = sorted(n for table in (_atgpu.SIGNATURES, _atgpu.DVDA_SIGNATURES,
                                     _atgpu.MLP_SIGNATURES, _atgpu.TENSOR_SIGNATURES)
                     for n in table if n.endswith("last_error"))


def slots():
    lib = _atgpu.load_library()
    return {n: getattr(lib, n)() for n in OTHER_SLOTS}


# ------------------------------------------------------------------ the table
def test_table_agrees_with_header(monkeypatch):
    monkeypatch.setattr(test_signatures, "HEADER", HEADER)
    protos = test_signatures.prototypes()
    assert sorted(protos) == sorted(_atgpu.DITHER_SIGNATURES) and len(protos) == 4
    for name, (result, params) in protos.items():
        restype, argtypes = _atgpu.DITHER_SIGNATURES[name]
        got = (test_signatures.ctypes_kind(restype),
               [test_signatures.ctypes_kind(t) for t in argtypes])
        assert got == (result, params), name
    assert not set(protos) & (set(_atgpu.SIGNATURES) | set(_atgpu.DVDA_SIGNATURES) |
                              set(_atgpu.MLP_SIGNATURES) | set(_atgpu.TENSOR_SIGNATURES) |
                              set(_atgpu.PROBE_SIGNATURES))


def test_library_exports_the_block():
    lib = _atgpu.load_library()
    for name, (restype, argtypes) in _atgpu.DITHER_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes or ()) == tuple(argtypes), name


def test_struct_size_and_tile():
    assert ctypes.sizeof(_atgpu.DitherRun) == 32
    t = _atgpu.dither_tile_blocks()
    assert t > 0 and t % 64 == 0


def test_public_names():
    assert audiotools.DeviceDither is audiotools.pcmconverter.DeviceDither
    assert audiotools.DeviceDither(5).seed == 5
    assert audiotools.DeviceDither((1 << 64) - 1).seed == (1 << 64) - 1
    a, b = audiotools.DeviceDither(), audiotools.DeviceDither()
    assert 0 <= a.seed < 1 << 64 and a.seed != b.seed
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            audiotools.DeviceDither(bad)


# --------------------------------------------------------------- the refusals
def call(runs, d_out=OUT, cap=1 << 20, seed=1):
    lib = _atgpu.load_library()
    arr = (_atgpu.DitherRun * max(1, len(runs)))(*[_atgpu.DitherRun(*r) for r in runs])
    st = lib.atg_dither_fill_device(arr, len(runs), seed, d_out, cap, None)
    return st, lib.atg_dither_last_error()


SOUND = (0, 0, 4, 4096)  # a sound run beside the bad one: every run is checked
TOP = (1 << 64) - 1
REFUSALS = [
    ("offset off by 8", [(0, 0, 1, 8)], {}, INVALID, b"byte_offset"),
    ("offset off by 1", [(0, 0, 1, 17)], {}, INVALID, b"byte_offset"),
    ("offset off by 8 in an empty run", [(0, 0, 0, 8)], {}, INVALID, b"byte_offset"),
    ("output off by 8", [(0, 0, 1, 0)], dict(d_out=OUT + 8), INVALID, b"d_out"),
    ("output off by 1", [(0, 0, 1, 0)], dict(d_out=OUT + 1), INVALID, b"d_out"),
    ("output missing", [(0, 0, 1, 0)], dict(d_out=None), INVALID, b"d_out"),
    ("blocks past 2^64 by one", [(0, TOP, 2, 0)], {}, INVALID, b"2^64"),
    ("blocks past 2^64 from the middle", [(0, 1 << 63, (1 << 63) + 1, 0)], {}, INVALID,
     b"2^64"),
    ("runs overlap", [(1, 0, 2, 4096 + 48)], {}, INVALID, b"overlap"),
    ("runs overlap at the end", [(1, 0, 300, 0)], {}, INVALID, b"overlap"),
    ("run ends past the capacity", [(0, 0, 2, 8192)], dict(cap=8192 + 31), CAPACITY,
     b"out_cap"),
    ("run starts past the capacity", [(0, 0, 1, 1 << 21)], {}, CAPACITY, b"out_cap"),
    ("run of 2^60 blocks", [(0, 0, 1 << 60, 0)], {}, CAPACITY, b"out_cap"),
    ("16 * blocks wraps", [(0, 0, 1 << 61, 8192)], dict(cap=TOP), CAPACITY, b"out_cap"),
]


@pytest.mark.parametrize("what,bad,kw,status,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, bad, kw, status, word):
    before = slots()
    for runs in ([SOUND] + bad, bad + [SOUND]):
        st, msg = call(runs, **kw)
        assert st == status
        assert word in msg, msg
    assert slots() == before  # this component's slot alone was written


def test_the_message_names_the_run():
    st, msg = call([SOUND, SOUND[:3] + (8192,), (0, 0, 1, 24)])
    assert st == INVALID and msg.startswith(b"run 2:"), msg


def test_null_table():
    lib = _atgpu.load_library()
    assert lib.atg_dither_fill_device(None, 1, 0, OUT, 64, None) == INVALID
    assert b"runs" in lib.atg_dither_last_error()


def test_nothing_to_write_needs_no_gpu():
    """an empty table and a table of empty runs pass the checks and launch
    nothing: ATG_OK on a machine without a GPU, whatever d_out is"""
    lib = _atgpu.load_library()
    assert lib.atg_dither_fill_device(None, 0, 0, None, 0, None) == OK
    assert call([])[0] == OK
    assert call([(3, 5, 0, 0), (4, TOP, 0, 1 << 40)], d_out=None, cap=0)[0] == OK
    # a run that ends exactly at the capacity, and one at the last block, are
    # inside: with blocks to write the call goes on to the device
    assert call([(0, 0, 0, 64)], cap=64)[0] == OK
    _atgpu.dither_fill_device([], 1, None, 0)


def test_times_are_per_thread_and_honour_cap():
    lib = _atgpu.load_library()
    got = []
    t = threading.Thread(target=lambda: got.extend([
        lib.atg_dither_kernel_times(None, None, 1), lib.atg_dither_kernel_times(None, None, 0),
        _atgpu.dither_kernel_times()]))
    t.start()
    t.join()
    assert got == [0, 0, {}]
    assert lib.atg_dither_kernel_times(None, None, 0) == 0
