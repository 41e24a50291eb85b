"""CPU: the tensor block of the C ABI (include/atgpu_tensor.h).  Its table in
_atgpu agrees with the header, the library exports it, and every argument
check of atg_pcm_to_tensor_device / atg_pcm_from_tensor_device comes before
any GPU call: on a machine without a GPU each refusal still gives its own
status and message, with device pointers that are never dereferenced."""
import ctypes
import os
import threading

import pytest

import test_signatures
from audiotools import _atgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "atgpu_tensor.h")

OK, INVALID, CAPACITY = _atgpu.ATG_OK, _atgpu.ATG_ERR_INVALID, _atgpu.ATG_ERR_CAPACITY
S16, S32 = _atgpu.PCM_S16, _atgpu.PCM_S32
F16, F32, F64, I32 = (_atgpu.TENSOR_F16, _atgpu.TENSOR_F32, _atgpu.TENSOR_F64,
                      _atgpu.TENSOR_I32)
PTR, OUT, IN = 0x10000, 0x200000, 0x300000  # never read or written

# the last_error functions of every other component
OTHER_SLOTS = sorted(n for table in (_atgpu.SIGNATURES, _atgpu.DVDA_SIGNATURES,
                                     _atgpu.MLP_SIGNATURES)
                     for n in table if n.endswith("last_error"))


def slots():
    lib = _atgpu.load_library()
    return {n: getattr(lib, n)() for n in OTHER_SLOTS}


# ------------------------------------------------------------------ the table
def prototypes(monkeypatch):
    monkeypatch.setattr(test_signatures, "HEADER", HEADER)
    monkeypatch.setitem(test_signatures.SCALARS, "atg_tensor_dtype", "i32")
    return test_signatures.prototypes()


def test_table_agrees_with_header(monkeypatch):
    protos = prototypes(monkeypatch)
    assert sorted(protos) == sorted(_atgpu.TENSOR_SIGNATURES) and len(protos) == 5
    for name, (result, params) in protos.items():
        restype, argtypes = _atgpu.TENSOR_SIGNATURES[name]
        got = (test_signatures.ctypes_kind(restype),
               [test_signatures.ctypes_kind(t) for t in argtypes])
        assert got == (result, params), name
    assert not set(protos) & (set(_atgpu.SIGNATURES) | set(_atgpu.DVDA_SIGNATURES) |
                              set(_atgpu.MLP_SIGNATURES) | set(_atgpu.PROBE_SIGNATURES))


def test_library_exports_the_block():
    lib = _atgpu.load_library()
    for name, (restype, argtypes) in _atgpu.TENSOR_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes or ()) == tuple(argtypes), name


def test_struct_sizes_and_tile():
    assert ctypes.sizeof(_atgpu.PcmToTensorRow) == 72
    assert ctypes.sizeof(_atgpu.PcmFromTensorRow) == 40
    t = _atgpu.pcm_tensor_tile_frames()
    assert t > 0 and t % 8 == 0


# -------------------------------------------------------------- PCM -> tensor
def to_row(frames=10, channels=2, bits=16, pad=None, out_offset=0, stride=None, d_pcm=PTR,
           fmt=S32, sample_offset=0, window_offset=0):
    pad = frames if pad is None else pad
    view = _atgpu.pcm_view(d_pcm, fmt, frames, sample_offset, window_offset)
    return _atgpu.pcm_to_tensor_row(view, channels, bits, pad, out_offset,
                                    pad if stride is None else stride)


def call_to(rows, d_out=OUT, dtype=F32, cap=1 << 20):
    lib = _atgpu.load_library()
    arr = (_atgpu.PcmToTensorRow * max(1, len(rows)))(*rows)
    st = lib.atg_pcm_to_tensor_device(arr, len(rows), d_out, dtype, cap, None)
    return st, lib.atg_pcm_tensor_last_error()


SOUND_TO = dict(out_offset=4096)  # a sound row beside the bad one: every row is checked
TO_REFUSALS = [
    ("no channels", [to_row(channels=0)], {}, b"channel count"),
    ("nine channels", [to_row(channels=9)], {}, b"channel count"),
    ("no bits", [to_row(bits=0)], {}, b"bits per sample"),
    ("25 bits", [to_row(bits=25)], {}, b"bits per sample"),
    ("unknown dtype", [to_row()], dict(dtype=4), b"dtype"),
    ("negative dtype", [to_row()], dict(dtype=-1), b"dtype"),
    ("unknown source format", [to_row(fmt=2)], {}, b"format"),
    ("pad below frames", [to_row(frames=10, pad=9, stride=10)], {}, b"pad_frames"),
    ("stride below pad", [to_row(frames=10, pad=12, stride=11)], {}, b"channel_stride"),
    ("float16 pointer off by 1", [to_row()], dict(d_out=OUT + 1, dtype=F16), b"element size"),
    ("float32 pointer off by 2", [to_row()], dict(d_out=OUT + 2), b"element size"),
    ("int32 pointer off by 2", [to_row()], dict(d_out=OUT + 2, dtype=I32), b"element size"),
    ("float64 pointer off by 4", [to_row()], dict(d_out=OUT + 4, dtype=F64), b"element size"),
    ("rows overlap", [to_row(out_offset=4096 + 5)], {}, b"overlap"),
    ("rows overlap at the end", [to_row(frames=3000, out_offset=0)], {}, b"overlap"),
    ("a row's second run in another row", [to_row(out_offset=4000, stride=100)], {}, b"overlap"),
    ("output missing", [to_row()], dict(d_out=None), b"d_out"),
    ("output missing for padding alone", [to_row(frames=0, pad=4)], dict(d_out=None), b"d_out"),
    ("source missing", [to_row(d_pcm=None)], {}, b"NULL"),
    ("int32 source off by 2", [to_row(d_pcm=PTR + 2)], {}, b"aligned"),
    ("int16 source off by 1", [to_row(d_pcm=PTR + 1, fmt=S16)], {}, b"aligned"),
    ("windowed source", [to_row(window_offset=1)], {}, b"window_offset"),
]


@pytest.mark.parametrize("what,bad,kw,word", TO_REFUSALS, ids=[r[0] for r in TO_REFUSALS])
def test_to_tensor_refusals(what, bad, kw, word):
    before = slots()
    st, msg = call_to([to_row(**SOUND_TO)] + bad, **kw)
    assert st == INVALID
    assert msg and word in msg, msg
    assert slots() == before


def test_two_runs_of_one_row_cannot_overlap():
    """channel_stride >= pad_frames keeps a row's own runs apart; the stride
    one below is refused"""
    st, msg = call_to([to_row(frames=8, pad=8, stride=7)])
    assert st == INVALID and b"channel_stride" in msg


def test_to_tensor_capacity():
    before = slots()
    # the second run ends at 100 + 12 + 10 = 122
    st, msg = call_to([to_row(frames=10, out_offset=100, stride=12)], cap=121)
    assert st == CAPACITY and b"out_cap_elems" in msg
    assert slots() == before
    assert call_to([to_row(frames=0, pad=5, out_offset=100)], cap=109)[0] == CAPACITY


def test_to_tensor_with_nothing_to_do():
    """no rows, and rows with nothing to write, pass and need no device"""
    lib = _atgpu.load_library()
    assert call_to([])[0] == OK
    assert call_to([to_row(frames=0), to_row(frames=0, channels=8)], d_out=None)[0] == OK
    assert lib.atg_pcm_to_tensor_device(None, 0, None, F32, 0, None) == OK
    assert lib.atg_pcm_to_tensor_device(None, 1, OUT, F32, 64, None) == INVALID
    assert b"rows" in lib.atg_pcm_tensor_last_error()


# -------------------------------------------------------------- tensor -> PCM
def from_row(frames=10, channels=2, bits=16, in_offset=0, stride=None, out_offset=0):
    return _atgpu.pcm_from_tensor_row(in_offset, frames if stride is None else stride, frames,
                                      channels, bits, out_offset)


def call_from(rows, d_in=IN, dtype=F32, in_cap=1 << 20, d_out=OUT, out_fmt=S32,
              out_cap=1 << 20):
    lib = _atgpu.load_library()
    arr = (_atgpu.PcmFromTensorRow * max(1, len(rows)))(*rows)
    st = lib.atg_pcm_from_tensor_device(arr, len(rows), d_in, dtype, in_cap, d_out, out_fmt,
                                        out_cap, None)
    return st, lib.atg_pcm_tensor_last_error()


SOUND_FROM = dict(in_offset=4096, out_offset=1024)
FROM_REFUSALS = [
    ("no channels", [from_row(channels=0)], {}, b"channel count"),
    ("nine channels", [from_row(channels=9)], {}, b"channel count"),
    ("no bits", [from_row(bits=0)], {}, b"bits per sample"),
    ("25 bits", [from_row(bits=25)], {}, b"bits per sample"),
    ("unknown dtype", [from_row()], dict(dtype=4), b"dtype"),
    ("unknown output format", [from_row()], dict(out_fmt=2), b"format"),
    ("stride below frames", [from_row(frames=10, stride=9)], {}, b"channel_stride"),
    ("24 bits into int16", [from_row(bits=24)], dict(out_fmt=S16), b"S16"),
    ("17 bits into int16", [from_row(bits=17)], dict(out_fmt=S16), b"S16"),
    ("int32 output off a boundary", [from_row(out_offset=6)], {}, b"16-byte"),
    ("int16 output off a boundary", [from_row(out_offset=4)], dict(out_fmt=S16), b"16-byte"),
    ("output buffer off a boundary", [from_row()], dict(d_out=OUT + 8), b"16-byte"),
    ("float16 pointer off by 1", [from_row()], dict(d_in=IN + 1, dtype=F16), b"element size"),
    ("float32 pointer off by 2", [from_row()], dict(d_in=IN + 2), b"element size"),
    ("float64 pointer off by 4", [from_row()], dict(d_in=IN + 4, dtype=F64), b"element size"),
    ("rows overlap", [from_row(out_offset=1024 + 16)], {}, b"overlap"),
    ("rows overlap at the end", [from_row(frames=600, out_offset=0)], {}, b"overlap"),
    ("input missing", [from_row()], dict(d_in=None), b"d_in"),
    ("output missing", [from_row()], dict(d_out=None), b"d_out"),
]


@pytest.mark.parametrize("what,bad,kw,word", FROM_REFUSALS, ids=[r[0] for r in FROM_REFUSALS])
def test_from_tensor_refusals(what, bad, kw, word):
    before = slots()
    st, msg = call_from([from_row(**SOUND_FROM)] + bad, **kw)
    assert st == INVALID
    assert msg and word in msg, msg
    assert slots() == before


def test_from_tensor_capacity():
    st, msg = call_from([from_row(frames=10, in_offset=100, stride=12)], in_cap=121)
    assert st == CAPACITY and b"in_cap_elems" in msg
    st, msg = call_from([from_row(frames=10, out_offset=1024)], out_cap=1024 + 19)
    assert st == CAPACITY and b"out_cap_samples" in msg


def test_from_tensor_with_nothing_to_do():
    lib = _atgpu.load_library()
    assert call_from([])[0] == OK
    assert call_from([from_row(frames=0)], d_in=None, d_out=None)[0] == OK
    assert lib.atg_pcm_from_tensor_device(None, 0, None, F32, 0, None, S16, 0, None) == OK
    assert lib.atg_pcm_from_tensor_device(None, 1, IN, F32, 64, OUT, S16, 64, None) == INVALID
    assert b"rows" in lib.atg_pcm_tensor_last_error()


def test_the_wrappers_raise_the_status():
    with pytest.raises(_atgpu.ATGError) as e:
        _atgpu.pcm_to_tensor_device([to_row(channels=9)], OUT, F32, 64)
    assert e.value.status == INVALID and "channel count" in e.value.message
    with pytest.raises(_atgpu.ATGError) as e:
        _atgpu.pcm_from_tensor_device([from_row(frames=10)], IN, F32, 64, OUT, S16, 8)
    assert e.value.status == CAPACITY


# ------------------------------------------------------------------ the times
def test_times_are_per_thread_and_honour_cap():
    """a thread that launched nothing has no times, and cap bounds the count"""
    lib = _atgpu.load_library()
    got = []
    t = threading.Thread(target=lambda: got.extend([
        lib.atg_pcm_tensor_kernel_times(None, None, 4),
        lib.atg_pcm_tensor_kernel_times(None, None, 0), _atgpu.pcm_tensor_kernel_times()]))
    t.start()
    t.join()
    assert got == [0, 0, {}]
    assert lib.atg_pcm_tensor_kernel_times(None, None, 0) == 0
    assert lib.atg_pcm_tensor_kernel_times(None, None, -1) == 0
