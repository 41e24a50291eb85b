"""CPU: the frame index block of the C ABI (include/atgpu_flac_index.h).  Its
table in _atgpu agrees with the header, the library exports it, and every
argument check of atg_flac_index_device / _host comes before any GPU call: on
a machine without a GPU each refusal still gives its own status and message,
with a device pointer that is never dereferenced."""
import ctypes
import os
import threading

import pytest

import test_signatures
from audiotools import _atgpu, decoders

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "atgpu_flac_index.h")

OK, INVALID, UNSUPPORTED = _atgpu.ATG_OK, _atgpu.ATG_ERR_INVALID, _atgpu.ATG_ERR_UNSUPPORTED
DATA = 0x200000  # never read
LEN = 1 << 20

OTHER_TABLES = (_atgpu.SIGNATURES, _atgpu.DVDA_SIGNATURES, _atgpu.MLP_SIGNATURES,
                _atgpu.TENSOR_SIGNATURES, _atgpu.DITHER_SIGNATURES, _atgpu.PROBE_SIGNATURES)
OTHER_SLOTS = sorted(n for table in OTHER_TABLES for n in table if n.endswith("last_error"))


def slots():
    lib = _atgpu.load_library()
    return {n: getattr(lib, n)() for n in OTHER_SLOTS}


# ------------------------------------------------------------------ the table
def test_table_agrees_with_header(monkeypatch):
    monkeypatch.setattr(test_signatures, "HEADER", HEADER)
    protos = test_signatures.prototypes()
    assert sorted(protos) == sorted(_atgpu.FLAC_INDEX_SIGNATURES) and len(protos) == 4
    for name, (result, params) in protos.items():
        restype, argtypes = _atgpu.FLAC_INDEX_SIGNATURES[name]
        got = (test_signatures.ctypes_kind(restype),
               [test_signatures.ctypes_kind(t) for t in argtypes])
        assert got == (result, params), name
    for table in OTHER_TABLES:
        assert not set(protos) & set(table)


def test_library_exports_the_block():
    lib = _atgpu.load_library()
    for name, (restype, argtypes) in _atgpu.FLAC_INDEX_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes or ()) == tuple(argtypes), name


def test_struct_sizes_and_version():
    assert ctypes.sizeof(_atgpu.FlacIndexRange) == 40
    assert ctypes.sizeof(_atgpu.FlacIndexEntry) == 24
    assert _atgpu.FLAC_INDEX_ENTRY_DTYPE.itemsize == 24
    assert _atgpu.load_library().atg_abi_version() == 11
    assert callable(decoders.flac_frame_index_batch)


# --------------------------------------------------------------- the refusals
def rng(offset=0, nbytes=4096, rate=44100, ch=2, bps=16, max_bs=4096, min_bs=4096, reserved=0):
    return _atgpu.FlacIndexRange(offset, nbytes, rate, ch, bps, max_bs, min_bs, reserved)


def call(ranges, data=DATA, length=LEN, cap=16, entries=True, count=True, host=False, n=None):
    lib = _atgpu.load_library()
    arr = (_atgpu.FlacIndexRange * max(1, len(ranges)))(*ranges)
    ents = (_atgpu.FlacIndexEntry * max(1, cap))()
    cnt = ctypes.c_uint64(77)
    args = (arr if ranges or n is None else None, len(ranges) if n is None else n,
            ents if entries else None, cap, ctypes.byref(cnt) if count else None)
    if host:
        st = lib.atg_flac_index_host(0, data, length, *args)
    else:
        st = lib.atg_flac_index_device(data, length, *(args + (None,)))
    return st, lib.atg_flac_index_last_error(), cnt.value


SOUND = rng()
REFUSALS = [
    ("range past the end", rng(offset=LEN - 100, nbytes=101), {}, INVALID, b"passes len"),
    ("range starts past the end", rng(offset=LEN + 1, nbytes=0), {}, INVALID, b"passes len"),
    ("offset + bytes wraps", rng(offset=16, nbytes=(1 << 64) - 8), {}, INVALID, b"passes len"),
    ("no channels", rng(ch=0), {}, INVALID, b"channels"),
    ("nine channels", rng(ch=9), {}, INVALID, b"channels"),
    ("3 bits", rng(bps=3), {}, INVALID, b"bits_per_sample"),
    ("33 bits", rng(bps=33), {}, INVALID, b"bits_per_sample"),
    ("no block size", rng(max_bs=0, min_bs=0), {}, INVALID, b"max_block_size"),
    ("block size 65536", rng(max_bs=65536), {}, INVALID, b"max_block_size"),
    ("min above max", rng(max_bs=576, min_bs=577), {}, INVALID, b"min_block_size"),
    ("reserved set", rng(reserved=1), {}, INVALID, b"reserved"),
    ("no data", SOUND, dict(data=None), INVALID, b"data is NULL"),
    ("no entries", SOUND, dict(entries=False), INVALID, b"entries is NULL"),
    ("no count", SOUND, dict(count=False), INVALID, b"n_entries"),
    ("2^40 bytes", rng(nbytes=1 << 40), dict(length=1 << 41), UNSUPPORTED, b"2^40"),
]


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("what,bad,kw,status,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, bad, kw, status, word, host):
    before = slots()
    for ranges in ([SOUND, bad], [bad, SOUND]):  # every range is checked
        st, msg, _ = call(ranges, host=host, **kw)
        assert st == status
        assert word in msg, msg
    assert slots() == before  # this component's slot alone was written


def test_the_message_names_the_range():
    st, msg, _ = call([SOUND, SOUND, rng(ch=0)])
    assert st == INVALID and msg.startswith(b"range 2:"), msg


def test_device_pointer_alignment():
    for off in (1, 2, 3):
        st, msg, _ = call([SOUND], data=DATA + off)
        assert st == INVALID and b"4-byte" in msg
    # the host entry takes bytes at any address: nothing to refuse there


def test_null_table():
    st, msg, _ = call([], n=1)
    assert st == INVALID and b"ranges" in msg


def test_nothing_to_scan_needs_no_gpu():
    """no range, or only ranges too short to hold a frame: ATG_OK with no
    entries on a machine without a GPU, whatever the data pointer is"""
    for host in (False, True):
        assert call([], host=host) == (OK, call([], host=host)[1], 0)
        st, _, n = call([rng(nbytes=0), rng(offset=LEN, nbytes=0), rng(nbytes=8)], data=None,
                        host=host)
        assert (st, n) == (OK, 0)
        st, _, n = call([rng(nbytes=8)], cap=0, entries=False, host=host)
        assert (st, n) == (OK, 0)
    assert _atgpu.flac_index_host(b"", []) == []
    assert decoders.flac_frame_index_batch([]) == []


def test_host_entry_refuses_device_minus_1():
    import bad_device
    lib = _atgpu.load_library()
    arr = (_atgpu.FlacIndexRange * 1)(rng(nbytes=64))
    ents = (_atgpu.FlacIndexEntry * 4)()
    cnt = ctypes.c_uint64()
    bad_device.check_refused(lib.atg_flac_index_host(-1, bytes(64), 64, arr, 1, ents, 4,
                                                     ctypes.byref(cnt)), "flac_index")


def test_times_are_per_thread_and_honour_cap():
    lib = _atgpu.load_library()
    got = []
    t = threading.Thread(target=lambda: got.extend([
        lib.atg_flac_index_kernel_times(None, None, 3),
        lib.atg_flac_index_kernel_times(None, None, 0), _atgpu.flac_index_kernel_times()]))
    t.start()
    t.join()
    assert got == [0, 0, {}]
    assert lib.atg_flac_index_kernel_times(None, None, 0) == 0
