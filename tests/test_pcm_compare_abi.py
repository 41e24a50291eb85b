"""CPU: the argument checks of atg_pcm_compare_device and
atg_pcm_offset_search_device come before any GPU call -- every refusal gives
its status and a message, with host pointers that are never dereferenced --
and empty batches return ATG_OK without a GPU."""
import ctypes

import pytest

from audiotools import _atgpu

INVALID, UNSUPPORTED = _atgpu.ATG_ERR_INVALID, _atgpu.ATG_ERR_UNSUPPORTED
PTR = 0x10000  # never read


def view(**kw):
    d = dict(d_pcm=PTR, fmt=_atgpu.PCM_S32, src_frames=10, sample_offset=0, window_offset=0)
    d.update(kw)
    return _atgpu.pcm_view(d["d_pcm"], d["fmt"], d["src_frames"], d["sample_offset"],
                           d["window_offset"])


def pair(a=None, b=None, frames=10, channels=2):
    return _atgpu.pcm_pair(a or view(), b or view(), frames, channels)


def call(pairs, max_offset=None):
    lib = _atgpu.load_library()
    n = len(pairs)
    arr = (_atgpu.PcmPair * max(1, n))(*pairs)
    res = (_atgpu.PcmCmpResult * max(1, n))()
    if max_offset is None:
        st = lib.atg_pcm_compare_device(arr, n, res, None)
    else:
        st = lib.atg_pcm_offset_search_device(arr, n, max_offset, res, None)
    return st, res, lib.atg_pcm_compare_last_error()


REFUSALS = [
    ("unknown format a", pair(a=view(fmt=2)), INVALID),
    ("unknown format b", pair(b=view(fmt=7)), INVALID),
    ("null pcm", pair(a=view(d_pcm=None)), INVALID),
    ("null pcm b", pair(b=view(d_pcm=None)), INVALID),
    ("s32 off by 2", pair(a=view(d_pcm=PTR + 2)), INVALID),
    ("s16 off by 1", pair(b=view(d_pcm=PTR + 1, fmt=_atgpu.PCM_S16)), INVALID),
    ("no channels", pair(channels=0), INVALID),
    ("frames too many", pair(frames=1 << 61, channels=2), INVALID),
    ("frames too many 3ch", pair(frames=((1 << 62) + 2) // 3, channels=3), INVALID),
    ("source too long", pair(a=view(src_frames=1 << 61)), INVALID),
    ("source too long b", pair(b=view(src_frames=1 << 62), channels=1), INVALID),
    ("window too far", pair(a=view(window_offset=1 << 62)), INVALID),
    ("window too far back", pair(b=view(window_offset=-(1 << 62))), INVALID),
    ("nine channels", pair(channels=9), UNSUPPORTED),
]


@pytest.mark.parametrize("search", [False, True], ids=["compare", "search"])
@pytest.mark.parametrize("what,bad,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, bad, status, search):
    # a sound pair first: every pair of the table is checked
    st, _, msg = call([pair(), bad], 3 if search else None)
    assert st == status
    assert msg


def test_largest_accepted_sizes_pass_the_checks():
    """just under the bounds is no refusal: with frames == 0 nothing runs"""
    ok = pair(a=view(src_frames=(1 << 61) - 1, window_offset=(1 << 62) - 1),
              b=view(d_pcm=None, src_frames=0, window_offset=-(1 << 62) + 1), frames=0)
    st, res, _ = call([ok])
    assert st == _atgpu.ATG_OK
    assert res[0].first_mismatch == _atgpu.PCM_NO_MISMATCH


def test_null_arrays():
    lib = _atgpu.load_library()
    res = (_atgpu.PcmCmpResult * 1)()
    arr = (_atgpu.PcmPair * 1)(pair())
    assert lib.atg_pcm_compare_device(None, 1, res, None) == INVALID
    assert lib.atg_pcm_compare_last_error()
    assert lib.atg_pcm_compare_device(arr, 1, None, None) == INVALID
    assert lib.atg_pcm_offset_search_device(None, 1, 0, res, None) == INVALID
    assert lib.atg_pcm_offset_search_device(arr, 1, 0, None, None) == INVALID


def test_max_offset_bound():
    st, _, msg = call([pair()], 65536)
    assert st == UNSUPPORTED and b"65535" in msg
    # the bound is checked for an empty table too, and 65535 itself passes
    assert call([], 65536)[0] == UNSUPPORTED
    assert call([pair(frames=0)], 65535)[0] == _atgpu.ATG_OK


def test_nothing_to_do_needs_no_gpu():
    lib = _atgpu.load_library()
    assert lib.atg_pcm_compare_device(None, 0, None, None) == _atgpu.ATG_OK
    assert lib.atg_pcm_offset_search_device(None, 0, 5, None, None) == _atgpu.ATG_OK
    empties = [pair(frames=0), pair(frames=0, channels=8)]
    st, res, _ = call(empties)
    assert st == _atgpu.ATG_OK
    for r in res:
        assert (r.first_mismatch, r.offset, r.offset_found) == (_atgpu.PCM_NO_MISMATCH, 0, 0)
    st, res, _ = call(empties, 7)
    assert st == _atgpu.ATG_OK
    for r in res:
        assert (r.first_mismatch, r.offset, r.offset_found) == (_atgpu.PCM_NO_MISMATCH, 0, 1)


def test_binding_wrappers_on_empty_input():
    assert _atgpu.pcm_compare_device([]) == []
    assert _atgpu.pcm_compare_device([pair(frames=0)]) == [None]
    assert _atgpu.pcm_offset_search_device([pair(frames=0)], 3) == [(0, None)]
    with pytest.raises(_atgpu.ATGError) as e:
        _atgpu.pcm_compare_device([pair(channels=9)])
    assert e.value.status == UNSUPPORTED
    assert _atgpu.pcm_compare_tile_frames() > 0


def test_struct_sizes_match_the_header():
    assert ctypes.sizeof(_atgpu.PcmView) == 40
    assert ctypes.sizeof(_atgpu.PcmPair) == 96
    assert ctypes.sizeof(_atgpu.PcmCmpResult) == 16
