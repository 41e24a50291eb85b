"""GPU: csrc/pcm_tensor.hip against the numpy port (tests/pcm_tensor_port.py).

Every call works on byte buffers that torch holds on the device.  The whole
tensor-side (or PCM-side) buffer is filled with a canary pattern before the
call and compared afterwards, as bit patterns, with the buffer the port
leaves: so a write before, between or behind the rows or into a stride gap
shows, and -0.0, NaN and subnormals count."""
import numpy as np
import pytest
import torch

import pcm_tensor_port as port
from pcm_tensor_port import F16, F32, F64, I32, bits
from audiotools import _atgpu

pytestmark = pytest.mark.gpu

S16, S32 = _atgpu.PCM_S16, _atgpu.PCM_S32
PCM_DTYPE = {S16: np.int16, S32: np.int32}
CANARY = 0x5A


def tile():
    return _atgpu.pcm_tensor_tile_frames()


def upload(host):
    """a numpy array -> (a torch byte tensor on the device holding it, its pointer)"""
    t = torch.from_numpy(np.ascontiguousarray(host).view(np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr()


def download(t, dtype):
    return t.cpu().numpy().view(dtype)


def samples_of(rng, n, bps):
    """both extremes of the width, 0, +-1 and noise"""
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    x = rng.randint(lo, hi + 1, size=n).astype(np.int32)
    head = np.array([lo, hi, 0, 1, -1, hi, lo], dtype=np.int32)[:n]
    x[:len(head)] = head
    return x


class Row(object):
    """one row of a call: its parameters and, for PCM -> tensor, its samples"""

    def __init__(self, ch, bps, frames, pad_extra, stride_extra, src_phase, elem_phase, fmt,
                 by_pointer=False):
        self.ch, self.bps, self.frames = ch, bps, frames
        self.pad = frames + pad_extra
        self.stride = self.pad + stride_extra
        self.src_phase, self.elem_phase, self.fmt, self.by_pointer = (src_phase, elem_phase, fmt,
                                                                      by_pointer)


def grid(fmt, group, seed):
    """rows over every channel count, frame count and padding of the issue's
    list, the bit depths, source phases, element phases and strides cycling
    through all their values"""
    t = tile()
    per = 8 if fmt == S16 else 4
    depths = (8, 16) if fmt == S16 else (8, 16, 24)
    rows, k = [], seed
    for ch in (1, 2, 3, 5, 6, 8):
        for frames in (0, 1, 2, t - 1, t, t + 1, 2 * t + 3):
            for pad_extra in (0, 1, t + 5):
                rows.append(Row(ch, depths[k % len(depths)], frames, pad_extra, (0, 3)[k // 2 % 2],
                                k % per, (k // 3) % group, fmt, by_pointer=bool(k // 5 % 2)))
                k += 1
    # every source phase against every element phase, on rows that cross a tile
    for sp in range(per):
        for ep in range(group):
            rows.append(Row(2 + (sp + ep) % 2, depths[(sp + ep) % len(depths)], t + 3 + sp, ep % 3,
                            ep % 2 * 3, sp, ep, fmt, by_pointer=bool(sp % 2)))
    return rows


def lay_out_sources(rows, rng):
    """-> (per format the host PCM buffer, per row (format, sample index of the
    16-byte boundary before its first sample)); a row's samples in r.samples"""
    pos = {S16: 8, S32: 8}
    where = []
    for r in rows:
        per = 8 if r.fmt == S16 else 4
        r.samples = samples_of(rng, r.frames * r.ch, r.bps)
        where.append(pos[r.fmt])
        pos[r.fmt] += (r.src_phase + len(r.samples) + per - 1) // per * per + per
    bufs = {}
    for fmt in (S16, S32):
        bufs[fmt] = rng.randint(-100, 100, size=pos[fmt] + 8).astype(PCM_DTYPE[fmt])
    for r, at in zip(rows, where):
        a = at + r.src_phase
        bufs[r.fmt][a:a + len(r.samples)] = r.samples
    return bufs, where


def lay_out_runs(rows, group, start=5):
    """element offsets of the rows' channel 0 runs, each at its element phase
    within a 16-byte unit, a gap of canaries between rows -> (offsets, size)"""
    offs, pos = [], start
    for r in rows:
        pos += (r.elem_phase - pos) % group
        offs.append(pos)
        pos += (r.ch - 1) * r.stride + r.pad + 1 + r.elem_phase % 3
    return offs, pos + 7


def run_to_tensor(rows, dtype, seed=3):
    """-> (the buffer the GPU leaves, the buffer the port leaves), as bits"""
    np_dtype = port.DTYPES[dtype]
    size = np.dtype(np_dtype).itemsize
    group = 16 // size
    rng = np.random.RandomState(seed)
    bufs, where = lay_out_sources(rows, rng)
    dev = {fmt: upload(b) for fmt, b in bufs.items()}
    offs, total = lay_out_runs(rows, group)
    want = np.full(total * size, CANARY, dtype=np.uint8).view(np_dtype)
    # the tensor buffer starts one element past a 16-byte boundary
    t_out, p_out = upload(np.full((total + 1) * size, CANARY, dtype=np.uint8))
    table = []
    for r, at, off in zip(rows, where, offs):
        width = 2 if r.fmt == S16 else 4
        base = dev[r.fmt][1]
        if r.by_pointer:
            view = _atgpu.pcm_view(base + (at + r.src_phase) * width, r.fmt, r.frames, 0)
        else:
            view = _atgpu.pcm_view(base + at * width, r.fmt, r.frames, r.src_phase)
        table.append(_atgpu.pcm_to_tensor_row(view, r.ch, r.bps, r.pad, off, r.stride))
        port.to_tensor_row(want, r.samples, r.ch, r.bps, dtype, r.pad, off, r.stride)
    _atgpu.pcm_to_tensor_device(table, p_out + size, dtype, total,
                                torch.cuda.current_stream().cuda_stream)
    got = download(t_out, np_dtype)
    canary = bits(np.full(size, CANARY, dtype=np.uint8).view(np_dtype))[0]
    assert bits(got[:1])[0] == canary, "the element before the buffer was written"
    return bits(got[1:]), bits(want)


def explain(got, want):
    bad = np.nonzero(got != want)[0]
    return "%d elements differ, the first at %d: %#x for %#x" % (
        len(bad), bad[0], got[bad[0]], want[bad[0]]) if len(bad) else ""


DTYPE_IDS = {F16: "float16", F32: "float32", F64: "float64", I32: "int32"}


@pytest.mark.parametrize("fmt", [S16, S32], ids=["from16", "from32"])
@pytest.mark.parametrize("dtype", [F16, F32, F64, I32], ids=lambda d: DTYPE_IDS[d])
def test_to_tensor_grid(dtype, fmt):
    rows = grid(fmt, 16 // np.dtype(port.DTYPES[dtype]).itemsize, seed=dtype)
    got, want = run_to_tensor(rows, dtype)
    assert np.array_equal(got, want), explain(got, want)
    again, _ = run_to_tensor(rows, dtype)
    assert np.array_equal(again, got), "a second run differs"


def test_float16_subnormal_is_not_flushed():
    r = Row(1, 16, 4, 0, 0, 0, 0, S16)
    got, want = run_to_tensor([r], F16)
    assert np.array_equal(got, want)
    # the row's third sample is 0, the fourth 1: 2^-15
    assert r.samples[3] == 1 and 0x0200 in got.tolist()


def test_zero_frames_with_padding_is_zero_filled():
    for dtype in (F16, F32, F64, I32):
        rows = [Row(ch, 16, 0, pad, 3, 0, ch % 2, S32) for ch in (1, 2, 8)
                for pad in (1, 7, tile() + 9)]
        got, want = run_to_tensor(rows, dtype)
        assert np.array_equal(got, want), explain(got, want)
        assert (got == 0).sum() == sum(r.ch * r.pad for r in rows)


def test_300_mixed_rows_in_one_call():
    rng = np.random.RandomState(300)
    rows = []
    for k in range(300):
        fmt = (S16, S32)[k % 2]
        frames = int(rng.choice([0, 1, 5, 40, 333, tile() + 1])) if k % 10 else 3 * tile() + 7
        rows.append(Row(int(rng.randint(1, 9)), int(rng.choice((8, 16) if fmt == S16
                                                                 else (8, 16, 24))),
                        frames, int(rng.choice([0, 2, 9])), int(rng.choice([0, 1, 5])),
                        int(rng.randint(0, 8 if fmt == S16 else 4)), int(rng.randint(0, 8)), fmt,
                        by_pointer=bool(k % 3)))
    for dtype in (F32, F16):
        for r in rows:
            r.elem_phase %= 16 // np.dtype(port.DTYPES[dtype]).itemsize
        got, want = run_to_tensor(rows, dtype, seed=9)
        assert np.array_equal(got, want), explain(got, want)
    assert set(_atgpu.pcm_tensor_kernel_times()) == {"to_tensor"}


def test_full_8_channel_tile_off_a_unit_boundary():
    """A full tile of 8 channels is as many 16-byte units as the lanes' loads
    hold; a source that starts inside a unit adds one, which lane 0 loads
    (pcm_rows.h).  One row per non-zero source phase of either format."""
    rows = [Row(8, 16 if fmt == S16 else 24, tile() + 1, 0, 0, phase, phase % 4, fmt,
                by_pointer=bool(phase % 2))
            for fmt, per in ((S16, 8), (S32, 4)) for phase in range(1, per)]
    assert len(rows) == 10
    got, want = run_to_tensor(rows, F32, seed=8)
    assert np.array_equal(got, want), explain(got, want)


# ------------------------------------------------------------- tensor -> PCM
def elements_of(rng, n, bps, dtype):
    """what the issue lists, then noise: exact k / 2^(b-1), +-(k + 0.5) /
    2^(b-1), the neighbours of integers and of +-1.0, +-2.0, NaN, +-inf, -0.0,
    the smallest subnormals; for int32 values past both clamps"""
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    if dtype == I32:
        x = rng.randint(lo, hi + 1, size=n).astype(np.int32)
        head = np.array([lo - 1, hi + 1, -(1 << 31), (1 << 31) - 1, lo, hi, 0, -1, lo * 2, hi * 3],
                        dtype=np.int64).astype(np.int32)[:n]
        x[:len(head)] = head
        return x
    t = port.DTYPES[dtype]
    scale = float(1 << (bps - 1))
    k = rng.randint(lo, hi + 1, size=n).astype(np.float64)
    x = (k / scale).astype(t)
    ks = np.array([lo, hi, 0, 1, -1, 3, -3, hi - 1, lo + 1, 100 % hi, -(77 % hi)], dtype=np.float64)
    exact = (ks / scale).astype(t)
    halves = np.concatenate([((ks + 0.5) / scale), (-(ks + 0.5) / scale)]).astype(t)
    ones = np.array([1.0, -1.0], dtype=t)
    around = np.concatenate([exact, ones])
    up = np.nextafter(around, np.array(np.inf, dtype=t))
    down = np.nextafter(around, np.array(-np.inf, dtype=t))
    tiny = np.nextafter(np.array(0, dtype=t), np.array(1, dtype=t))
    special = np.array([2.0, -2.0, np.nan, np.inf, -np.inf, -0.0, 0.0, tiny, -tiny,
                        np.finfo(t).max, -np.finfo(t).max, np.finfo(t).tiny], dtype=t)
    head = np.concatenate([exact, halves, ones, up, down, special]).astype(t)
    if n >= len(head):
        x[:len(head)] = head
    else:
        # a short row takes its share of the list, by its length
        x[:] = np.roll(head, -7 * n)[:n]
    return x


def run_from_tensor(rows, dtype, out_fmt, seed=4):
    np_dtype = port.DTYPES[dtype]
    size = np.dtype(np_dtype).itemsize
    group = 16 // size
    rng = np.random.RandomState(seed)
    offs, total = lay_out_runs(rows, group)
    host = np.full((total + 1) * size, CANARY, dtype=np.uint8).view(np_dtype)
    inp = host[1:]  # one element past a 16-byte boundary, as on the device
    for r, off in zip(rows, offs):
        for c in range(r.ch):
            a = off + c * r.stride
            inp[a:a + r.frames] = elements_of(rng, r.frames, r.bps, dtype)
    t_in, p_in = upload(host)
    out_per = 8 if out_fmt == S16 else 4
    starts, pos = [], out_per
    for r in rows:
        starts.append(pos)
        pos += (r.frames * r.ch + out_per - 1) // out_per * out_per + out_per * (r.elem_phase % 2)
    want = np.full((pos + out_per) * (16 // out_per), CANARY,
                   dtype=np.uint8).view(PCM_DTYPE[out_fmt])
    t_out, p_out = upload(want)
    table = []
    with np.errstate(all="ignore"):
        for r, off, at in zip(rows, offs, starts):
            table.append(_atgpu.pcm_from_tensor_row(off, r.stride, r.frames, r.ch, r.bps, at))
            want[at:at + r.frames * r.ch] = port.from_tensor_row(inp, off, r.stride, r.frames,
                                                                 r.ch, r.bps)
    _atgpu.pcm_from_tensor_device(table, p_in + size, dtype, total, p_out, out_fmt, len(want),
                                  torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(download(t_in, np.uint8), host.view(np.uint8)), "the input changed"
    return download(t_out, PCM_DTYPE[out_fmt]), want


@pytest.mark.parametrize("out_fmt", [S16, S32], ids=["to16", "to32"])
@pytest.mark.parametrize("dtype", [F16, F32, F64, I32], ids=lambda d: DTYPE_IDS[d])
def test_from_tensor_grid(dtype, out_fmt):
    # the grid's bit depths follow its format argument: 8 and 16 for int16 output
    rows = grid(out_fmt, 16 // np.dtype(port.DTYPES[dtype]).itemsize, seed=dtype + 1)
    got, want = run_from_tensor(rows, dtype, out_fmt)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%d samples differ, the first at %d: %d for %d" % (
        len(bad), bad[0], got[bad[0]], want[bad[0]])
    again, _ = run_from_tensor(rows, dtype, out_fmt)
    assert np.array_equal(again, got), "a second run differs"
    assert set(_atgpu.pcm_tensor_kernel_times()) == {"from_tensor"}


def test_round_trip_on_the_device():
    """int -> float32 -> int through both kernels is the identity"""
    rows = [Row(ch, bps, tile() + 11, 2, 3, ch % 4, ch % 4, S32)
            for ch in (1, 2, 6) for bps in (8, 16, 24)]
    size, group = 4, 4
    rng = np.random.RandomState(5)
    bufs, where = lay_out_sources(rows, rng)
    t_src, p_src = upload(bufs[S32])
    offs, total = lay_out_runs(rows, group)
    t_mid, p_mid = upload(np.full(total * size, CANARY, dtype=np.uint8))
    stream = torch.cuda.current_stream().cuda_stream
    _atgpu.pcm_to_tensor_device(
        [_atgpu.pcm_to_tensor_row(_atgpu.pcm_view(p_src, S32, r.frames, at + r.src_phase), r.ch,
                                  r.bps, r.pad, off, r.stride)
         for r, at, off in zip(rows, where, offs)], p_mid, F32, total, stream)
    starts, pos = [], 0
    for r in rows:
        starts.append(pos)
        pos += (r.frames * r.ch + 3) // 4 * 4
    t_out, p_out = upload(np.zeros(pos, dtype=np.int32))
    _atgpu.pcm_from_tensor_device(
        [_atgpu.pcm_from_tensor_row(off, r.stride, r.frames, r.ch, r.bps, at)
         for r, off, at in zip(rows, offs, starts)], p_mid, F32, total, p_out, S32, pos, stream)
    out = download(t_out, np.int32)
    for r, at in zip(rows, starts):
        assert np.array_equal(out[at:at + len(r.samples)], r.samples)
