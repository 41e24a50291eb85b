"""GPU: the packed-PCM kernels (csrc/pcm_bytes.hip) through the C ABI.

One batch per (layout, integer format) holds every combination of packed
start offset mod 16 (all 16) and run length (0 ... 2T+3, T the kernels' tile)
in one launch: 16 groups of runs laid back to back on the packed side, group
g starting on an offset = g mod 16 after 0..15 canary bytes, so that every
length meets every offset and neighbours share 16-byte units; a last run
makes the batch end on the last byte of the buffer.  Unpack is compared with
the numpy port of the reference's converters and with pcm.FrameList, pack
with the port and FrameList.to_bytes; canaries between the integer slots and
around the packed runs must come back unchanged."""
import numpy as np
import pytest

import pcm_bytes_port as port
from audiotools import _atgpu, pcm

pytestmark = pytest.mark.gpu

COMBOS = [(lay, fmt) for lay in port.LAYOUTS for fmt in ("s16", "s32")
          if not (fmt == "s16" and lay[0] == 3)]
COMBO_IDS = ["%s-%s" % (port.layout_id(l), f) for l, f in COMBOS]
SLOT = 8  # samples: a 16-byte group of either format


def lengths():
    t = _atgpu.pcm_bytes_tile_samples()
    return [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257,
            t - 1, t, t + 1, 2 * t + 3]


def _dtype(fmt):
    return np.int16 if fmt == "s16" else np.int32


def _fmt(fmt):
    return _atgpu.PCM_S16 if fmt == "s16" else _atgpu.PCM_S32


class Batch(object):
    """the run table of one combination, with its buffers' sizes"""

    def __init__(self, layout):
        b = layout[0]
        self.layout = layout
        self.runs = []           # (byte_offset, samples, sample_offset)
        self.gaps = []           # canary byte ranges of the packed side
        pos, slot = 0, 0
        groups = list(range(1, 16)) + [0]
        for g in groups:
            pad = (g - pos) % 16
            self.gaps.append((pos, pos + pad))
            pos += pad
            assert pos % 16 == g
            for n in lengths():
                self.runs.append((pos, n, slot))
                pos += n * b
                slot += (n + SLOT - 1) // SLOT * SLOT + SLOT
        # the run that ends the buffer on a 16-byte boundary
        f = next(f for f in range(1, 17) if (pos + f * b) % 16 == 0)
        self.runs.append((pos, f, slot))
        pos += f * b
        slot += (f + SLOT - 1) // SLOT * SLOT + SLOT
        self.n_bytes, self.n_samples = pos, slot
        seen = set((off % 16, n) for off, n, _ in self.runs)
        assert all((o, n) in seen for o in range(16) for n in lengths())

    def random_values(self, rng, lo, hi):
        """values in [lo, hi] for every run, the extremes, 0 and -1 forced
        into each (as far as its length goes)"""
        vals = []
        for _, n, _ in self.runs:
            v = rng.integers(lo, hi + 1, n, dtype=np.int64)
            forced = [lo, hi, 0, -1][:n]
            v[:len(forced)] = forced
            vals.append(v)
        return vals


def _device(eng, arr):
    d = eng.device_alloc(max(16, arr.nbytes))
    if arr.nbytes:
        eng.copy_to_device(d, arr)
    return d


@pytest.fixture(scope="module")
def batches():
    return {lay: Batch(lay) for lay in port.LAYOUTS}


@pytest.mark.parametrize("layout,fmt", COMBOS, ids=COMBO_IDS)
def test_unpack_matrix(gpu_engine, batches, layout, fmt):
    eng, bt = gpu_engine, batches[layout]
    b, be, sg = layout
    rng = np.random.default_rng(COMBOS.index((layout, fmt)))
    lo, hi = port.value_range(layout)
    image = rng.integers(0, 256, bt.n_bytes, dtype=np.uint8)
    for (off, n, _), v in zip(bt.runs, bt.random_values(rng, lo, hi)):
        image[off:off + n * b] = np.frombuffer(port.pack(v, layout), dtype=np.uint8)
    canary = (np.arange(bt.n_samples, dtype=np.int64) * 2654435761 >> 7).astype(_dtype(fmt))
    want = canary.copy()
    for off, n, slot in bt.runs:
        raw = image[off:off + n * b].tobytes()
        w = port.unpack(raw, layout)
        assert np.array_equal(w, pcm.FrameList(raw, 1, 8 * b, be, sg).samples)
        want[slot:slot + n] = w
    assert bt.n_bytes % 16 == 0
    d_bytes, d_pcm = _device(eng, image), _device(eng, canary)
    try:
        _atgpu.pcm_unpack_device(d_bytes, bt.n_bytes, _atgpu.pcm_layout(b, be, sg), bt.runs,
                                 d_pcm, _fmt(fmt), bt.n_samples)
        got = eng.copy_to_host(np.empty_like(canary), d_pcm)
    finally:
        eng.device_free(d_bytes)
        eng.device_free(d_pcm)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "first wrong sample at %d of %d" % (bad[0], len(got))
    assert "unpack" in _atgpu.pcm_bytes_kernel_times()


def _pack_case(eng, bt, fmt, values):
    """pack `values` (one array per run) on the device -> (got, want) images
    with 16 canary bytes after the last run"""
    b, be, sg = bt.layout
    src = (np.arange(bt.n_samples, dtype=np.int64) * 40503 >> 3).astype(_dtype(fmt))
    fill = (np.arange(bt.n_bytes + 16) * 37 + 11).astype(np.uint8)
    want = fill.copy()
    for (off, n, slot), v in zip(bt.runs, values):
        src[slot:slot + n] = v.astype(_dtype(fmt))
        raw = port.pack(src[slot:slot + n], bt.layout)
        assert raw == pcm.FrameList._wrap(src[slot:slot + n], 1, 8 * b).to_bytes(be, sg)
        want[off:off + n * b] = np.frombuffer(raw, dtype=np.uint8)
    d_pcm, d_bytes = _device(eng, src), _device(eng, fill)
    try:
        _atgpu.pcm_pack_device(d_pcm, _fmt(fmt), bt.n_samples, _atgpu.pcm_layout(b, be, sg),
                               bt.runs, d_bytes, bt.n_bytes + 16)
        got = eng.copy_to_host(np.empty_like(fill), d_bytes)
    finally:
        eng.device_free(d_bytes)
        eng.device_free(d_pcm)
    return got, want, fill


@pytest.mark.parametrize("layout,fmt", COMBOS, ids=COMBO_IDS)
def test_pack_matrix(gpu_engine, batches, layout, fmt):
    bt = batches[layout]
    rng = np.random.default_rng(100 + COMBOS.index((layout, fmt)))
    lo, hi = port.value_range(layout)
    got, want, fill = _pack_case(gpu_engine, bt, fmt, bt.random_values(rng, lo, hi))
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "first wrong byte at %d of %d" % (bad[0], len(got))
    # the canaries: before the first run, between the groups, after the last
    for a, z in bt.gaps + [(bt.n_bytes, bt.n_bytes + 16)]:
        assert np.array_equal(got[a:z], fill[a:z])
    assert bt.gaps[0] == (0, 1)
    assert "pack" in _atgpu.pcm_bytes_kernel_times()


@pytest.mark.parametrize("layout,fmt", COMBOS, ids=COMBO_IDS)
def test_pack_masks_out_of_range(gpu_engine, batches, layout, fmt):
    """values over the whole range of the integer format: the low bits are
    kept, as FrameList.to_bytes keeps them"""
    bt = batches[layout]
    rng = np.random.default_rng(200 + COMBOS.index((layout, fmt)))
    info = np.iinfo(_dtype(fmt))
    got, want, _ = _pack_case(gpu_engine, bt, fmt,
                              bt.random_values(rng, int(info.min), int(info.max)))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("layout,fmt", COMBOS, ids=COMBO_IDS)
def test_pack_then_unpack_is_identity(gpu_engine, batches, layout, fmt):
    eng, bt = gpu_engine, batches[layout]
    b, be, sg = layout
    rng = np.random.default_rng(300 + COMBOS.index((layout, fmt)))
    lo, hi = port.value_range(layout)
    src = np.zeros(bt.n_samples, dtype=_dtype(fmt))
    for (_, n, slot), v in zip(bt.runs, bt.random_values(rng, lo, hi)):
        src[slot:slot + n] = v
    lay = _atgpu.pcm_layout(b, be, sg)
    d_src, d_bytes = _device(eng, src), eng.device_alloc(bt.n_bytes)
    d_back = _device(eng, np.zeros_like(src))
    try:
        _atgpu.pcm_pack_device(d_src, _fmt(fmt), bt.n_samples, lay, bt.runs, d_bytes, bt.n_bytes)
        _atgpu.pcm_unpack_device(d_bytes, bt.n_bytes, lay, bt.runs, d_back, _fmt(fmt),
                                 bt.n_samples)
        back = eng.copy_to_host(np.empty_like(src), d_back)
    finally:
        for d in (d_src, d_bytes, d_back):
            eng.device_free(d)
    assert np.array_equal(back, src)


def test_empty_tables(gpu_engine):
    eng = gpu_engine
    lay = _atgpu.pcm_layout(3, True, True)
    d = eng.device_alloc(64)
    try:
        for runs in ([], [(0, 0, 0), (5, 0, 8), (64, 0, 16)]):
            _atgpu.pcm_unpack_device(d, 64, lay, runs, d, _atgpu.PCM_S32, 16)
            _atgpu.pcm_pack_device(d, _atgpu.PCM_S32, 16, lay, runs, d, 64)
    finally:
        eng.device_free(d)


def test_host_entries_agree_with_device(gpu_engine):
    """one mixed batch: a few runs of three layouts through the _host entries
    (unaligned host buffers, odd sizes) and through the device entries"""
    eng = gpu_engine
    rng = np.random.default_rng(7)
    for layout, fmt in (((3, True, True), "s32"), ((2, True, False), "s16"),
                        ((1, False, False), "s32")):
        b, be, sg = layout
        lay = _atgpu.pcm_layout(b, be, sg)
        runs = [(3, 1000, 0), (3 + 1000 * b, 0, 1000), (5 + 1000 * b, 4099, 1008),
                (5 + 5099 * b, 7, 5112)]
        n_bytes, n_samples = 5 + 5106 * b, 5120
        image = rng.integers(0, 256, n_bytes + 1, dtype=np.uint8)[1:]   # odd host address
        out = np.full(n_samples, 77, dtype=_dtype(fmt))
        _atgpu.pcm_unpack_host(image, lay, runs, out)
        cap = (n_bytes + 15) // 16 * 16
        d_bytes = _device(eng, np.concatenate([image, np.zeros(cap - n_bytes, np.uint8)]))
        d_pcm = _device(eng, np.full(n_samples, 77, dtype=_dtype(fmt)))
        try:
            _atgpu.pcm_unpack_device(d_bytes, cap, lay, runs, d_pcm, _fmt(fmt), n_samples)
            dev = eng.copy_to_host(np.empty_like(out), d_pcm)
        finally:
            eng.device_free(d_bytes)
            eng.device_free(d_pcm)
        assert np.array_equal(out, dev)
        for off, n, slot in runs:
            assert np.array_equal(out[slot:slot + n],
                                  port.unpack(image[off:off + n * b].tobytes(), layout))
        # and back: the packed image is restored, the bytes between the runs kept
        packed = np.full(n_bytes, 0xEE, dtype=np.uint8)
        _atgpu.pcm_pack_host(out, lay, runs, packed)
        want = np.full(n_bytes, 0xEE, dtype=np.uint8)
        for off, n, slot in runs:
            want[off:off + n * b] = image[off:off + n * b]
        assert np.array_equal(packed, want)
