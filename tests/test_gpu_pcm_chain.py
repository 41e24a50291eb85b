"""GPU: csrc/pcm_chain.hip against the numpy port of a row
(tests/pcm_chain_port.py), and convert_pcm_batch against the reader path.

Every kernel test goes through atg_pcm_chain_host, which puts each source on
the device at its host address modulo 16 and sends the output buffer up and
back whole, so a source's phase is the one laid out here and a write outside
a row's range shows in the canaries."""
import numpy as np
import pytest

import pcm_chain_port as port
import signals
import audiotools
from audiotools import _atgpu, pcmconverter

pytestmark = pytest.mark.gpu

S16, S32 = _atgpu.PCM_S16, _atgpu.PCM_S32
CANARY = {S16: -23131, S32: 0x5A5A5A5A}


def tile(ic, oc):
    return _atgpu.pcm_chain_tile_frames(ic, oc)


def aligned(values, dtype, phase):
    """values in an array whose sample `phase` past a 16-byte boundary is
    values[0] -> (the array, the boundary's address)"""
    size = np.dtype(dtype).itemsize
    buf = np.zeros(len(values) + 32, dtype=dtype)
    skip = (-buf.ctypes.data % 16) // size
    buf[skip + phase:skip + phase + len(values)] = values
    return buf, buf.ctypes.data + skip * size


class Case(object):
    def __init__(self, frames, ic=2, op=port.MAP, in_bps=16, out_bps=16, cmap=None, mask=0,
                 fmt=S32, phase=0, kind="noise", seed=1, pcm=None):
        self.ic, self.op, self.in_bps, self.out_bps = ic, op, in_bps, out_bps
        self.cmap, self.mask, self.fmt, self.phase = cmap, mask, fmt, phase
        self.oc = port.out_channels(op, ic, cmap)
        self.pcm = (signals.make(kind, frames, ic, in_bps, seed=seed) if pcm is None
                    else np.asarray(pcm, dtype=np.int32))
        self.frames = len(self.pcm) // ic


def run(cases, out_fmt, seed=7, gap=8):
    """all cases in one call -> (per case the GPU output, per case the port's,
    the whole output buffer, the mask of the samples that belong to no row)"""
    rng = np.random.RandomState(seed)
    keep, rows, where, bit, pos = [], [], [], 0, gap
    for c in cases:
        buf, base = aligned(c.pcm, np.int16 if c.fmt == S16 else np.int32, c.phase)
        keep.append(buf)
        pos = (pos + 7) // 8 * 8
        bit += 3 if bit % 8 == 0 else 0  # no row's first bit on a byte boundary
        assert bit % 8 or c.out_bps >= c.in_bps
        rows.append(_atgpu.pcm_chain_row(
            _atgpu.pcm_view(base, c.fmt, c.frames, c.phase), c.ic, c.oc, c.in_bps, c.out_bps, pos,
            c.op, c.cmap, c.mask, bit))
        where.append((pos, bit))
        pos += c.frames * c.oc + gap
        if c.out_bps < c.in_bps:
            bit += c.frames * c.oc + 5
    dither = rng.bytes(bit // 8 + 2)
    out = np.full(pos + gap, CANARY[out_fmt], dtype=np.int16 if out_fmt == S16 else np.int32)
    _atgpu.pcm_chain_host(rows, out, dither)
    free = np.ones(len(out), dtype=bool)
    got, want = [], []
    for c, (o, b) in zip(cases, where):
        n = c.frames * c.oc
        free[o:o + n] = False
        got.append(out[o:o + n].astype(np.int32))
        want.append(port.convert_row(c.pcm, c.ic, c.op, c.in_bps, c.out_bps, c.cmap, c.mask,
                                     dither, b))
    return got, want, out, free


def check(cases, out_fmt, **kw):
    got, want, out, free = run(cases, out_fmt, **kw)
    for k, (g, w) in enumerate(zip(got, want)):
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "case %d: first difference at sample %d of %d" % (k, bad[0], len(w))
    assert np.all(out[free] == CANARY[out_fmt]), "a sample outside every row was written"
    return out


@pytest.mark.parametrize("out_fmt", [S16, S32], ids=["to16", "to32"])
@pytest.mark.parametrize("in_fmt", [S16, S32], ids=["from16", "from32"])
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_frame_counts(in_fmt, out_fmt, ch):
    """the dither read boundary and the tile boundary, every format pair"""
    f = tile(ch, ch)
    counts = [0, 1, 3, 4095, 4096, 4097, f - 1, f, f + 1, 2 * f + 5]
    cases = [Case(n, ic=ch, in_bps=16, out_bps=8, fmt=in_fmt, seed=n + 1, phase=k % 4)
             for k, n in enumerate(counts)]
    check(cases, out_fmt)


@pytest.mark.parametrize("out_fmt", [S16, S32], ids=["to16", "to32"])
def test_source_offsets(out_fmt):
    """every phase of a source within its 16-byte unit"""
    cases = []
    for ch in (1, 3):
        f = tile(ch, ch)
        cases += [Case(f + 3, ic=ch, in_bps=16, out_bps=8, fmt=S16, phase=p, seed=p)
                  for p in range(8)]
        cases += [Case(f + 3, ic=ch, in_bps=24, out_bps=16, fmt=S32, phase=p, seed=10 + p)
                  for p in range(4)]
        cases += [Case(5, ic=ch, in_bps=16, out_bps=16, fmt=S16, phase=p) for p in range(8)]
    check(cases, out_fmt)


CHANNEL_CASES = [
    ("identity", dict(ic=4)),
    ("permutation", dict(ic=4, cmap=[3, 0, 2, 1])),
    ("silent output", dict(ic=6, cmap=[0, 1, None, 4])),
    ("all silent", dict(ic=2, cmap=[None, None])),
    ("mono to stereo", dict(ic=1, cmap=[0, 0])),
    ("mono to eight", dict(ic=1, cmap=[0] * 8)),
    ("eight to one", dict(ic=8, cmap=[7])),
    ("average 2", dict(ic=2, op=port.AVERAGE)),
    ("average 7", dict(ic=7, op=port.AVERAGE)),
    ("downmix+average 6", dict(ic=6, op=port.DOWNMIX_AVERAGE, mask=0x3F)),
    ("downmix+average 6, no mask", dict(ic=6, op=port.DOWNMIX_AVERAGE)),
] + [("downmix %d mask %#x" % (ch, m), dict(ic=ch, op=port.DOWNMIX, mask=m))
     for ch, real in [(3, 0x7), (4, 0x33), (5, 0x37), (6, 0x3F), (8, 0x3F)] for m in (real, 0)]


@pytest.mark.parametrize("fmt,bps", [(S16, 16), (S32, 24)], ids=["from16", "from32"])
@pytest.mark.parametrize("name,kw", CHANNEL_CASES, ids=[c[0] for c in CHANNEL_CASES])
def test_channel_operations(name, kw, fmt, bps):
    c0 = Case(0, in_bps=bps, out_bps=bps, fmt=fmt, **kw)
    f = tile(c0.ic, c0.oc)
    cases = [Case(n, in_bps=bps, out_bps=bps, fmt=fmt, phase=1 + k, seed=n, **kw)
             for k, n in enumerate([1, f - 1, f + 1, 2 * f + 5])]
    # and with the bits stage behind it: its dither order is the output's
    cases += [Case(4097, in_bps=bps, out_bps=8, fmt=fmt, phase=3, seed=5, **kw)]
    check(cases, S32)
    check(cases[-1:], S16)


@pytest.mark.parametrize("in_bps,out_bps", [(24, 16), (24, 8), (16, 8), (8, 16), (16, 24),
                                            (16, 16), (24, 24), (8, 8)])
def test_bits(in_bps, out_bps):
    cases = [Case(n, ic=2, in_bps=in_bps, out_bps=out_bps, seed=in_bps + n, phase=n % 4,
                  kind="tone" if n % 2 else "noise") for n in (4097, 8192, 77)]
    check(cases, S32)
    if out_bps <= 16:
        check(cases, S16, seed=11)
        if in_bps <= 16:
            check([Case(4097, ic=2, in_bps=in_bps, out_bps=out_bps, fmt=S16, phase=5)], S16)


def random_case(rng, out_fmt):
    op = int(rng.choice([port.MAP, port.MAP, port.DOWNMIX, port.AVERAGE, port.DOWNMIX_AVERAGE]))
    ic = int(rng.randint(3, 9)) if op in (port.DOWNMIX, port.DOWNMIX_AVERAGE) else \
        int(rng.randint(1, 9))
    cmap, mask = None, 0
    if op == port.MAP:
        oc = int(rng.randint(1, 9))
        cmap = [None if rng.rand() < 0.15 else int(rng.randint(0, ic)) for _ in range(oc)]
    elif rng.rand() < 0.5:
        mask = [0, 0, 0, 0x7, 0x33, 0x37, 0x3F, 0x3F, 0x3F][ic]
    fmt = int(rng.choice([S16, S32]))
    in_bps = int(rng.choice([8, 16] if fmt == S16 else [8, 16, 24]))
    out_bps = int(rng.choice([8, 16] if out_fmt == S16 else [8, 16, 24]))
    oc = port.out_channels(op, ic, cmap)
    f = tile(ic, oc)
    frames = int(rng.choice([0, 1, 2, 7, 100, f - 1, f, f + 1, 4095, 4096, 4097,
                             int(rng.randint(1, 2 * f + 9))]))
    return Case(frames, ic=ic, op=op, in_bps=in_bps, out_bps=out_bps, cmap=cmap, mask=mask,
                fmt=fmt, phase=int(rng.randint(0, 8 if fmt == S16 else 4)),
                seed=int(rng.randint(1, 1 << 20)))


@pytest.mark.parametrize("out_fmt", [S16, S32], ids=["to16", "to32"])
def test_mixed_call_of_300_rows(out_fmt):
    rng = np.random.RandomState(300 + out_fmt)
    cases = [random_case(rng, out_fmt) for _ in range(300)]
    assert len(set((c.ic, c.oc, c.op, c.in_bps, c.out_bps, c.fmt, c.phase)
                   for c in cases)) > 200
    first = check(cases, out_fmt, gap=24, seed=3)
    # a second run leaves the same buffer, canaries and all
    assert np.array_equal(first, run(cases, out_fmt, gap=24, seed=3)[2])


@pytest.mark.parametrize("bps,fmt", [(16, S16), (16, S32), (24, S32), (8, S32)])
def test_downmix_clamps_both_ways(bps, fmt):
    hi, lo = (1 << (bps - 1)) - 1, -(1 << (bps - 1))
    frames = np.array([[hi] * 6, [lo] * 6, [hi, lo, hi, 0, hi, hi], [lo, hi, lo, 0, lo, lo],
                       [hi, hi, 0, 0, lo, lo], [lo, lo, 0, 0, hi, hi], [0, 0, hi, 0, hi, lo],
                       [hi, lo, lo, hi, lo, hi], [1, -1, 0, 0, 0, 0]] * 3, dtype=np.int32)
    for op in (port.DOWNMIX, port.DOWNMIX_AVERAGE):
        c = Case(0, ic=6, op=op, mask=0x3F, in_bps=bps, out_bps=bps, fmt=fmt, phase=1,
                 pcm=frames.reshape(-1))
        got, want, _, _ = run([c], S32)
        assert np.array_equal(got[0], want[0])
        if op == port.DOWNMIX:
            assert got[0].max() == hi and got[0].min() == lo  # both clamps were reached


# ------------------------------------------- convert_pcm_batch vs the readers
class Stream(object):
    """a dither source: the bytes of one seeded stream, handed out in order"""

    def __init__(self, seed, skip=0, zero=False):
        self.data = (b"\0" * (1 << 20) if zero
                     else np.random.RandomState(seed).bytes(1 << 20))
        self.pos = skip

    def __call__(self, n):
        self.pos += n
        assert self.pos <= len(self.data)
        return self.data[self.pos - n:self.pos]


def through_readers(x, params, target, dither):
    """PCMConverter over a reader of exact 4096-frame FrameLists, drained"""
    ch, mask, bits, rate = params
    reader = audiotools.PCMConverter(
        audiotools.FrameListReader(np.asarray(x, dtype=np.int32), rate, ch, bits, mask),
        target["sample_rate"], target["channels"], target["channel_mask"],
        target["bits_per_sample"])
    if isinstance(reader, pcmconverter.BPSConverter):
        reader._rand = dither
    parts = []
    while True:
        fl = reader.read(4096)
        if fl.frames == 0:
            break
        parts.append(np.asarray(fl.samples, dtype=np.int32))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)


def drawn(frames_out, channels, params, target):
    """bytes convert_pcm_batch draws for a track"""
    return (frames_out * channels + 7) // 8 if target["bits_per_sample"] < params[2] else 0


PLAIN_CHAINS = [  # (source params, target), no rate change
    ((6, 0x3F, 24, 48000), dict(channels=2, channel_mask=0x3, bits_per_sample=16)),
    ((6, 0x3F, 24, 48000), dict(channels=1, channel_mask=0x4, bits_per_sample=8)),
    ((2, 0x3, 16, 44100), dict(channels=1, channel_mask=0x4, bits_per_sample=8)),
    ((1, 0x4, 16, 44100), dict(channels=2, channel_mask=0x3, bits_per_sample=24)),
    ((6, 0x3F, 24, 96000), dict(channels=4, channel_mask=0x33, bits_per_sample=16)),
    ((6, 0, 24, 96000), dict(channels=4, channel_mask=0, bits_per_sample=16)),
    ((2, 0x3, 24, 44100), dict(channels=2, channel_mask=0x3, bits_per_sample=16)),
    ((2, 0x3, 16, 44100), dict(channels=2, channel_mask=0x3, bits_per_sample=16)),
    ((5, 0x37, 16, 44100), dict(channels=2, channel_mask=0, bits_per_sample=8)),
]


# every chain from int32 arrays, those of at most 16 bits from int16 too
PLAIN_RUNS = [(p, t, False) for p, t in PLAIN_CHAINS] + \
    [(p, t, True) for p, t in PLAIN_CHAINS if p[2] <= 16]


@pytest.mark.parametrize("params,target,as16", PLAIN_RUNS,
                         ids=["%dch%d-to-%dch%d-%s" % (p[0], p[2], t["channels"],
                                                       t["bits_per_sample"],
                                                       "int16" if a else "int32")
                              for p, t, a in PLAIN_RUNS])
def test_batch_equals_readers_without_resampler(params, target, as16):
    target = dict(target, sample_rate=params[3])
    tracks = [signals.make("noise", n, params[0], params[2], seed=n) for n in (1, 4096, 10000, 0)]
    arrays = [t.astype(np.int16) if as16 else t for t in tracks]
    got = audiotools.convert_pcm_batch(arrays, [params] * len(tracks), dither=Stream(42),
                                       **target)
    skip = 0
    for x, g in zip(tracks, got):
        want = through_readers(x, params, target, Stream(42, skip))
        skip += drawn(len(x) // params[0], target["channels"], params, target)
        assert g.dtype == np.int32 and np.array_equal(g, want)


RATES = [(96000, 44100), (44100, 48000)]


@pytest.fixture(scope="module")
def resampled():
    """per (rates, channels): the tracks, and the zero-dither batch result at
    the source's bits (the resampler's own output)"""
    out = {}
    for rates in RATES:
        for ch in (1, 2, 6):
            mask = {1: 0x4, 2: 0x3, 6: 0x3F}[ch]
            params = (ch, mask, 24, rates[0])
            tracks = [signals.make("tone", n, ch, 24, seed=n + ch) for n in (1, 4096, 10000)]
            plain = audiotools.convert_pcm_batch(tracks, [params] * 3, sample_rate=rates[1])
            out[rates, ch] = (params, tracks, plain)
    return out


@pytest.mark.parametrize("ch", [1, 2, 6])
@pytest.mark.parametrize("rates", RATES, ids=["96k-44k1", "44k1-48k"])
def test_batch_equals_readers_with_resampler_under_zero_dither(resampled, rates, ch):
    params, tracks, plain = resampled[rates, ch]
    target = dict(sample_rate=rates[1], channels=ch, channel_mask=params[1], bits_per_sample=16)
    got = audiotools.convert_pcm_batch(tracks, [params] * 3, dither=Stream(0, zero=True),
                                       **target)
    for x, g, p in zip(tracks, got, plain):
        assert np.array_equal(g, through_readers(x, params, target, Stream(0, zero=True)))
        assert np.array_equal(g, p >> 8)
        # the resampler alone is the reader path's too
        same = dict(target, bits_per_sample=24)
        assert np.array_equal(p, through_readers(x, params, same, None))


@pytest.mark.parametrize("rates", RATES, ids=["96k-44k1", "44k1-48k"])
def test_downmix_then_resampler_under_zero_dither(rates):
    """the channel stage in front of the resampler, the bits behind it"""
    params = (6, 0x3F, 24, rates[0])
    tracks = [signals.make("tone", n, 6, 24, seed=n) for n in (4096, 10000)]
    for ch, mask in [(2, 0x3), (1, 0x4)]:
        target = dict(sample_rate=rates[1], channels=ch, channel_mask=mask, bits_per_sample=16)
        got = audiotools.convert_pcm_batch(tracks, [params] * 2, dither=Stream(0, zero=True),
                                           **target)
        for x, g in zip(tracks, got):
            assert np.array_equal(g, through_readers(x, params, target, Stream(0, zero=True)))


@pytest.mark.parametrize("ch", [1, 2, 6])
@pytest.mark.parametrize("rates", RATES, ids=["96k-44k1", "44k1-48k"])
def test_seeded_dither_behind_resampler_only_flips_the_low_bit(resampled, rates, ch):
    params, tracks, plain = resampled[rates, ch]
    got = audiotools.convert_pcm_batch(tracks, [params] * 3, sample_rate=rates[1],
                                       bits_per_sample=16, dither=Stream(77))
    flipped = 0
    for g, p in zip(got, plain):
        low = g ^ (p >> 8)
        assert np.all((low == 0) | (low == 1))
        flipped += int(low.sum())
    assert flipped > 0


def test_mixed_params_in_one_batch_call():
    """tracks that differ in every parameter, one target"""
    specs = [(6, 0x3F, 24, 96000, 5000), (2, 0x3, 16, 44100, 4097), (1, 0x4, 8, 44100, 300),
             (2, 0x3, 24, 48000, 10000), (4, 0x33, 16, 44100, 1)]
    target = dict(sample_rate=44100, channels=2, channel_mask=0x3, bits_per_sample=16)
    tracks = [signals.make("tone", n, ch, bits, seed=n) for ch, _, bits, _, n in specs]
    got = audiotools.convert_pcm_batch(tracks, [s[:4] for s in specs],
                                       dither=Stream(0, zero=True), **target)
    for x, s, g in zip(tracks, specs, got):
        assert np.array_equal(g, through_readers(x, s[:4], target, Stream(0, zero=True)))
