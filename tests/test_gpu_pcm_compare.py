"""GPU: csrc/pcm_compare.hip and audiotools.trackcmp against the numpy port
(tests/pcm_compare_port.py).  Raw buffers are torch device tensors whose
pointers go to the library; everything is exact integer work."""
import itertools

import numpy as np
import pytest

import pcm_compare_port as port
import signals
from audiotools import _atgpu

pytestmark = pytest.mark.gpu

S16, S32 = _atgpu.PCM_S16, _atgpu.PCM_S32
DTYPE = {S16: np.int16, S32: np.int32}
FMT_PAIRS = [(S16, S16), (S16, S32), (S32, S16), (S32, S32)]
FMT_IDS = ["s16-s16", "s16-s32", "s32-s16", "s32-s32"]


@pytest.fixture(scope="module")
def T():
    return _atgpu.pcm_compare_tile_frames()


def lengths(T):
    return [0, 1, 2, 7, T - 1, T, T + 1, 2 * T + 3]


class Pool(object):
    """host arrays laid into one device buffer of one sample format, every
    gap filled with non-silent filler, so that a read outside a source shows"""

    def __init__(self, fmt, seed=99):
        self.fmt = fmt
        self.parts, self.pos = [], 0
        self.rng = np.random.default_rng(seed)
        self.tensor = None

    def _filler(self, n):
        return self.rng.integers(1, 100, n).astype(DTYPE[self.fmt])

    def put(self, samples, phase=0, abut=False):
        """-> the sample index at which `samples` start: a multiple of 8 plus
        phase, or right behind the last array with abut"""
        if not abut:
            gap = (-self.pos) % 8 + 8 + phase
            self.parts.append(self._filler(gap))
            self.pos += gap
        start = self.pos
        self.parts.append(np.asarray(samples).astype(DTYPE[self.fmt]))
        self.pos += len(samples)
        return start

    def upload(self):
        import torch
        self.parts.append(self._filler(16))
        self.host = np.concatenate(self.parts)
        self.tensor = torch.from_numpy(self.host).cuda()
        torch.cuda.synchronize()
        return self

    def view(self, start, src_frames, channels, window_offset=0, skew=0):
        """skew: samples moved from sample_offset into the pointer"""
        size = self.host.itemsize
        return _atgpu.pcm_view(self.tensor.data_ptr() + skew * size, self.fmt, src_frames,
                               start - skew, window_offset)


def rand_pcm(rng, n, narrow):
    lo, hi = (-(1 << 15), 1 << 15) if narrow else (-(1 << 31), 1 << 31)
    return rng.integers(lo, hi, n).astype(np.int64)


def compare(pairs):
    return _atgpu.pcm_compare_device(pairs)


# ---- alignment and width ---------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 3, 6, 8])
@pytest.mark.parametrize("fa,fb", FMT_PAIRS, ids=FMT_IDS)
def test_every_phase_and_length(T, fa, fb, channels):
    """identical content at every pair of start phases 0..7 and every length
    gives no mismatch; one changed sample gives the port's answer"""
    rng = np.random.default_rng(channels * 10 + fa * 2 + fb)
    L = lengths(T)
    full = L[-1]
    x = rand_pcm(rng, full * channels, narrow=(fa == S16 or fb == S16))
    # places of a changed sample: (frame, channel)
    last = channels - 1
    places = [(0, 0), (1, 0), (T - 1, 0), (T, last), (2 * T - 1, last), (2 * T, 0)]
    pa, pb = Pool(fa), Pool(fb)
    a_at = [pa.put(x, ph) for ph in range(8)]
    b_at = [pb.put(x, ph) for ph in range(8)]
    # a changed copy per place and phase; the last frame's change moves with
    # the length, so it gets a copy per length below
    changed = {}
    for frame, ch in places:
        y = x.copy()
        y[frame * channels + ch] ^= 1
        changed[(frame, ch)] = (y, [pb.put(y, ph) for ph in range(8)])
    tails = {}
    for n in L[1:]:
        y = x.copy()
        y[(n - 1) * channels + last] ^= 1   # the last frame, the last channel only
        tails[n] = (y, [pb.put(y, ph) for ph in range(8)])
    pa.upload()
    pb.upload()

    pairs, want = [], []
    answers = {}

    def add(n, b_starts, key, y):
        if (key, n) not in answers:
            answers[(key, n)] = port.compare(x[:n * channels], 0, y[:n * channels], 0, n,
                                             channels)
        for i, j in itertools.product(range(8), range(8)):
            pairs.append(_atgpu.pcm_pair(pa.view(a_at[i], n, channels),
                                         pb.view(b_starts[j], n, channels), n, channels))
            want.append(answers[(key, n)])

    for n in L:
        add(n, b_at, "same", x)
        for place, (y, starts) in changed.items():
            if place[0] < n:
                add(n, starts, place, y)
        if n:
            add(n, tails[n][1], "tail", tails[n][0])
    assert answers[("same", full)] is None and answers[((T, last), full)] == T
    assert answers[("tail", T + 1)] == T
    got = compare(pairs)
    bad = [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    print("%d pairs, %d wrong" % (len(pairs), len(bad)))
    assert not bad[:5]


@pytest.mark.parametrize("fa,fb", FMT_PAIRS, ids=FMT_IDS)
def test_pointer_off_sixteen_bytes(T, fa, fb):
    """buffers aligned to their sample size only: the phase sits in d_pcm"""
    rng = np.random.default_rng(5)
    n, ch = T + 9, 2
    x = rand_pcm(rng, n * ch, True)
    y = x.copy()
    y[-1] ^= 1
    pa, pb = Pool(fa), Pool(fb)
    a0, b0, c0 = pa.put(x), pb.put(x), pb.put(y)
    pa.upload(), pb.upload()
    pairs, want = [], []
    for sa, sb in itertools.product([1, 3, 5], [1, 2, 7]):
        va = pa.view(a0, n, ch, skew=a0 - sa)
        pairs.append(_atgpu.pcm_pair(va, pb.view(b0, n, ch, skew=b0 - sb), n, ch))
        pairs.append(_atgpu.pcm_pair(va, pb.view(c0, n, ch, skew=c0 - sb), n, ch))
        want += [None, n - 1]
    assert compare(pairs) == want


# ---- sign and width ---------------------------------------------------------
def test_sign_and_width():
    p16, p32 = Pool(S16), Pool(S32)
    m1 = p16.put([-1, -1])
    lo16 = p16.put([-32768, -32768])
    w65535 = p32.put([65535, 65535])
    lo32 = p32.put([-32768, -32768])
    base = p32.put([5, 5])
    bit23 = p32.put([5, 5 | (1 << 23)])
    bit31 = p32.put([5 - (1 << 31), 5])
    p16.upload(), p32.upload()

    def one(va, vb, frames=2, ch=1):
        return _atgpu.pcm_pair(va, vb, frames, ch)

    got = compare([
        one(p16.view(m1, 2, 1), p32.view(w65535, 2, 1)),     # -1 is not 65535
        one(p32.view(w65535, 2, 1), p16.view(m1, 2, 1)),
        one(p16.view(lo16, 2, 1), p32.view(lo32, 2, 1)),     # -32768 both ways
        one(p32.view(lo32, 2, 1), p16.view(lo16, 2, 1)),
        one(p32.view(base, 2, 1), p32.view(bit23, 2, 1)),    # bit 23 alone
        one(p32.view(base, 2, 1), p32.view(bit31, 2, 1)),    # bit 31 alone
        one(p32.view(base, 1, 2), p32.view(bit23, 1, 2), 1, 2),
    ])
    assert got == [0, 0, None, None, 1, 0, 0]


# ---- earliest wins ----------------------------------------------------------
def test_three_mismatches_in_every_order(T):
    """one pair of 64 tiles: whatever is planted so far, the first wins"""
    rng = np.random.default_rng(11)
    n, ch = 64 * T, 2
    x = rand_pcm(rng, n * ch, True)
    spots = [5 * T + 17, 31 * T, 63 * T + 4095]
    pa, pb = Pool(S16), Pool(S16)
    a0 = pa.put(x, 3)
    starts, want = [], []
    for order in itertools.permutations(spots):
        y = x.copy()
        for step, frame in enumerate(order):
            y[frame * ch + 1] ^= 1
            starts.append(pb.put(y, step + 1))
            want.append(min(order[:step + 1]))
    pa.upload(), pb.upload()
    got = compare([_atgpu.pcm_pair(pa.view(a0, n, ch), pb.view(s, n, ch), n, ch)
                   for s in starts])
    assert got == want


def test_three_hundred_pairs_in_one_call(T):
    rng = np.random.default_rng(12)
    ch = 2
    pa, pb = Pool(S16), Pool(S32)
    pairs, want = [], []
    specs = []
    for k in range(300):
        n = lengths(T)[k % 8]
        x = rand_pcm(rng, n * ch, True)
        y = x.copy()
        if k % 3 == 0 and n:
            y[int(rng.integers(0, n * ch))] ^= 1
        specs.append((n, pa.put(x, k % 8), pb.put(y, (k * 3) % 4), x, y))
    pa.upload(), pb.upload()
    for n, a0, b0, x, y in specs:
        pairs.append(_atgpu.pcm_pair(pa.view(a0, n, ch), pb.view(b0, n, ch), n, ch))
        want.append(port.compare(x, 0, y, 0, n, ch))
    assert sum(w is not None for w in want) > 60
    assert compare(pairs) == want


def test_long_pair_then_empty_pairs(T):
    """more tiles than the grid has workgroups, then pairs of no frames"""
    rng = np.random.default_rng(13)
    n = 2100 * T + 5
    x = rng.integers(-30000, 30000, n).astype(np.int16)
    y = x.copy()
    y[n - 3] ^= 1
    pa, pb = Pool(S16), Pool(S16)
    a0, b0, c0 = pa.put(x, 1), pb.put(x, 6), pb.put(y, 2)
    pa.upload(), pb.upload()
    va = pa.view(a0, n, 1)
    empty = _atgpu.pcm_pair(va, pb.view(b0, n, 1), 0, 1)
    got = compare([_atgpu.pcm_pair(va, pb.view(c0, n, 1), n, 1), empty,
                   _atgpu.pcm_pair(va, pb.view(b0, n, 1), n, 1), empty, empty])
    assert got == [n - 3, None, None, None, None]
    times = _atgpu.pcm_compare_kernel_times()
    assert times["compare"] > 0 and times["probe"] == 0


# ---- windows ------------------------------------------------------------------
@pytest.mark.parametrize("fa,fb,ch", [(S16, S32, 2), (S32, S16, 3), (S32, S32, 1)])
def test_window_offsets_on_either_side(T, fa, fb, ch):
    rng = np.random.default_rng(14 + ch)
    src = T + 7
    x = rand_pcm(rng, src * ch, True)
    x[:3 * ch] = 0          # a silent head: some shifted windows agree a while
    pa, pb = Pool(fa), Pool(fb)
    a0, b0 = pa.put(x, 5), pb.put(x, 2)
    pa.upload(), pb.upload()
    offsets = [-T - 1, -1, 0, 1, src - 1, src, src + T]
    pairs, want = [], []
    for wa, wb in itertools.product(offsets, offsets):
        for frames in (src + 9, 2 * T + 9):   # past what is left: a silent tail
            pairs.append(_atgpu.pcm_pair(pa.view(a0, src, ch, wa), pb.view(b0, src, ch, wb),
                                         frames, ch))
            want.append(port.compare(x, wa, x, wb, frames, ch))
    assert any(w is None for w in want) and any(w not in (None, 0) for w in want)
    assert compare(pairs) == want


def test_empty_source_and_shared_buffer(T):
    rng = np.random.default_rng(15)
    ch, n = 2, T + 50
    x = rand_pcm(rng, n * ch, False)
    x[:40 * ch] = 0
    x[40 * ch] = 0          # the first non-zero sample is in the second channel
    x[40 * ch + 1] = 9
    p = Pool(S32)
    x0 = p.put(x, 3)
    z0 = p.put(np.zeros(n * ch), 1)
    p.upload()
    nothing = _atgpu.pcm_view(None, S16, 0)
    nowhere = p.view(x0, 0, ch)             # a source of no frames in the buffer
    got = compare([
        _atgpu.pcm_pair(nothing, p.view(z0, n, ch), n, ch),
        _atgpu.pcm_pair(p.view(z0, n, ch), nowhere, n + 5, ch),
        _atgpu.pcm_pair(nothing, p.view(x0, n, ch), n, ch),
        _atgpu.pcm_pair(p.view(x0, n, ch), nowhere, n, ch),
        _atgpu.pcm_pair(nothing, nowhere, 3 * T, ch),
        # both views in one buffer: the same view, and the view one frame on
        _atgpu.pcm_pair(p.view(x0, n, ch), p.view(x0, n, ch), n + 3, ch),
        _atgpu.pcm_pair(p.view(x0, n, ch), p.view(x0, n, ch, 1), n, ch),
    ])
    assert got == [None, None, 40, 40, None, None, port.compare(x, 0, x, 1, n, ch)]
    assert got[-1] == 39


@pytest.mark.parametrize("fa,fb", FMT_PAIRS, ids=FMT_IDS)
def test_neighbours_are_not_seen(T, fa, fb):
    """sources back to back in one buffer, other content on both sides"""
    rng = np.random.default_rng(16)
    ch = 3
    pa, pb = Pool(fa), Pool(fb)
    specs = []
    for k, n in enumerate([1, 5, T - 1, T + 2, 2 * T + 1]):
        x = rand_pcm(rng, n * ch, True)
        a0 = pa.put(x, 1, abut=k > 0)
        b0 = pb.put(x, 6, abut=k > 0)
        specs.append((n, a0, b0))
    pa.put(rand_pcm(rng, 40, True), abut=True)
    pb.put(rand_pcm(rng, 40, True), abut=True)
    pa.upload(), pb.upload()
    pairs = []
    for n, a0, b0 in specs:
        # the source alone, and a window that reaches past both its ends
        pairs.append(_atgpu.pcm_pair(pa.view(a0, n, ch), pb.view(b0, n, ch), n, ch))
        pairs.append(_atgpu.pcm_pair(pa.view(a0, n, ch, -9), pb.view(b0, n, ch, -9), n + 20, ch))
    assert compare(pairs) == [None] * len(pairs)


# ---- offset search --------------------------------------------------------------
def search(pairs, K):
    return _atgpu.pcm_offset_search_device(pairs, K)


def padded(rng, n, ch, K):
    """noise with K + 1 silent frames at both ends where there is room"""
    x = rand_pcm(rng, n * ch, True)
    x[x == 0] = 1
    if n > 2 * K + 2:
        x[:(K + 1) * ch] = 0
        x[-(K + 1) * ch:] = 0
    return x


def shifted(x, k, ch):
    """B with B(i + k) == A(i) wherever i + k is inside, silence shifted in"""
    n = len(x) // ch
    y = np.zeros_like(x)
    lo, hi = max(0, k), min(n, n + k)
    if lo < hi:
        y[lo * ch:hi * ch] = x[(lo - k) * ch:(hi - k) * ch]
    return y


@pytest.mark.parametrize("K", [0, 1, 7, 64])
def test_search_against_brute_force(T, K):
    rng = np.random.default_rng(20 + K)
    ch = 2
    pa, pb = Pool(S16), Pool(S32)
    specs = []
    for n in [1, 100, T + 5, 3 * T]:
        for k in sorted(set([-K, -1, 0, 1, K, K + 1, -K - 1])):
            # silence outside: B is a source of its own
            x = padded(rng, n, ch, K)
            y = shifted(x, k, ch)
            specs.append((n, pa.put(x, 3), x, pb.put(y, 5), y, n, 0))
            # neighbours present: B is a longer source, A lies inside it
            big = rand_pcm(rng, (n + 2 * K + 8) * ch, True)
            c = K + 3
            x = big[c * ch:(c + n) * ch]
            specs.append((n, pa.put(x, 1), x, pb.put(big, 2), big, len(big) // ch, c - k))
    pa.upload(), pb.upload()
    pairs, want = [], []
    for n, a0, x, b0, y, nb, wb in specs:
        pairs.append(_atgpu.pcm_pair(pa.view(a0, n, ch), pb.view(b0, nb, ch, wb), n, ch))
        want.append((port.best_offset(x, 0, y, wb, n, ch, K), port.compare(x, 0, y, wb, n, ch)))
    found = [w[0] for w in want]
    assert None in found and set(found) >= set(k for k in (-K, 0, K))
    assert search(pairs, K) == want


def test_search_special_signals(T):
    rng = np.random.default_rng(30)
    ch, K, n = 2, 64, 3 * T
    pa, pb = Pool(S32), Pool(S16)
    specs = []

    def add(x, y, nb=None, wb=0):
        specs.append((len(x) // ch, pa.put(x, 2), x, pb.put(y, 7), y,
                      len(y) // ch if nb is None else nb, wb))

    silent = np.zeros(n * ch, dtype=np.int64)
    add(silent, silent)                               # silence against silence: 0
    loud = silent.copy()
    loud[(n - 1) * ch] = 3                            # B non-silent only in its last frame:
    add(silent, loud)                                 # one frame back it is out of sight
    add(silent, padded(rng, n, ch, K))                # nothing fits
    # a tone of period 8 under the probe, noise after it: many candidates
    big = rand_pcm(rng, (n + 2 * K + 8) * ch, True)
    cycle = rand_pcm(rng, 8 * ch, True)
    big[:(2000 + K) * ch] = np.tile(cycle, (2000 + K) // 8 + 1)[:(2000 + K) * ch]
    c = K + 3
    add(big[c * ch:(c + n) * ch], big, wb=c - 24)
    # noise with one sample changed: no shift fits
    x = big[c * ch:(c + n) * ch].copy()
    x[2 * T * ch + 1] ^= 1
    add(x, big, wb=c)
    # the tie: B periodic with period 6 everywhere, A three frames on
    cyc6 = rand_pcm(rng, 6 * ch, True)
    per = np.tile(cyc6, (n + 2 * K + 8) // 6 + 2)[:(n + 2 * K + 8) * ch]
    add(per[(c + 3) * ch:(c + 3 + n) * ch], per, wb=c)
    pa.upload(), pb.upload()
    pairs, want = [], []
    for n_, a0, x, b0, y, nb, wb in specs:
        pairs.append(_atgpu.pcm_pair(pa.view(a0, n_, ch), pb.view(b0, nb, ch, wb), n_, ch))
        want.append((port.best_offset(x, 0, y, wb, n_, ch, K), port.compare(x, 0, y, wb, n_, ch)))
    assert [w[0] for w in want] == [0, -1, None, 24, None, 3]
    assert search(pairs, K) == want
    assert _atgpu.pcm_compare_kernel_times()["probe"] > 0


def test_search_wide(T):
    """K = 2940 (a CD drive's widest read offset, in frames) on 3T frames"""
    rng = np.random.default_rng(31)
    ch, K, n = 2, 2940, 3 * T
    big = rand_pcm(rng, (n + 2 * K + 8) * ch, True)
    c = K + 3
    x = big[c * ch:(c + n) * ch]
    pa, pb = Pool(S16), Pool(S16)
    a0, b0 = pa.put(x, 5), pb.put(big, 2)
    pa.upload(), pb.upload()
    nb = len(big) // ch
    pairs = [_atgpu.pcm_pair(pa.view(a0, n, ch), pb.view(b0, nb, ch, c - k), n, ch)
             for k in (6, -2940, 2941)]
    got = search(pairs, K)
    assert [g[0] for g in got] == [6, -2940, None]
    assert got[0] == (port.best_offset(x, 0, big, c - 6, n, ch, K),
                      port.compare(x, 0, big, c - 6, n, ch))


# ---- files ------------------------------------------------------------------------
RATE = 44100


def _encode(path, kind, x, ch=2, bits=16, rate=RATE):
    """one file in one of the nine formats, by the project's own encoders"""
    import audiotools
    from audiotools import encoders
    cls, kw = {
        "flac": (audiotools.FlacAudio, {}),
        "oga": (audiotools.OggFlacAudio, dict(encoding_function=encoders.encode_oggflac)),
        "m4a": (audiotools.ALACAudio, {}),
        "tta": (audiotools.TrueAudio, {}),
        "wv": (audiotools.WavPackAudio, dict(encoding_function=encoders.encode_wavpack)),
        "shn": (audiotools.ShortenAudio, {}),
        "wav": (audiotools.WaveAudio, {}),
        "aiff": (audiotools.AiffAudio, {}),
        "au": (audiotools.AuAudio, {}),
    }[kind]
    mask = {1: 0x4, 2: 0x3}[ch]
    cls.from_pcm(path, audiotools.FrameListReader(x, rate, ch, bits, mask),
                 total_pcm_frames=len(x) // ch, **kw)
    return path


KINDS = ["flac", "oga", "m4a", "tta", "wv", "shn", "wav", "aiff", "au"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("trackcmp")
    x = signals.make("tone", 3000, 2, 16, seed=7)
    y = x.copy()
    y[1234 * 2 + 1] ^= 1
    out = {"pcm": x}
    for k in KINDS:
        out[k] = _encode(str(d / ("same." + k)), k, x)
        out["changed." + k] = _encode(str(d / ("changed." + k)), k, y)
    out["short"] = _encode(str(d / "short.flac"), "flac", x[:2999 * 2])
    out["mono"] = _encode(str(d / "mono.wav"), "wav", x[::2].copy(), ch=1)
    out["48k"] = _encode(str(d / "48k.flac"), "flac", x, rate=48000)
    whole = open(out["flac"], "rb").read()
    out["cut"] = whole[:-1]
    x24 = signals.make("tone", 2000, 2, 24, seed=8)
    out["wav24"] = _encode(str(d / "a24.wav"), "wav", x24, bits=24)
    out["flac24"] = _encode(str(d / "a24.flac"), "flac", x24, bits=24)
    return out


def test_files_all_eighty_one_pairs(files):
    import audiotools
    pairs = [(files[a], files[b]) for a in KINDS for b in KINDS]
    assert audiotools.compare_files_batch(pairs) == [None] * 81


def test_files_changed_sample_and_lengths(files):
    import audiotools
    pairs = [(files["changed." + k], files[k]) for k in KINDS]
    pairs += [(files[KINDS[i]], files["changed." + KINDS[(i + 4) % 9]]) for i in range(9)]
    assert audiotools.compare_files_batch(pairs) == [1234] * 18
    got = audiotools.compare_files_batch([
        (files["short"], files["wav"]), (files["tta"], files["short"]),
        (files["mono"], files["flac"]), (files["48k"], files["au"]),
        (files["cut"], files["flac"]), (files["wv"], files["cut"]),
        (files["wav24"], files["flac24"]), (files["wav24"], files["flac"]),
        (open(files["shn"], "rb").read(), files["aiff"]),
        (files["flac"] + ".missing", files["flac"]), (b"not audio at all", files["flac"]),
    ])
    assert audiotools.frame_cmp_value(None, 2999, 3000) == 2998
    assert got == [2998, 2998, -1, -1, -2, -2, None, -1, None, -2, -2]


def test_files_agree_with_the_host_comparison(files):
    """the device's answers are what pcm_frame_cmp gives over the same files"""
    import audiotools
    a = audiotools.FlacAudio(files["changed.flac"])
    b = audiotools.WaveAudio(files["wav"])
    s = audiotools.FlacAudio(files["short"])
    assert audiotools.pcm_frame_cmp(a.to_pcm(), b.to_pcm()) == 1234
    assert audiotools.pcm_frame_cmp(s.to_pcm(), b.to_pcm()) == 2998
    assert audiotools.pcm_frame_cmp(b.to_pcm(), b.to_pcm()) is None


def test_compare_pcm_batch(T):
    import audiotools
    rng = np.random.default_rng(40)
    x = rng.integers(-3000, 3000, (T + 9) * 2).astype(np.int32)
    y = x.astype(np.int16)
    z = x.copy()
    z[2 * T + 1] += 1
    got = audiotools.compare_pcm_batch([x, y, x, x[:-2], x[:0]], [y, x, z, y, y], 2)
    assert got == [None, None, T, T + 7, 0]
    assert audiotools.compare_pcm_batch([], [], 2) == []


# ---- image --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def image(tmp_path_factory):
    d = tmp_path_factory.mktemp("image")
    parts = [signals.make("tone", n, 2, 16, seed=60 + k) for k, n in enumerate([3000, 4321, 2500])]
    out = {"image": _encode(str(d / "image.flac"), "flac", np.concatenate(parts))}
    for k, (kind, x) in enumerate(zip(["wav", "tta", "wv"], parts)):
        out[k] = _encode(str(d / ("track%d.%s" % (k, kind))), kind, x)
    y = parts[1].copy()
    y[10 * 2] ^= 1
    out["changed"] = _encode(str(d / "changed.m4a"), "m4a", y)
    # an image shifted by six frames, silence shifted in; its last frames silent
    a = np.concatenate(parts)
    a[-20:] = 0
    b = np.concatenate([np.zeros(12, dtype=a.dtype), a[:-12]])
    out["a"] = _encode(str(d / "a.flac"), "flac", a)
    out["b"] = _encode(str(d / "b.wav"), "wav", b)
    out["a_pcm"], out["b_pcm"] = a, b
    return out


def test_image_against_its_tracks(image, monkeypatch):
    import audiotools
    from audiotools import trackcmp
    calls = []
    for name in ("flac", "oggflac", "alac", "tta", "wavpack", "shn", "pcm"):
        def counted(headers, _name=name, _real=getattr(trackcmp, "_decode_" + name)):
            calls.append((_name, len(headers)))
            return _real(headers)
        monkeypatch.setattr(trackcmp, "_decode_" + name, counted)
    tracks = [image[0], image[1], image[2]]
    assert audiotools.compare_image_batch([(image["image"], tracks)]) == [[None, None, None]]
    # the image once, each track once: one decode per format, one file each
    assert sorted(calls) == [("flac", 1), ("pcm", 1), ("tta", 1), ("wavpack", 1)]
    del calls[:]
    got = audiotools.compare_image_batch([
        (image["image"], [image[0], image["changed"], image[2]]),
        (image["image"], tracks)])
    assert got == [[None, 10, None], [None, None, None]]
    assert sorted(calls) == [("alac", 1), ("flac", 1), ("pcm", 1), ("tta", 1), ("wavpack", 1)]
    # tracks that do not add up to the image: the last window ends in silence
    got = audiotools.compare_image_batch([(image["image"], [image[1], image[0], image[2]])])
    assert got[0][0] is not None and got[0][1] is not None and got[0][2] is None


def test_find_offset_between_two_images(image):
    import audiotools
    a, b = image["a_pcm"], image["b_pcm"]
    n = len(a) // 2
    want = (port.best_offset(a, 0, b, 0, n, 2, 16), port.compare(a, 0, b, 0, n, 2))
    assert want[0] == 6 and want[1] is not None
    got = audiotools.find_offset_batch([(image["a"], image["b"]), (image["a"], image["a"]),
                                        (image["b"], image["a"]), (image["a"], image[0])], 16)
    assert got[0] == want
    assert got[1] == (0, None)
    assert got[2][0] == port.best_offset(b, 0, a, 0, n, 2, 16)
    assert got[3][0] is None
