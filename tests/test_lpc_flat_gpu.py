"""K1's raw autocorrelation sums, through the probe entry
(atg_flac_lpc_probe_host: the production kernel with its probe pointer set),
against one rounded multiply and one rounded add per term in the reference's
order, computed on the host from the window table the probe returned.  All
max_lpc_order + 1 = 13 sums of every (frame, candidate) are compared as bit
patterns: the kernel's fused multiply-add inside the window's flat span
(csrc/lpc_flat.h) must not change a bit, which image parity cannot see (the
coefficients are quantised).

Shapes: 16-bit stereo mid/side, 17 tracks of 2 frames (one full wave of 16
frames and a partial one) at the block lengths 4096 4608 576 256 208 192 160
57 (52-sample groups: none flat at 192 and 57, one at 256, a first group at
the range's start at 576 and 160, a last group at its end at 208), once with
16-byte aligned track starts (4 pairs per load) and once one PCM frame off
(the one-pair loop); tracks with a short last frame (a wave with mixed N:
the general path); 24-bit 2- and 6-channel at 4096 and 1152 (the general
path with one N per wave); max_lpc_order 8 and 32 at 4096 and 576 (the other
two instantiations).  In the same shapes: the images, byte for byte,
against oracle_port.encode with the FLAC-8 options."""
import numpy as np
import pytest

import oracle_port
from audiotools import _atgpu

LENGTHS = [4096, 4608, 576, 256, 208, 192, 160, 57]
TRACKS, FRAMES = 17, 2
LAGS = 12


def options(block_size, order=LAGS):
    o = dict(oracle_port.PRESETS["8"])
    o["block_size"] = block_size
    o["max_lpc_order"] = order
    return o


def candidates(pcm, channels, mid_side):
    """interleaved int PCM -> int64 array [candidates, frames]"""
    ch = pcm.reshape(-1, channels).T.astype(np.int64)
    if channels == 2 and mid_side:
        return np.stack([ch[0], ch[1], (ch[0] + ch[1]) >> 1, ch[0] - ch[1]])
    return ch


def strict_sums(rows, window, lags=LAGS):
    """rows: int64 [r, n] samples -> float64 [r, lags + 1]: x = s * w rounded,
    every product rounded, every sum a strict left-to-right running sum"""
    x = rows.astype(np.float64) * window[None, :]
    n = x.shape[1]
    out = np.zeros((x.shape[0], lags + 1))
    for lag in range(lags + 1):
        if lag < n:
            prod = x[:, :n - lag] * x[:, lag:]
            out[:, lag] = np.add.accumulate(prod, axis=1)[:, -1]
    return out


def test_strict_sum_helper_is_sequential():
    """np.add.accumulate against a plain Python loop (one add per term)"""
    rng = np.random.default_rng(5)
    s = rng.integers(-65535, 65536, (1, 300))
    w = np.cos(np.linspace(-1.5, 1.5, 300)) ** 2
    got = strict_sums(s, w)[0]
    x = [float(a) * float(b) for a, b in zip(s[0], w)]
    for lag in range(LAGS + 1):
        acc = 0.0
        for i in range(300 - lag):
            acc = acc + x[i] * x[i + lag]
        assert acc.hex() == float(got[lag]).hex()


def test_probe_signature_agrees_with_the_header():
    """CPU: the ctypes row of include/atgpu_probe.h's one entry"""
    import re
    import test_signatures as ts
    text = open(ts.HEADER.replace("atgpu.h", "atgpu_probe.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    protos = {}
    for result, name, args in re.findall(
            r"([A-Za-z_][\w\s\*]*?)\b(atg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        protos[name] = (ts.c_kind(result, False),
                        [ts.c_kind(a, True) for a in " ".join(args.split()).split(",")])
    assert sorted(protos) == sorted(_atgpu.PROBE_SIGNATURES) == ["atg_flac_lpc_probe_host"]
    lib = _atgpu.load_library()
    for name, want in protos.items():
        restype, argtypes = _atgpu.PROBE_SIGNATURES[name]
        assert (ts.ctypes_kind(restype), [ts.ctypes_kind(t) for t in argtypes]) == want
        assert len(getattr(lib, name).argtypes) == len(want[1])
    assert not set(protos) & (set(_atgpu.SIGNATURES) | set(_atgpu.DVDA_SIGNATURES) |
                              set(_atgpu.MLP_SIGNATURES))


def noise16(frames, seed, block):
    rng = np.random.default_rng(seed)
    pcm = rng.integers(-32768, 32768, frames * 2).astype(np.int16)
    # full-scale opposite channels: |side| = 65535 in the middle of the first frame
    q = block // 2 - 8
    pcm[2 * q:2 * q + 16:2] = 32767
    pcm[2 * q + 1:2 * q + 16:2] = -32768
    return pcm


def check_sums(eng, pcm, tracks, channels, bps, block, frame_lengths, order=LAGS):
    """probe the batch; frame_lengths: per track, the lengths of its frames"""
    opt = _atgpu.make_options(**options(block, order))
    mid_side = channels == 2
    sums, win = eng.lpc_probe(opt, pcm, tracks, channels, bps, window_n=block)
    windows = {block: win}
    for n in {n for fl in frame_lengths for n in fl} - {block}:
        windows[n] = eng.lpc_probe(opt, pcm, tracks, channels, bps, window_n=n)[1]
    cand = candidates(np.asarray(pcm), channels, mid_side)
    pos, bad = 0, []
    for (start, _total), lens in zip(tracks, frame_lengths):
        at = start
        for n in lens:
            want = strict_sums(cand[:, at:at + n], windows[n], order) if n > order + 1 else \
                np.zeros((cand.shape[0], order + 1))
            got = sums[pos]
            if not np.array_equal(want.view(np.uint64), got.view(np.uint64)):
                bad.append((pos, n, int((want.view(np.uint64) != got.view(np.uint64)).sum())))
            at += n
            pos += 1
    assert pos == sums.shape[0]
    assert not bad, "frames whose sums differ (position, n, differing sums): %r" % bad[:8]
    return windows


def check_images(eng, pcm, tracks, channels, bps, block, cache=None, order=LAGS):
    opt = options(block, order)
    out, res, _, _ = eng.encode(_atgpu.make_options(**opt), pcm, tracks, channels, bps, 44100)
    for t, ((start, total), r) in enumerate(zip(tracks, res)):
        key = (block, t)
        if cache is None or key not in cache:
            want, _ = oracle_port.encode(
                np.asarray(pcm[start * channels:(start + total) * channels], dtype=np.int32),
                channels, bps, 44100, **opt)
            if cache is not None:
                cache[key] = want
        want = cache[key] if cache is not None else want
        got = out[r.out_offset:r.out_offset + r.bytes].tobytes()
        assert got == want, "block %d track %d: image differs from the port" % (block, t)


_images16 = {}  # (block, track) -> the port's image, shared by both alignments


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd_offset"])
@pytest.mark.parametrize("block", LENGTHS)
def test_stereo16_sums_and_images(gpu_engine, block, offset):
    per = block * FRAMES
    body = noise16(per * TRACKS, block, block)
    pcm = np.concatenate([np.zeros(2 * offset, np.int16), body])
    tracks = [(offset + t * per, per) for t in range(TRACKS)]
    win = check_sums(gpu_engine, pcm, tracks, 2, 16, block, [[block] * FRAMES] * TRACKS)[block]
    # the table the kernel read is flat where lpc_flat.h says, margin included
    w1, w2 = (block - 1) // 4, (3 * (block - 1)) // 4
    assert np.all(win[w1 + 1:w2 + 1] == 1.0)
    check_images(gpu_engine, pcm, tracks, 2, 16, block, _images16)


@pytest.mark.gpu
@pytest.mark.parametrize("block", [4096, 576])
@pytest.mark.parametrize("order", [8, 32])
def test_other_instantiations(gpu_engine, order, block):
    """max_lpc_order 8 and 32: the kernel's other two instantiations, whose
    margin is their own lag count (groups of 36 and 132 samples)"""
    per = block * FRAMES
    pcm = noise16(per * TRACKS, order, block)
    tracks = [(t * per, per) for t in range(TRACKS)]
    check_sums(gpu_engine, pcm, tracks, 2, 16, block, [[block] * FRAMES] * TRACKS, order)
    check_images(gpu_engine, pcm, tracks, 2, 16, block, None, order)


@pytest.mark.gpu
def test_stereo16_short_last_frame_mixed_wave(gpu_engine):
    """17 full frames, then 17 of 1000: the second wave holds one full frame
    and 15 short ones, and takes the general path"""
    block, short = 4096, 1000
    per = block + short
    pcm = noise16(per * TRACKS, 7, block)
    tracks = [(t * per, per) for t in range(TRACKS)]
    check_sums(gpu_engine, pcm, tracks, 2, 16, block, [[block, short]] * TRACKS)
    check_images(gpu_engine, pcm, tracks, 2, 16, block)


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [2, 6])
@pytest.mark.parametrize("block", [4096, 1152])
def test_24bit_general_path(gpu_engine, block, channels):
    per = block * FRAMES
    rng = np.random.default_rng(block + channels)
    pcm = rng.integers(-(1 << 23), 1 << 23, per * TRACKS * channels).astype(np.int32)
    tracks = [(t * per, per) for t in range(TRACKS)]
    check_sums(gpu_engine, pcm, tracks, channels, 24, block, [[block] * FRAMES] * TRACKS)
    check_images(gpu_engine, pcm, tracks, channels, 24, block)
