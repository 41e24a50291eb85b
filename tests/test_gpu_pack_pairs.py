"""GPU parity for the frame packer's paired Rice codes (flac_frame.hip
emit_codes: two codes per bit-writer put while 2 (k + 1) + qB <= 32, a
wave-uniform fall-back to two puts otherwise), byte for byte against the CPU
oracle.

* spikes: a partition with small k and isolated spikes, so single lanes fail
  the length test; the spike sits at every offset of the 64-sample run over
  the frame's lanes (first code of a pair in some lanes, second in others),
  and some runs hold two adjacent spikes;
* k = 0: near-silent runs of 0 and +-1;
* k = 14, where only qB <= 2 pairs: full-scale white noise (which the
  encoder ends up writing VERBATIM) and noise shaped so that k = 14 is
  chosen and Rice-coded;
* odd code count: autoregressive signals of odd order (lane 0 writes
  64 - order codes), the odd order read back from the oracle's image;
* the other callers of emit_codes: every track ends in a short frame (the
  LDS-staged path), and one 6-channel 24-bit track takes the multi-wave
  kernel and the 64-bit residual loop.
"""
import numpy as np
import pytest

import oracle_port
from flac_orders import first_subframe_orders
from test_gpu_flac import check_batch
from test_gpu_k2_packed import _stereo
from test_gpu_k2_pass2_swar import _ar

pytestmark = pytest.mark.gpu

N = 4096 * 3 + 517  # three full frames and a short one
OPTS = dict(oracle_port.PRESETS["8"])


def _spikes(seed, height):
    g = np.random.default_rng(seed)
    t = np.arange(N)
    run = t // 64
    # one spike per run, its offset stepping through 0..63 (both parities);
    # every fifth run a second spike right after it, every seventh none
    at = (t % 64) == ((run + seed) % 64)
    at2 = np.roll(at, 1) & (run % 5 == 0)
    at = at & (run % 7 != 3)
    sign = np.where(g.integers(0, 2, N) == 0, -1, 1)
    l = np.round(g.normal(0, 1.2, N)) + np.where(at | at2, height * sign, 0)
    r = np.round(g.normal(0, 2.5, N)) + np.where(np.roll(at, 31), 3 * height * sign, 0)
    return _stereo(l, r)


def _near_silent(seed):
    g = np.random.default_rng(seed)
    l = np.round(g.normal(0, 0.35, N))
    r = np.where(g.integers(0, 9, N) == 0, g.integers(-1, 2, N), 0)
    return _stereo(l, r)


def _full_scale(seed):
    g = np.random.default_rng(seed)
    return _stereo(g.integers(-32768, 32768, N), g.integers(-32768, 32768, N))


def _k14(seed):
    # full-scale white noise codes VERBATIM, so k = 14 needs a shape.  The
    # encoder takes the smallest k with 2^k >= mean |r|: 65 % of the
    # magnitudes in [9000, 16000) (u >> 14 = 1), 30 % under 8000 (0) and 5 %
    # from 24576 up (u >> 14 >= 3: too long to pair) have a mean of about
    # 10900, so k = 14, and the estimate stays under VERBATIM's 16 bits.
    g = np.random.default_rng(seed)

    def chan():
        kind = g.integers(0, 100, N)
        mag = np.where(kind < 65, g.integers(9000, 16000, N), g.integers(0, 8000, N))
        mag = np.where(kind >= 95, g.integers(24576, 32768, N), mag)
        return mag * np.where(g.integers(0, 2, N) == 0, -1, 1)
    return _stereo(chan(), chan())


def test_spike_after_short_code(gpu_engine):
    pcms = [_spikes(1, 60), _spikes(2, 150), _spikes(3, 700), _spikes(4, 4000)]
    check_batch(gpu_engine, pcms, 2, 16, OPTS)


def test_k0_and_k14_partitions(gpu_engine):
    pcms = [_near_silent(1), _near_silent(2), _full_scale(3), _k14(4), _k14(5)]
    check_batch(gpu_engine, pcms, 2, 16, OPTS)
    # the shaped noise is Rice-coded, not VERBATIM
    img, lst = oracle_port.encode(pcms[3], 2, 16, 44100, **OPTS)
    kinds = {kind for kind, _ in first_subframe_orders(img, [off for off, _ in lst])}
    assert "verbatim" not in kinds


def test_odd_code_count(gpu_engine):
    pcms = [_stereo(np.round(_ar(300 + p, p, 1.0)), np.round(_ar(400 + p, p, 1.0)))
            for p in (1, 3, 5, 7, 9, 11)]
    check_batch(gpu_engine, pcms, 2, 16, OPTS)
    odd = 0
    for p in pcms:
        img, lst = oracle_port.encode(p, 2, 16, 44100, **OPTS)
        # full frames only: the register-staged kernel packs those
        offs = [off for off, n in lst if n == 4096]
        odd += sum(1 for kind, o in first_subframe_orders(img, offs) if kind == "lpc" and o % 2)
    assert odd > 0


def test_multi_wave_and_wide_residuals(gpu_engine):
    # 6 channels, 24 bits: several waves per frame, the 64-bit residual loop
    g = np.random.default_rng(9)
    n = 4096 + 300
    t = np.arange(n)
    x = np.empty((n, 6), dtype=np.int64)
    for c in range(6):
        x[:, c] = np.round(3.0e6 * np.sin(2 * np.pi * (200 + 170 * c) * t / 44100)
                           + g.normal(0, 30.0 * 4 ** c, n))
    x[::97, 2] += 4000000  # spikes: long unary runs in the generic loop too
    pcm = np.clip(x, -(1 << 23), (1 << 23) - 1).reshape(-1).astype(np.int32)
    check_batch(gpu_engine, [pcm], 6, 24, OPTS)
