"""GPU parity for K2's three-op pass 2 (flac_search16.hip packed_vsum_swar,
pass2_swar.h), byte for byte against the CPU oracle.

A wave takes the three-op form only when every lane has kv - 1 >= 0 (kv - 9
under the loud selector) and B's low half is zero; otherwise it keeps the
five-op packed form, and a wave that fails the 2^15 / 2^23 qualification
recomputes.  These signals put each of those decisions both ways inside one
frame:

* mixed kv: 64-sample lane runs alternate between near silence (k <= 1, so
  kv = 0) and moderate noise (k about 6);
* qualification boundary: a quiet tone with one impulse per lane run, the
  impulse sizes swept so the lanes' sum |r| straddle 2^15; and full-scale
  sign-alternating bursts with swept amplitude for the loud selector's 2^23;
* loud selector kv edges: noise whose per-run sigma makes k = 8, 9, 10, 11
  in neighbouring runs (kv - 8 = -1 .. 2);
* 1..7 wasted bits (B's low half not zero);
* lane 0's warm-up for orders 1..12: autoregressive signals of every order,
  with the chosen orders read back from the oracle's image.
"""
import numpy as np
import pytest

import oracle_port
from flac_orders import first_subframe_orders
from test_gpu_flac import check_batch
from test_gpu_k2_packed import _stereo, _wasted

pytestmark = pytest.mark.gpu

N = 4096 * 3 + 517  # three full frames and a short one
OPTS = dict(oracle_port.PRESETS["8"])


def _mixed_kv(seed, period):
    g = np.random.default_rng(seed)
    run = np.arange(N) // 64
    amp_l = np.where(run % period == 0, 0.45, 45.0)
    amp_r = np.where(run % period == 0, 60.0, 0.3)
    return _stereo(np.round(g.normal(0, 1, N) * amp_l), np.round(g.normal(0, 1, N) * amp_r))


def _impulses_15(seed):
    # one impulse per 64-sample run on a quiet tone; sizes sweep 9000..32767
    # over the frame's 64 runs, so sum |r| of a lane (about the impulse and
    # its echo through the predictor) lies under 2^15 in some lanes, over in
    # others, for every order
    g = np.random.default_rng(seed)
    t = np.arange(N)
    run = t // 64
    size = 9000 + ((run * 37 + seed) % 64) * 377
    at = (t % 64) == ((run * 5 + seed) % 64)
    sign = np.where(g.integers(0, 2, N) == 0, -1, 1)
    l = np.round(150 * np.sin(2 * np.pi * 300 * t / 44100)) + np.where(at, size * sign, 0)
    r = np.round(90 * np.sin(2 * np.pi * 410 * t / 44100) + g.normal(0, 2, N))
    r = r + np.where(np.roll(at, 17), (size // 2) * sign, 0)
    return _stereo(l, r)


def _bursts_23(seed):
    # sign-alternating full-scale bursts with a swept envelope: the low
    # orders leave residuals of several times the sample range, so lane sums
    # run from under to over 2^23 across runs and orders
    g = np.random.default_rng(seed)
    t = np.arange(N)
    run = t // 64
    env = 2000 + ((run * 29 + seed) % 64) * 480
    alt = np.where(t % 2 == 0, 1, -1) * np.where((t // 5) % 2 == 0, 1, -1)
    l = env * alt + np.round(g.normal(0, 300, N))
    r = -env[::-1] * alt + np.round(g.normal(0, 300, N))
    return _stereo(l, r)


def _k_edges(seed):
    # white noise, sigma per 64-sample run: the Rice parameter of a run is
    # about log2(1.1 sigma), so 230, 460, 920, 1840 give k = 8, 9, 10, 11
    g = np.random.default_rng(seed)
    run = np.arange(N) // 64
    sig_l = np.array([230.0, 460.0, 920.0, 1840.0])[run % 4]
    sig_r = np.array([920.0, 300.0, 520.0, 700.0])[(run + seed) % 4]
    return _stereo(np.round(g.normal(0, 1, N) * sig_l), np.round(g.normal(0, 1, N) * sig_r))


def _ar(seed, order, sigma):
    # a stable autoregressive process of the given order (poles at radius
    # 0.9) driven by noise: the exhaustive search settles near that order
    g = np.random.default_rng(seed)
    ang = np.linspace(0.3, 2.6, (order + 1) // 2)
    poles = list(0.9 * np.exp(1j * ang[: order // 2]))
    poles = poles + [np.conj(p) for p in poles] + ([0.85] if order % 2 else [])
    a = np.real(np.poly(poles))  # 1, a1, ..., a_order
    e = g.normal(0, sigma, N + 256)
    x = np.zeros(N + 256)
    for i in range(order, N + 256):
        x[i] = e[i] - np.dot(a[1:], x[i - order:i][::-1])
    x = x[256:]
    return x * (6000.0 / max(1.0, np.abs(x).max()))


def _ar_tracks():
    return [_stereo(np.round(_ar(100 + p, p, 1.0)), np.round(_ar(200 + p, 13 - p, 1.0)))
            for p in range(1, 13)]


@pytest.mark.parametrize("seed", [1, 2])
def test_mixed_kv_in_one_frame(gpu_engine, seed):
    check_batch(gpu_engine, [_mixed_kv(seed, 2), _mixed_kv(seed + 10, 3)], 2, 16, OPTS)


def test_qualification_boundaries(gpu_engine):
    pcms = [_impulses_15(1), _impulses_15(2), _bursts_23(3), _bursts_23(4)]
    check_batch(gpu_engine, pcms, 2, 16, OPTS)


def test_loud_selector_kv_edges(gpu_engine):
    check_batch(gpu_engine, [_k_edges(s) for s in (1, 2, 3)], 2, 16, OPTS)


def test_wasted_bits(gpu_engine):
    check_batch(gpu_engine, [_wasted(5, w) for w in range(1, 8)], 2, 16, OPTS)


def test_lane0_warmup_every_order(gpu_engine):
    pcms = _ar_tracks()
    check_batch(gpu_engine, pcms, 2, 16, OPTS)
    # the images equal the oracle's (checked above): read the orders chosen
    # for the first subframe of every frame from the oracle's images
    orders = set()
    for p in pcms:
        img, lst = oracle_port.encode(p, 2, 16, 44100, **OPTS)
        got = {o for kind, o in first_subframe_orders(img, [off for off, _ in lst])
               if kind == "lpc"}
        orders |= got
    assert any(o % 2 for o in orders) and any(o % 2 == 0 for o in orders), orders
