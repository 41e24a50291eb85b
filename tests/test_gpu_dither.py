"""GPU: csrc/dither.hip against the numpy port of the stream definition
(tests/dither_port.py).  Every test fills a device buffer that was set to a
canary byte, brings it back whole and compares all of it: the runs with the
port's bytes, everything else with the canary."""
import threading

import numpy as np
import pytest

import dither_port as port
from audiotools import _atgpu

pytestmark = pytest.mark.gpu

CANARY = 0xA5
SEED = 0x8F1D3A5C77E0B241


def fill(eng, runs, size, seed=SEED):
    """the runs written into a canary buffer of `size` bytes -> the buffer"""
    d = eng.device_alloc(max(16, size))
    try:
        assert d % 16 == 0
        eng.copy_to_device(d, np.full(max(16, size), CANARY, dtype=np.uint8))
        _atgpu.dither_fill_device(runs, seed, d, size)
        return eng.copy_to_host(np.empty(max(16, size), dtype=np.uint8), d)[:size]
    finally:
        eng.device_free(d)


def expected(runs, size, seed=SEED):
    want = np.full(size, CANARY, dtype=np.uint8)
    for stream, first, blocks, at in runs:
        want[at:at + 16 * blocks] = port.blocks(seed, stream, first, blocks)
    return want


def laid_out(specs, gap=16):
    """specs: [(stream, first_block, blocks)] -> (runs with a `gap`-byte
    canary before, between and after them, the buffer's size)"""
    runs, pos = [], gap
    for stream, first, blocks in specs:
        runs.append((stream, first, blocks, pos))
        pos += 16 * blocks + gap
    return runs, pos


def check(eng, specs, seed=SEED):
    runs, size = laid_out(specs)
    got, want = fill(eng, runs, size, seed), expected(runs, size, seed)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "first difference at byte %d of %d" % (bad[0], size)
    return got


def test_run_lengths(gpu_engine):
    t = _atgpu.dither_tile_blocks()
    counts = [0, 1, 2, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1]
    check(gpu_engine, [(k, 0, n) for k, n in enumerate(counts)])
    for n in counts:  # and each alone: the run is the table's only row
        check(gpu_engine, [(9, 0, n)])
    assert _atgpu.dither_kernel_times().get("fill", -1.0) >= 0.0


def test_first_blocks(gpu_engine):
    """a run may start anywhere in a stream, and the block index carries into
    the counter's second word"""
    got = check(gpu_engine, [(3, 0, 70), (3, 5, 70), (3, (1 << 32) - 1, 3),
                             (3, (1 << 64) - 2, 2)])
    # blocks 5 .. 69 of the first run are blocks 0 .. 64 of the second
    assert np.array_equal(got[16 + 16 * 5:16 + 16 * 70],
                          got[32 + 16 * 70:32 + 16 * 70 + 16 * 65])


def test_streams(gpu_engine):
    t = _atgpu.dither_tile_blocks()
    got = check(gpu_engine, [(0, 0, t + 3), (1, 0, t + 3), (1 << 32, 0, t + 3),
                             ((1 << 64) - 1, 7, 5)])
    n = 16 * (t + 3)
    a, b, c = (got[16 + k * (n + 16):16 + k * (n + 16) + n] for k in range(3))
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)


@pytest.mark.parametrize("seed", [0, 1, 1 << 32, (1 << 64) - 1])
def test_seeds(gpu_engine, seed):
    check(gpu_engine, [(0, 0, 65), (5, (1 << 32) - 2, 4)], seed)


def test_300_ragged_runs(gpu_engine):
    rng = np.random.RandomState(300)
    t = _atgpu.dither_tile_blocks()
    specs = []
    for k in range(300):
        blocks = int(rng.choice([0, 1, 2, 3, 63, 64, 65, 200, t - 1, t, t + 1,
                                 int(rng.randint(1, 2 * t + 9))]))
        first = int(rng.choice([0, 1, 5, (1 << 32) - 2, int(rng.randint(0, 1 << 62))]))
        specs.append((int(rng.choice([k, 1 << 32, int(rng.randint(0, 1 << 62))])), first, blocks))
    first = check(gpu_engine, specs)
    # a second call leaves the same buffer, canaries and all
    runs, size = laid_out(specs)
    assert np.array_equal(first, fill(gpu_engine, runs, size))


def test_an_empty_table_launches_nothing(gpu_engine):
    got = []

    def empty_calls():
        # in a thread of its own: its stage times are its own calls' alone
        got.append(fill(gpu_engine, [], 64))
        got.append(fill(gpu_engine, [(1, 2, 0, 16), (2, 0, 0, 48)], 64))
        got.append(_atgpu.dither_kernel_times())

    th = threading.Thread(target=empty_calls)
    th.start()
    th.join()
    assert len(got) == 3
    assert np.all(got[0] == CANARY) and np.all(got[1] == CANARY)
    assert got[2] == {}
