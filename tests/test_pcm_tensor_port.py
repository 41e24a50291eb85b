"""CPU: the numpy port of the tensor kernels (tests/pcm_tensor_port.py) against
hand-written values, `import audiotools` stays torch-free, and the
ValueErrors of the tensor interface that need no GPU."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import pcm_tensor_port as port
from pcm_tensor_port import F16, F32, F64, I32, bits

NAN, INF = float("nan"), float("inf")


def one(sample, bps, dtype):
    return port.to_values([sample], 1, bps, dtype)[0, 0]


def back(x, bps, dtype=np.float64):
    return int(port.from_values(np.array([[x]], dtype=dtype), bps)[0])


# ------------------------------------------------------------- PCM -> tensor
def test_float16_keeps_the_subnormal():
    """16-bit sample 1 is 2^-15, below float16's smallest normal 2^-14"""
    v = one(1, 16, F16)
    assert v.dtype == np.float16 and bits(np.array([v]))[0] == 0x0200
    assert float(v) == 2.0 ** -15
    assert bits(np.array([one(-1, 16, F16)]))[0] == 0x8200


def test_float16_rounds_to_nearest_even():
    # 32767 / 32768 = 1 - 2^-15 lies between 1 - 2^-11 and 1.0, nearer 1.0
    assert bits(np.array([one(32767, 16, F16)]))[0] == 0x3C00
    assert bits(np.array([one(-32768, 16, F16)]))[0] == 0xBC00
    # 2049 / 32768: a tie between 2048 and 2050 (11 significant bits) goes to even
    assert float(one(2049, 16, F16)) == 2048.0 / 32768
    assert float(one(2051, 16, F16)) == 2052.0 / 32768
    # the 24-bit 1 is 2^-23: float16's smallest subnormal is 2^-24, so it is kept
    assert float(one(1, 24, F16)) == 2.0 ** -23


@pytest.mark.parametrize("bps", [8, 16, 24])
def test_float32_and_float64_are_exact(bps):
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    for s in (lo, lo + 1, -1, 0, 1, hi - 1, hi):
        for dtype in (F32, F64):
            v = one(s, bps, dtype)
            assert float(v) * (1 << (bps - 1)) == s
        assert one(s, bps, I32) == s
    assert bits(np.array([one(0, bps, F32)]))[0] == 0  # +0.0


def test_planes_and_padding():
    x = np.arange(1, 13, dtype=np.int32)  # 4 frames of 3 channels
    assert port.to_values(x, 3, 16, I32).tolist() == [[1, 4, 7, 10], [2, 5, 8, 11], [3, 6, 9, 12]]
    out = np.full(40, 9.0, dtype=np.float32)
    port.to_tensor_row(out, x, 3, 16, F32, pad_frames=6, out_offset=2, channel_stride=8)
    want = np.full(40, 9.0, dtype=np.float32)
    for c in range(3):
        want[2 + 8 * c:2 + 8 * c + 4] = (x[c::3] / 32768.0).astype(np.float32)
        want[2 + 8 * c + 4:2 + 8 * c + 6] = 0
    assert np.array_equal(bits(out), bits(want))


# ------------------------------------------------------------- tensor -> PCM
@pytest.mark.parametrize("bps", [8, 16, 24])
def test_truncation_toward_zero(bps):
    scale = float(1 << (bps - 1))
    assert back(0.5 / scale, bps) == 0
    assert back(-0.5 / scale, bps) == 0
    assert back(-0.0, bps) == 0
    assert back(1.5 / scale, bps) == 1
    assert back(-1.5 / scale, bps) == -1
    assert back(5e-324, bps) == 0 and back(-5e-324, bps) == 0


def test_minus_one_and_a_half_over_2_15():
    assert back(-1.5 / 2 ** 15, 16) == -1


@pytest.mark.parametrize("bps", [8, 16, 24])
def test_clamps_and_the_cast(bps):
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    assert back(1.0, bps) == hi
    assert back(2.0, bps) == hi
    assert back(-1.0, bps) == lo
    assert back(-2.0, bps) == lo
    assert back(np.nextafter(1.0, 0.0), bps) == hi
    # the x86 cast gives INT_MIN for what does not fit int32: the most negative sample
    assert back(NAN, bps) == lo
    assert back(INF, bps) == lo
    assert back(-INF, bps) == lo
    assert back(1e300, bps) == lo
    # 2^31 / 2^(bps-1) is the first value past int32
    assert back(2.0 ** (32 - bps), bps) == lo
    assert back(np.nextafter(2.0 ** (32 - bps), 0.0), bps) == hi
    for dtype in (np.float16, np.float32):
        assert back(NAN, bps, dtype) == lo and back(INF, bps, dtype) == lo
        assert back(1.0, bps, dtype) == hi
    assert port.from_values(np.array([[hi + 1, lo - 1, 5]], dtype=np.int32), bps).tolist() == [
        hi, lo, 5]


def test_interleave():
    planes = np.array([[0.5, -0.5], [0.25, 0.0], [-1.0, 1.0]])
    assert port.from_values(planes, 16).tolist() == [16384, 8192, -32768, -16384, 0, 32767]
    buf = np.zeros(30, dtype=np.float32)
    buf[3:5], buf[10:12] = [0.5, 0.25], [-0.5, -0.25]
    assert port.from_tensor_row(buf, 3, 7, 2, 2, 8).tolist() == [64, -64, 32, -32]


@pytest.mark.parametrize("bps", [8, 16])
def test_round_trip_of_every_value(bps):
    x = np.arange(-(1 << (bps - 1)), 1 << (bps - 1), dtype=np.int32)
    for dtype in (F32, F64):
        assert np.array_equal(port.from_values(port.to_values(x, 1, bps, dtype), bps), x)


def test_round_trip_24_bits():
    x = np.random.RandomState(24).randint(-(1 << 23), 1 << 23, size=10000).astype(np.int32)
    x[:4] = [-(1 << 23), (1 << 23) - 1, -1, 1]
    for dtype in (F32, F64):
        assert np.array_equal(port.from_values(port.to_values(x, 2, 24, dtype), 24), x)


# ------------------------------------------------------------- the interface
def test_import_audiotools_leaves_torch_out():
    code = ("import sys; import audiotools; assert 'torch' not in sys.modules; "
            "import audiotools.convert, audiotools.pcmconverter; "
            "assert 'torch' not in sys.modules; "
            "f = audiotools.load_batch; assert 'torch' in sys.modules; "
            "assert f is audiotools.tensors.load_batch; "
            "assert audiotools.save_flac_batch and audiotools.pcm_to_tensor "
            "and audiotools.tensor_to_pcm")
    subprocess.run([sys.executable, "-c", code], check=True,
                   env=dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path)))
    import audiotools
    with pytest.raises(AttributeError):
        audiotools.no_such_name


def _wav(path, channels=2, frames=20):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(b"\0" * (2 * channels * frames))
    return str(path)


BAD_TARGETS = [dict(sample_rate=0), dict(channels=0), dict(bits_per_sample=12),
               dict(channels=2, channel_mask=0x7), dict(sample_rate=44100 * 300)]


@pytest.mark.parametrize("target", BAD_TARGETS, ids=[str(sorted(t.items())) for t in BAD_TARGETS])
def test_load_batch_refuses_a_bad_target_before_any_gpu_work(target, tmp_path):
    import audiotools
    with pytest.raises(ValueError):
        audiotools.load_batch([_wav(tmp_path / "a.wav")], **target)


def test_load_batch_refuses_differing_channel_counts(tmp_path):
    import audiotools
    with pytest.raises(ValueError) as e:
        audiotools.load_batch([_wav(tmp_path / "a.wav", 2), _wav(tmp_path / "b.wav", 1),
                               str(tmp_path / "missing.wav")])
    assert "1, 2" in str(e.value) and "channels=" in str(e.value)
    import torch
    with pytest.raises(ValueError):
        audiotools.load_batch([_wav(tmp_path / "c.wav")], dtype=torch.bfloat16)


def test_length_mismatches(tmp_path):
    import torch
    import audiotools
    audio = torch.zeros((3, 2, 10))
    names = [str(tmp_path / ("%d.flac" % k)) for k in range(3)]
    bad = [
        dict(lengths=[10, 10], targets=names, sample_rate=44100),
        dict(lengths=[10, 10, 11], targets=names, sample_rate=44100),
        dict(lengths=[10, 10, -1], targets=names, sample_rate=44100),
        dict(lengths=[10, 10, 10], targets=names[:2], sample_rate=44100),
        dict(lengths=[10, 10, 10], targets=names, sample_rate=[44100, 48000]),
        dict(lengths=[10, 10, 10], targets=names, sample_rate=44100, bits_per_sample=[16] * 4),
        dict(lengths=[10, 10, 10], targets=names, sample_rate=44100, bits_per_sample=12),
        dict(lengths=[10, 10, 10], targets=names, sample_rate=0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            audiotools.save_flac_batch(audio, **kw)
    with pytest.raises(ValueError):
        audiotools.save_flac_batch(audio[0], [10], names[:1], 44100)
    with pytest.raises(ValueError):
        audiotools.tensor_to_pcm(audio, [10, 10], 16)
    with pytest.raises(ValueError):
        audiotools.tensor_to_pcm(audio, [10, 10, 10], [16, 16])
    with pytest.raises(ValueError):
        audiotools.tensor_to_pcm(audio, [10, 10, 10], 25)
    with pytest.raises(ValueError):
        audiotools.tensor_to_pcm(audio.to(torch.int64), [10, 10, 10], 16)
    assert not any((tmp_path / ("%d.flac" % k)).exists() for k in range(3))
    from audiotools.pcmconverter import DevicePcm
    rows = [(DevicePcm(16, 1, 0, 10), 2, 16), (DevicePcm(16, 1, 0, 10), 1, 16)]
    with pytest.raises(ValueError):
        audiotools.pcm_to_tensor(rows)
    with pytest.raises(ValueError):
        audiotools.pcm_to_tensor(rows[:1], frames=9)
