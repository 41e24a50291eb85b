"""CPU: the argument checks of atg_pcm_chain_device / _host come before any
GPU call -- on a machine without a GPU every refusal still gives its own
status and message, with device pointers that are never dereferenced; the
numpy port of a row agrees with oracle_port.convert; and both batch calls
raise PCMConverter's ValueErrors before any GPU work."""
import ctypes

import numpy as np
import pytest

import bad_device
import oracle_port
import pcm_chain_port as port
import signals
import audiotools
from audiotools import _atgpu

INVALID, CAPACITY = _atgpu.ATG_ERR_INVALID, _atgpu.ATG_ERR_CAPACITY
PTR, OUT, DITHER = 0x10000, 0x200000, 0x300000  # never read or written


def row(frames=10, in_channels=2, out_channels=None, in_bps=16, out_bps=16, out_offset=0,
        d_pcm=PTR, fmt=_atgpu.PCM_S32, sample_offset=0, window_offset=0, **kw):
    view = _atgpu.pcm_view(d_pcm, fmt, frames, sample_offset, window_offset)
    oc = in_channels if out_channels is None else out_channels
    return _atgpu.pcm_chain_row(view, in_channels, oc, in_bps, out_bps, out_offset, **kw)


def call(rows, d_out=OUT, out_fmt=_atgpu.PCM_S32, cap=1 << 20, d_dither=DITHER,
         dither_bytes=1 << 20):
    lib = _atgpu.load_library()
    arr = (_atgpu.PcmChainRow * max(1, len(rows)))(*rows)
    st = lib.atg_pcm_chain_device(arr, len(rows), d_out, out_fmt, cap, d_dither, dither_bytes,
                                  None)
    return st, lib.atg_pcm_chain_last_error()


SOUND = dict(out_offset=1024)  # a sound row beside the bad one: every row is checked
REFUSALS = [
    ("no input channels", [row(in_channels=0, out_channels=1)], {}, b"channel count"),
    ("nine input channels", [row(in_channels=9, out_channels=2)], {}, b"channel count"),
    ("no output channels", [row(out_channels=0)], {}, b"channel count"),
    ("nine output channels", [row(out_channels=9, channel_map=[0] * 9)], {}, b"channel count"),
    ("map past the input", [row(out_channels=3, channel_map=[0, 1, 2])], {}, b"map"),
    ("map far past the input", [row(in_channels=8, channel_map=[0, 1, 2, 3, 4, 5, 6, 8])], {},
     b"map"),
    ("no input bits", [row(in_bps=0)], {}, b"bits per sample"),
    ("25 input bits", [row(in_bps=25)], {}, b"bits per sample"),
    ("no output bits", [row(out_bps=0)], {}, b"bits per sample"),
    ("25 output bits", [row(out_bps=25)], {}, b"bits per sample"),
    ("24 bits into int16", [row(in_bps=24, out_bps=24)], dict(out_fmt=_atgpu.PCM_S16), b"S16"),
    ("17 bits into int16", [row(in_bps=16, out_bps=17)], dict(out_fmt=_atgpu.PCM_S16), b"S16"),
    ("int32 output off a boundary", [row(out_offset=6)], {}, b"16-byte"),
    ("int16 output off a boundary", [row(out_offset=4)], dict(out_fmt=_atgpu.PCM_S16),
     b"16-byte"),
    ("output buffer off a boundary", [row()], dict(d_out=OUT + 8), b"16-byte"),
    ("rows overlap", [row(out_offset=1024 + 16)], {}, b"overlap"),
    ("rows overlap at the end", [row(frames=600, out_offset=0)], {}, b"overlap"),
    ("dither range past the bytes", [row(in_bps=24, out_bps=16, dither_bit0=70)],
     dict(dither_bytes=11), b"dither"),
    ("dither range past by one bit", [row(frames=8, in_channels=1, in_bps=16, out_bps=8,
                                          dither_bit0=1)], dict(dither_bytes=1), b"dither"),
    ("dither missing", [row(in_bps=24, out_bps=16)], dict(d_dither=None), b"d_dither"),
    ("output missing", [row()], dict(d_out=None), b"d_out"),
    ("downmix to three", [row(in_channels=6, out_channels=3,
                              channel_op=_atgpu.CHAIN_DOWNMIX)], {}, b"out_channels"),
    ("average to two", [row(in_channels=2, out_channels=2,
                            channel_op=_atgpu.CHAIN_AVERAGE)], {}, b"out_channels"),
    ("downmix mask too wide", [row(in_channels=3, out_channels=2, channel_mask=0x3F,
                                   channel_op=_atgpu.CHAIN_DOWNMIX)], {}, b"mask"),
    ("unknown operation", [row(channel_op=4)], {}, b"operation"),
    ("unknown source format", [row(fmt=2)], {}, b"format"),
    ("unknown output format", [row()], dict(out_fmt=2), b"format"),
    ("source missing", [row(d_pcm=None)], {}, b"NULL"),
    ("int32 source off by 2", [row(d_pcm=PTR + 2)], {}, b"aligned"),
    ("int16 source off by 1", [row(d_pcm=PTR + 1, fmt=_atgpu.PCM_S16)], {}, b"aligned"),
    ("windowed source", [row(window_offset=1)], {}, b"window_offset"),
]


@pytest.mark.parametrize("what,bad,kw,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, bad, kw, word):
    st, msg = call([row(**SOUND)] + bad, **kw)
    assert st == INVALID
    assert word in msg, msg


def test_the_same_rows_pass_when_sound():
    """tables with nothing to convert pass the checks and need no GPU"""
    assert call([])[0] == _atgpu.ATG_OK
    assert call([row(frames=0)], d_out=None, d_dither=None)[0] == _atgpu.ATG_OK
    # a dither range that ends exactly at the last bit is inside
    st, _ = call([row(frames=0, in_bps=16, out_bps=8, dither_bit0=1 << 40)], dither_bytes=0)
    assert st == _atgpu.ATG_OK


def test_capacity():
    st, msg = call([row(frames=10, out_offset=1024)], cap=1024 + 19)
    assert st == CAPACITY and b"out_cap_samples" in msg


def test_null_table():
    lib = _atgpu.load_library()
    assert lib.atg_pcm_chain_device(None, 1, OUT, _atgpu.PCM_S32, 64, None, 0,
                                    None) == INVALID
    assert b"rows" in lib.atg_pcm_chain_last_error()
    assert lib.atg_pcm_chain_device(None, 0, None, _atgpu.PCM_S32, 0, None, 0,
                                    None) == _atgpu.ATG_OK


def test_host_entry_refuses_the_same():
    lib = _atgpu.load_library()
    src = np.zeros(64, dtype=np.int32)
    out = np.zeros(64, dtype=np.int32)
    bad = row(d_pcm=src.ctypes.data, in_channels=9)
    arr = (_atgpu.PcmChainRow * 1)(bad)
    assert lib.atg_pcm_chain_host(0, arr, 1, out.ctypes.data, _atgpu.PCM_S32, 64, None,
                                  0) == INVALID
    assert b"channel count" in lib.atg_pcm_chain_last_error()
    assert lib.atg_pcm_chain_host(0, None, 1, out.ctypes.data, _atgpu.PCM_S32, 64, None,
                                  0) == INVALID
    with pytest.raises(_atgpu.ATGError) as e:
        _atgpu.pcm_chain_host([row(d_pcm=src.ctypes.data, in_bps=24, out_bps=16)], out)
    assert e.value.status == INVALID  # no dither bytes


def test_host_entry_refuses_device_minus_1():
    lib = _atgpu.load_library()
    src = np.zeros(64, dtype=np.int32)
    out = np.zeros(64, dtype=np.int32)
    arr = (_atgpu.PcmChainRow * 1)(row(d_pcm=src.ctypes.data))
    bad_device.check_refused(lib.atg_pcm_chain_host(-1, arr, 1, out.ctypes.data, _atgpu.PCM_S32,
                                                    64, None, 0), "pcm_chain")
    # the rows are judged first
    arr[0].in_channels = 9
    assert lib.atg_pcm_chain_host(-1, arr, 1, out.ctypes.data, _atgpu.PCM_S32, 64, None,
                                  0) == INVALID
    assert b"channel count" in lib.atg_pcm_chain_last_error()


def test_struct_size_and_tile():
    assert ctypes.sizeof(_atgpu.PcmChainRow) == 88
    t = _atgpu.pcm_chain_tile_samples()
    assert t > 0 and t % 8 == 0
    for ic, oc in [(1, 1), (2, 2), (6, 2), (3, 3), (7, 1), (1, 8)]:
        f = _atgpu.pcm_chain_tile_frames(ic, oc)
        assert f % 8 == 0 and 0 < f * max(ic, oc) <= t
    assert set(_atgpu.pcm_chain_kernel_times()) <= {"chain"}


# ------------------------------------------------------------------ the port
@pytest.mark.parametrize("frames", [0, 1, 4095, 4096, 4097, 9000])
def test_port_bits_agree_with_oracle(frames):
    x = signals.make("noise", frames, 2, 24, seed=frames + 1)
    rng = np.random.RandomState(frames)
    dither = rng.bytes(frames * 2 // 8 + 2)
    want = oracle_port.convert(oracle_port.CONV_BPS, x, 2, 24, 16, dither=dither)
    got = port.convert_row(x, 2, port.MAP, 24, 16, dither=dither)
    assert np.array_equal(got, want)
    # a bit offset is the same stream read from further on
    shifted = b"\xA5" + dither
    bits = np.unpackbits(np.frombuffer(shifted, dtype=np.uint8))
    moved = np.packbits(np.concatenate([np.zeros(3, np.uint8), bits[8:]])).tobytes()
    assert np.array_equal(port.convert_row(x, 2, port.MAP, 24, 16, dither=moved, bit0=3), want)
    assert np.array_equal(port.convert_row(x, 2, port.MAP, 16, 24),
                          oracle_port.convert(oracle_port.CONV_BPS, x, 2, 16, 24))


@pytest.mark.parametrize("ch,mask", [(3, 0x7), (4, 0x33), (5, 0x37), (6, 0x3F), (8, 0),
                                     (6, 0), (4, 0)])
def test_port_downmix_and_average_agree_with_oracle(ch, mask):
    x = signals.make("noise", 1000, ch, 16, seed=ch)
    two = oracle_port.convert(oracle_port.CONV_DOWNMIX, x, ch, 16, mask=mask)
    assert np.array_equal(port.convert_row(x, ch, port.DOWNMIX, 16, 16, mask=mask), two)
    one = oracle_port.convert(oracle_port.CONV_AVERAGE, two, 2, 16)
    assert np.array_equal(port.convert_row(x, ch, port.DOWNMIX_AVERAGE, 16, 16, mask=mask), one)
    assert np.array_equal(port.convert_row(x, ch, port.AVERAGE, 16, 16),
                          oracle_port.convert(oracle_port.CONV_AVERAGE, x, ch, 16))


def test_port_map():
    x = np.arange(12, dtype=np.int32) + 1
    assert port.convert_row(x, 3, port.MAP, 16, 16, channel_map=[2, None, 0, 0]).tolist() == [
        3, 0, 1, 1, 6, 0, 4, 4, 9, 0, 7, 7, 12, 0, 10, 10]
    assert np.array_equal(port.convert_row(x, 3, port.MAP, 16, 16), x)


# ------------------------------------------------ PCMConverter's early errors
class _Reader(object):
    def __init__(self, channels=2, channel_mask=0x3, bits_per_sample=16, sample_rate=44100):
        self.channels, self.channel_mask = channels, channel_mask
        self.bits_per_sample, self.sample_rate = bits_per_sample, sample_rate


BAD_TARGETS = [
    dict(sample_rate=0), dict(sample_rate=-5), dict(channels=0), dict(bits_per_sample=12),
    dict(bits_per_sample=32), dict(channels=2, channel_mask=0x7),
    dict(channels=3, channel_mask=0x3),
]


@pytest.mark.parametrize("target", BAD_TARGETS, ids=[str(sorted(t.items())) for t in BAD_TARGETS])
def test_batch_calls_raise_what_pcmconverter_raises(target, tmp_path):
    full = dict(sample_rate=44100, channels=2, channel_mask=0x3, bits_per_sample=16)
    full.update(target)
    with pytest.raises(ValueError) as want:
        audiotools.PCMConverter(_Reader(), full["sample_rate"], full["channels"],
                                full["channel_mask"], full["bits_per_sample"])
    x = np.zeros(20, dtype=np.int32)
    with pytest.raises(ValueError) as got:
        audiotools.convert_pcm_batch([x], [(2, 0x3, 16, 44100)], **full)
    assert str(got.value) == str(want.value)
    # a WAV image: opened on the host, never decoded
    import wave
    src = str(tmp_path / "a.wav")
    with wave.open(src, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(b"\0" * 40)
    with pytest.raises(ValueError) as got:
        audiotools.convert_files_batch([src], [str(tmp_path / "a.flac")], **full)
    assert str(got.value) == str(want.value)
    assert not (tmp_path / "a.flac").exists()


def test_remask_mismatch_and_resampler_ratio_raise_early():
    # the remasking branch: fewer channels, neither mono nor stereo
    with pytest.raises(ValueError) as want:
        audiotools.PCMConverter(_Reader(6, 0x3F, 16, 44100), 44100, 4, 0x7, 16)
    with pytest.raises(ValueError) as got:
        audiotools.convert_pcm_batch([np.zeros(12, np.int32)], [(6, 0x3F, 16, 44100)],
                                     channels=4, channel_mask=0x7)
    assert str(got.value) == str(want.value)
    with pytest.raises(ValueError) as got:
        audiotools.convert_pcm_batch([np.zeros(4, np.int32)], [(2, 0x3, 16, 100)],
                                     sample_rate=44100)
    assert "SRC ratio" in str(got.value)
    with pytest.raises(ValueError):
        audiotools.convert_pcm_batch([np.zeros(5, np.int32)], [(2, 0x3, 16, 44100)])
    with pytest.raises(ValueError):
        audiotools.convert_pcm_batch([np.zeros(4, np.int64)], [(2, 0x3, 16, 44100)])
