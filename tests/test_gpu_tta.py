"""GPU parity: libatgpu's True Audio encoder (tta_encode.hip) against the
reference encoder's recorded output (tests/golden/tta_vectors.json: sha256 of
the files oracle/_ref/ttaenc wrote, and their seektables) and against
tests/tta_port.py on mixed batches; the encode_tta interface."""
import hashlib
import io
import json
import os
from collections import defaultdict

import numpy as np
import pytest

import signals
import tta_cases
import tta_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "tta_vectors.json")))


def gpu_encode(pcms, channels, bps, rate, sizes=None, **kw):
    """-> per track (frames bytes, frame sizes)"""
    from audiotools import _atgpu
    enc = _atgpu.tta_encoder()
    tracks, start = [], 0
    for k, p in enumerate(pcms):
        n = len(p) // channels
        tracks.append((start, n, sizes[k] if sizes else None))
        start += n
    pcm = np.concatenate(pcms).astype(np.int16 if bps <= 16 else np.int32)
    out, res, fsb = enc.encode(pcm, tracks, channels, bps, rate, **kw)
    got = []
    for r, p in zip(res, pcms):
        assert r.status == 0 and r.pcm_frames == len(p) // channels
        fs = [int(x) for x in fsb[r.first_frame:r.first_frame + r.n_frames]]
        assert sum(fs) == r.bytes
        got.append((out[r.out_offset:r.out_offset + r.bytes].tobytes(), fs))
    return got


def image(frames, sizes, channels, bps, rate, total):
    return tta_port.header(channels, bps, rate, total) + tta_port.seektable(sizes) + frames


def _groups():
    g = defaultdict(list)
    for case in tta_cases.encoder_cases():
        g[(case[1], case[2], case[3])].append(case)
    return sorted(g.items())


@pytest.mark.parametrize("key,cases", _groups(), ids=lambda x: str(x) if isinstance(x, tuple)
                         else None)
def test_encoder_vectors_batch(key, cases):
    """every vector of one format in one batch, the kinds mixed: header +
    seektable + frames is the file the reference wrote"""
    ch, bps, rate = key
    got = gpu_encode([c[4] for c in cases], ch, bps, rate)
    for (name, _, _, _, x), (frames, sizes) in zip(cases, got):
        v = G["encoder"][name]
        assert sizes == v["frame_sizes"], name
        img = image(frames, sizes, ch, bps, rate, len(x) // ch)
        assert len(img) == v["bytes"], name
        assert hashlib.sha256(img).hexdigest() == v["sha256"], name


def test_mixed_batch_against_port():
    """6 tracks of unequal length, byte for byte"""
    ch, bps, rate = 2, 16, tta_cases.RATE
    lens = (5, tta_cases.BLOCK + 17, 1, 3 * tta_cases.BLOCK, 777, 2 * tta_cases.BLOCK - 1)
    kinds = ("tone", "noise", "chirp", "tone", "silence", "noise")
    pcms = [signals.make(k, n, ch, bps, seed=n) for k, n in zip(kinds, lens)]
    want = tta_port.encode_frames_many([(p, ch, bps, rate, None) for p in pcms])
    for (frames, sizes), w in zip(gpu_encode(pcms, ch, bps, rate), want):
        assert sizes == [len(f) for f in w]
        assert frames == b"".join(w)


@pytest.mark.parametrize("ch,bps,loud", [(1, 16, 32), (2, 16, 32), (1, 24, 4), (2, 24, 4)])
def test_unbounded_frame_between_neighbours(ch, bps, loud):
    """a frame many times its raw size between two ordinary tracks: the
    output is sized from the length pass (the first offer of the raw PCM size
    is refused with the size needed), and no frame writes into its neighbour"""
    rate = tta_cases.RATE
    name = "quiet_loud_c%d_b%d" % (ch, bps)
    a = signals.make("tone", 1000, ch, bps, seed=5)
    b = tta_cases.quiet_then_full_scale(ch, bps, loud)
    c = signals.make("noise", tta_cases.BLOCK + 3, ch, bps, seed=6)
    got = gpu_encode([a, b, c], ch, bps, rate)
    v = G["encoder"][name]
    assert got[1][1] == v["frame_sizes"]
    assert v["bytes"] > len(b) * (bps // 8)  # larger than its PCM
    img = image(got[1][0], got[1][1], ch, bps, rate, len(b) // ch)
    assert hashlib.sha256(img).hexdigest() == v["sha256"]
    want = tta_port.encode_frames_many([(a, ch, bps, rate, None), (c, ch, bps, rate, None)])
    assert got[0][0] == b"".join(want[0])
    assert got[2][0] == b"".join(want[1])


def test_capacity_is_reported_not_overrun():
    """a buffer that is too small: ATG_ERR_CAPACITY and the size needed, and
    not one byte of the buffer is written"""
    import ctypes
    from audiotools import _atgpu
    enc = _atgpu.tta_encoder()
    x = signals.make("noise", 4000, 2, 16, seed=9).astype(np.int16)
    arr, n, keep = _atgpu._track_array([(0, 4000)])
    res = (_atgpu.TtaTrackResult * 1)()
    need = ctypes.c_uint64()
    out = np.full(4096, 0xA5, np.uint8)
    st = enc.lib.atg_tta_encode_host(
        enc.handle, x.ctypes.data_as(ctypes.c_void_p), _atgpu.PCM_S16, arr, n, 2, 16,
        tta_cases.RATE, out.ctypes.data_as(ctypes.c_void_p), 1000, res, None, 0,
        ctypes.byref(need))
    assert st == _atgpu.ATG_ERR_CAPACITY
    want = tta_port.encode_frames(x, 2, 16, tta_cases.RATE)
    assert need.value == sum(len(f) for f in want) > 1000
    assert (out == 0xA5).all()
    # exactly enough is enough
    out2 = np.full(need.value + 8, 0xA5, np.uint8)
    st = enc.lib.atg_tta_encode_host(
        enc.handle, x.ctypes.data_as(ctypes.c_void_p), _atgpu.PCM_S16, arr, n, 2, 16,
        tta_cases.RATE, out2.ctypes.data_as(ctypes.c_void_p), need.value, res, None, 0,
        ctypes.byref(need))
    assert st == 0
    assert out2[:need.value].tobytes() == b"".join(want)
    assert (out2[need.value:] == 0xA5).all()


def test_capacity_on_the_device_path():
    """atg_tta_encode_device with a device buffer that is too small: the size
    needed comes back and the buffer keeps every byte it had; with exactly
    that size the images are written and nothing after them"""
    import torch
    from audiotools import _atgpu
    enc = _atgpu.tta_encoder()
    ch, bps, rate = 2, 16, tta_cases.RATE
    xs = [signals.make("noise", 4000, ch, bps, seed=9),
          tta_cases.quiet_then_full_scale(ch, bps, 32),
          signals.make("tone", 700, ch, bps, seed=10)]
    tracks, start = [], 0
    for x in xs:
        tracks.append((start, len(x) // ch))
        start += len(x) // ch
    dev = torch.device("cuda:0")
    d_pcm = torch.from_numpy(np.concatenate(xs).astype(np.int16)).to(dev)
    d_out = torch.full((65536,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    want = [b"".join(w) for w in
            tta_port.encode_frames_many([(x, ch, bps, rate, None) for x in xs])]
    with pytest.raises(_atgpu.ATGError) as e:
        enc.encode_device(d_pcm.data_ptr(), _atgpu.PCM_S16, tracks, ch, bps, rate,
                          d_out.data_ptr(), 20000)
    assert e.value.status == _atgpu.ATG_ERR_CAPACITY
    need = e.value.needed
    assert 20000 < need <= 65536 - 64
    assert bool((d_out == 0xA5).all())
    fsb = np.zeros(3, np.uint32)
    res, need2 = enc.encode_device(d_pcm.data_ptr(), _atgpu.PCM_S16, tracks, ch, bps, rate,
                                   d_out.data_ptr(), need, fsb)
    assert need2 == need
    out = d_out.cpu().numpy()
    for r, w in zip(res, want):
        assert out[r.out_offset:r.out_offset + r.bytes].tobytes() == w
    assert res[-1].out_offset + res[-1].bytes == need
    assert (out[need:] == 0xA5).all()
    assert [int(v) for v in fsb] == [len(w) for w in want]
    # too few frame_bytes entries is a bad argument, not a capacity report
    with pytest.raises(_atgpu.ATGError) as e:
        enc.encode_device(d_pcm.data_ptr(), _atgpu.PCM_S16, tracks, ch, bps, rate,
                          d_out.data_ptr(), 65536, fsb[:2])
    assert e.value.status == _atgpu.ATG_ERR_INVALID


class SizedReader(object):
    """a PCMReader that ignores the size asked for"""

    def __init__(self, samples, channels, bps, rate, reads):
        from audiotools import pcm
        self.pcm = pcm
        self.x = np.asarray(samples, np.int32)
        self.channels, self.bits_per_sample, self.sample_rate = channels, bps, rate
        self.channel_mask = 0
        self.reads = list(reads)
        self.pos = 0

    def read(self, n):
        k = self.reads.pop(0) if self.reads else 0
        a = self.pos * self.channels
        self.pos += k
        return self.pcm.FrameList._wrap(self.x[a:a + k * self.channels].copy(), self.channels,
                                        self.bits_per_sample)

    def close(self):
        pass


def test_encode_tta_odd_reads():
    """every read is one frame, whatever its size"""
    from audiotools import encoders
    reads = [8359, 7, 1000, 8359, 3]
    ch, bps, rate = 2, 16, tta_cases.RATE
    x = signals.make("tone", sum(reads), ch, bps, seed=3)
    f = io.BytesIO()
    sizes = encoders.encode_tta(f, SizedReader(x, ch, bps, rate, reads))
    want = tta_port.encode_frames(x, ch, bps, rate, reads)
    assert len(sizes) == 5 and sizes == [len(w) for w in want]
    assert f.getvalue() == b"".join(want)


def test_encode_tta_batch_writes_each_file():
    from audiotools import encoders
    ch, bps, rate = 1, 8, tta_cases.RATE
    xs = [signals.make("tone", n, ch, bps, seed=n) for n in (100, tta_cases.BLOCK + 1)]
    files = [io.BytesIO(), io.BytesIO()]
    logs = encoders.encode_tta_batch(
        files, [SizedReader(x, ch, bps, rate, [tta_cases.BLOCK] * 3) for x in xs])
    for x, f, log in zip(xs, files, logs):
        want = tta_port.encode_frames(x, ch, bps, rate)
        assert log == [len(w) for w in want] and f.getvalue() == b"".join(want)


def test_encode_tta_errors():
    from audiotools import encoders

    class Broken(SizedReader):
        def read(self, n):
            raise ValueError("reader broke")

    x = signals.make("tone", 10, 2, 16)
    with pytest.raises(TypeError):
        encoders.encode_tta("not a file", SizedReader(x, 2, 16, tta_cases.RATE, [10]))
    with pytest.raises(ValueError):
        encoders.encode_tta(io.BytesIO(), Broken(x, 2, 16, tta_cases.RATE, [10]))


def test_kernel_times_named():
    from audiotools import _atgpu
    gpu_encode([signals.make("tone", 100, 2, 16)], 2, 16, tta_cases.RATE)
    t = _atgpu.tta_encoder().kernel_times()
    assert set(t) == {"tta_chain", "tta_size", "tta_pack", "tta_crc", "tta_total"}
