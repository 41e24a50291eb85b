"""The eight components without a handle over their shared scaffold
(csrc/host_common.h: DeviceContexts, StageTimes, use_device), the counterpart
of test_gpu_handles.py.  Each component's smallest real call:

  pcm_bytes    one run of 64 samples, 16-bit little-endian signed, unpack then pack
  pcm_compare  one pair of 100 stereo frames, equal, then with one sample changed
  pcm_chain    one row, 100 frames, stereo, 16 to 16 bits
  accuraterip  one track of 5 x 588 frames, max_offset 0
  replaygain   one stereo 16-bit 44.1 kHz track of 22,050 frames
  resample     one stereo 24-bit track of 4,096 frames, 44,100 -> 48,000
  aob_decode   the one-sector PCM title of dvda_cases
  mlp_decode   the one-unit title of mlp_cases

Times are per thread: a fresh thread reads {}, after its call the component's
stages in order, and a thread started afterwards reads {} again.  Results
under concurrency: four calls of 1, 3, 2 and 5 times the shape (the context's
buffers regrow between them) with four seeds, first on one thread, then on
four threads at once on device 0, each in its own rotation with its own
buffers on the null stream; every output array and result struct must equal
the serial one bit for bit.  Not exercised on more than one device."""
import ctypes
import math
import threading

import numpy as np
import pytest

import dvda_build
import dvda_cases
import mlp_cases
import mlp_port
from audiotools import _atgpu

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 2, 5)
S32 = _atgpu.PCM_S32


def dev(a):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()
    torch.cuda.synchronize()
    return t


def host(t):
    return t.cpu().numpy()


def raw(structs):
    """result structs as their bytes"""
    return b"".join(ctypes.string_at(ctypes.addressof(r), ctypes.sizeof(r)) for r in structs)


def noise(seed, n, bits, dtype=np.int32):
    rng = np.random.default_rng(seed)
    return rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=n).astype(dtype)


# A job: make(seed, k) uploads the inputs of a call k times the shape and
# allocates its outputs (on the calling thread, before any worker starts);
# run(job) makes the call and returns what comes back on the host;
# fetch(job) downloads the output arrays afterwards.
class PcmBytes:
    times = ["pack"]  # of the last launch

    @staticmethod
    def make(seed, k):
        n = 64 * k
        data = noise(seed, n, 16, np.int16).astype("<i2").view(np.uint8)
        return dict(n=n, data=dev(data), pcm=dev(np.full(n, 77, np.int32)),
                    back=dev(np.zeros(2 * n, np.uint8)), want=data)

    @staticmethod
    def run(j):
        lay, runs = _atgpu.pcm_layout(2, False, True), [(0, j["n"], 0)]
        _atgpu.pcm_unpack_device(j["data"].data_ptr(), 2 * j["n"], lay, runs, j["pcm"].data_ptr(),
                                 S32, j["n"])
        unpack = _atgpu.pcm_bytes_kernel_times()
        _atgpu.pcm_pack_device(j["pcm"].data_ptr(), S32, j["n"], lay, runs, j["back"].data_ptr(),
                               2 * j["n"])
        return list(unpack)

    @staticmethod
    def fetch(j):
        back = host(j["back"])
        assert np.array_equal(back, j["want"])
        return [host(j["pcm"]), back]


class PcmCompare:
    times = ["compare", "probe"]

    @staticmethod
    def make(seed, k):
        frames = 100 * k
        a = noise(seed, 2 * frames, 16)
        b, at = a.copy(), seed * 37 % (2 * frames)
        b[at] ^= 1
        return dict(frames=frames, a=dev(a), same=dev(a), b=dev(b), at=at // 2)

    @staticmethod
    def run(j):
        def pair(t):
            a, b = (_atgpu.pcm_view(x.data_ptr(), S32, j["frames"]) for x in (j["a"], t))
            return [_atgpu.pcm_pair(a, b, j["frames"], 2)]

        got = _atgpu.pcm_compare_device(pair(j["same"])) + _atgpu.pcm_compare_device(pair(j["b"]))
        assert got == [None, j["at"]]
        return got

    @staticmethod
    def fetch(j):
        return []


class PcmChain:
    times = ["chain"]

    @staticmethod
    def make(seed, k):
        x = noise(seed, 200 * k, 16)
        return dict(frames=100 * k, x=dev(x), out=dev(np.full(200 * k, 77, np.int32)), want=x)

    @staticmethod
    def run(j):
        row = _atgpu.pcm_chain_row(_atgpu.pcm_view(j["x"].data_ptr(), S32, j["frames"]), 2, 2, 16,
                                   16, 0)
        _atgpu.pcm_chain_device([row], j["out"].data_ptr(), S32, 2 * j["frames"])

    @staticmethod
    def fetch(j):
        out = host(j["out"])
        assert np.array_equal(out, j["want"])
        return [out]


class AccurateRip:
    times = None

    @staticmethod
    def make(seed, k):
        frames = 5 * 588 * k
        return dict(frames=frames, x=dev(noise(seed, 2 * frames, 16, np.int16)))

    @staticmethod
    def run(j):
        res, table = _atgpu.accuraterip_device(j["x"].data_ptr(), _atgpu.PCM_S16,
                                               [_atgpu.ar_track(0, j["frames"])], 0)
        assert res[0].status == 0
        return raw(res), table.tobytes()

    @staticmethod
    def fetch(j):
        return []


class ReplayGain:
    times = None

    @staticmethod
    def make(seed, k):
        frames = 22050 * k
        return dict(frames=frames, x=dev(noise(seed, 2 * frames, 16)))

    @staticmethod
    def run(j):
        res, peaks = _atgpu.replaygain_device(
            j["x"].data_ptr(), [_atgpu.RgTrack(0, j["frames"], 2, 16, 44100, 0)], 1)
        assert res[0].status == 0 and res[0].title_peak > 0
        return raw(res), peaks

    @staticmethod
    def fetch(j):
        return []


class Resample:
    times = ["rs_positions", "rs_filter"]

    @staticmethod
    def make(seed, k):
        frames = 4096 * k
        n_out = _atgpu.resample_output_frames(frames, 2, 44100, 48000)
        return dict(frames=frames, n_out=n_out, x=dev(noise(seed, 2 * frames, 24)),
                    out=dev(np.full(2 * n_out, 77, np.int32)))

    @staticmethod
    def run(j):
        offs, cnt = _atgpu.resample_device(j["x"].data_ptr(), j["out"].data_ptr(), 2 * j["n_out"],
                                           [(0, j["frames"], 44100, 48000)], 2, 24)
        assert list(offs) == [0] and list(cnt) == [j["n_out"]]
        return offs.tobytes(), cnt.tobytes()

    @staticmethod
    def fetch(j):
        return [host(j["out"])]


class Aob:
    times = ["sectors", "layout", "pcm"]

    @staticmethod
    def make(seed, k):
        built = [dvda_build.aob_image(dvda_cases.spec(seed * 8 + i, 16, 2, [2001]))
                 for i in range(k)]
        data = np.frombuffer(b"".join(img for img, _ in built), dtype=np.uint8)
        return dict(k=k, nbytes=data.nbytes, data=dev(data), cap=1024 * k,
                    out=dev(np.full(1024 * k, 77, np.int32)), want=[x for _, x in built])

    @staticmethod
    def run(j):
        res = _atgpu.aob_decode_device(j["data"].data_ptr(), j["nbytes"],
                                       [(2048 * i, 1) for i in range(j["k"])],
                                       j["out"].data_ptr(), S32, j["cap"])
        j["res"] = res
        return raw(res)

    @staticmethod
    def fetch(j):
        out = host(j["out"])
        for r, x in zip(j["res"], j["want"]):
            assert r.status == _atgpu.DVDA_OK and r.good_frames * r.channels == len(x)
            assert np.array_equal(out[r.sample_offset:r.sample_offset + len(x)], x)
        return [out]


class Mlp:
    times = ["sectors", "layout", "gather", "walk", "check", "parse", "resolve", "store",
             "filter", "output"]

    @staticmethod
    def make(seed, k):
        imgs = [mlp_cases.image_of(mlp_cases.spec("one-unit", seed * 8 + i, 16, 1, units=1,
                                                  frames=8, payloads=[2000]))[0] for i in range(k)]
        data = np.frombuffer(b"".join(imgs), dtype=np.uint8)
        titles, pos = [], 0
        for img in imgs:
            titles.append((pos, len(img) // 2048))
            pos += len(img)
        return dict(titles=titles, nbytes=data.nbytes, data=dev(data), cap=16 * k,
                    out=dev(np.full(16 * k, 77, np.int32)),
                    want=[mlp_port.decode(img)[1] for img in imgs])

    @staticmethod
    def run(j):
        res = _atgpu.mlp_decode_device(j["data"].data_ptr(), j["nbytes"], j["titles"],
                                       j["out"].data_ptr(), S32, j["cap"])
        assert all(r.good_frames == 8 and r.channels == 1 for r in res)
        j["res"] = res
        return raw(res)

    @staticmethod
    def fetch(j):
        out = host(j["out"])
        for r, x in zip(j["res"], j["want"]):
            assert np.array_equal(out[r.sample_offset:r.sample_offset + 8], x)
        return [out]


COMPONENTS = [PcmBytes, PcmCompare, PcmChain, AccurateRip, ReplayGain, Resample, Aob, Mlp]
TIMES_OF = {PcmBytes: _atgpu.pcm_bytes_kernel_times, PcmCompare: _atgpu.pcm_compare_kernel_times,
            PcmChain: _atgpu.pcm_chain_kernel_times, Resample: _atgpu.resample_kernel_times,
            Aob: _atgpu.aob_kernel_times, Mlp: _atgpu.mlp_kernel_times}


def in_thread(fn):
    """fn() on a fresh thread -> its return value; its exception re-raised"""
    box = {}

    def body():
        try:
            box["value"] = fn()
        except BaseException as e:  # handed to the caller
            box["error"] = e

    t = threading.Thread(target=body)
    t.start()
    t.join(60)
    assert not t.is_alive(), "the call did not return within 60 s"
    if "error" in box:
        raise box["error"]
    return box["value"]


@pytest.mark.parametrize("comp", sorted(TIMES_OF, key=COMPONENTS.index), ids=lambda c: c.__name__)
def test_times_are_per_thread(gpu_engine, comp):
    times = TIMES_OF[comp]
    job = comp.make(1, 1)

    def call():
        before = times()
        first = comp.run(job)
        return before, first, times()

    before, first, after = in_thread(call)
    assert before == {}
    if comp is PcmBytes:
        assert first == ["unpack"]
    assert list(after) == comp.times
    print(comp.__name__, after)
    for v in after.values():
        assert math.isfinite(v) and v >= 0
    assert in_thread(times) == {}
    comp.fetch(job)


def results(comp, jobs, order):
    out = {}
    for i in order:
        out[i] = comp.run(jobs[i])
    return out


@pytest.mark.parametrize("comp", COMPONENTS, ids=lambda c: c.__name__)
def test_results_under_concurrency(gpu_engine, comp):
    def jobs():
        return [comp.make(seed + 1, k) for seed, k in enumerate(SIZES)]

    serial = jobs()
    want = results(comp, serial, range(4))
    want_arrays = [comp.fetch(j) for j in serial]

    mine = [jobs() for _ in range(4)]
    got, errors = [None] * 4, []

    def worker(t):
        try:
            got[t] = results(comp, mine[t], [(t + i) % 4 for i in range(4)])
        except BaseException as e:  # reported below
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    # a thread still running: fail here, before any more GPU work
    assert not any(t.is_alive() for t in threads), "a worker did not return within 60 s"
    assert not errors, errors
    for t in range(4):
        assert got[t] == want, t
        for i in range(4):
            for a, b in zip(comp.fetch(mine[t][i]), want_arrays[i]):
                assert np.array_equal(a, b), (t, i)


def test_resample_host_refuses_a_bad_index(gpu_engine):
    """on a machine with a device the index itself is judged"""
    with pytest.raises(_atgpu.ATGError) as e:
        _atgpu.resample_host(noise(1, 128, 24), [(0, 64, 44100, 48000)], 2, 24, device=-1)
    assert e.value.status == _atgpu.ATG_ERR_INVALID
    assert "device index out of range" in str(e.value)
