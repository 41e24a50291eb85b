#!/usr/bin/env python3
"""Measurements of the packed-PCM kernels (csrc/pcm_bytes.hip) ->
profiles/pcm_bytes_bench.json.

    python3 tools/pcm_bytes_bench.py [--tracks 1024] [--seconds 10] [--out FILE]

runs three steps, each a child process under its own `timeout`, one after
the other, and stops at the first that fails:

  kernel  unpack and pack of --tracks tracks x --seconds s of 44.1 kHz stereo,
          16-bit and 24-bit big endian: kernel time from
          atg_pcm_bytes_kernel_times, as TB/s of packed + integer bytes and
          as a fraction of 8 TB/s
  upload  host buffer -> device-resident integer PCM: the packed bytes
          uploaded and unpacked on the device, against what the parent does
          for the same bytes, FrameList(bytes, 2, bps, True, True) track by
          track on the host and an int32 upload; alternating, four tracks
          compared after the clock
  flac    encode_flac_files_batch against encode_flac_batch over WaveReaders
          on the same 16-bit and 24-bit WAV files, alternating

--step NAME runs one of them in this process and prints its JSON.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-audio-tools_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HBM_TBS = 8.0
RATE, CH = 44100, 2


def stats(ms):
    ms = sorted(ms)
    return {"n": len(ms), "min_ms": round(ms[0], 3), "median_ms": round(ms[len(ms) // 2], 3),
            "max_ms": round(ms[-1], 3)}


def packed_batch(tracks, seconds, width, seed):
    """random big-endian packed samples, tracks back to back from byte 5"""
    from audiotools import _atgpu
    n = RATE * seconds * CH
    rng = np.random.default_rng(seed)
    group = 8
    lead = 5
    cap = (lead + tracks * n * width + 15) // 16 * 16
    image = rng.integers(0, 256, cap, dtype=np.uint8)
    slot = (n + group - 1) // group * group
    runs = [(lead + t * n * width, n, t * slot) for t in range(tracks)]
    return image, _atgpu.pcm_runs(runs), runs, cap, tracks * slot


def step_kernel(a):
    import torch
    torch.cuda.init()
    from audiotools import _atgpu
    eng = _atgpu.engine()
    out = {}
    for bps in (16, 24):
        width = bps // 8
        image, table, runs, cap, n_samples = packed_batch(a.tracks, a.seconds, width, bps)
        fmt, isize = (_atgpu.PCM_S16, 2) if bps == 16 else (_atgpu.PCM_S32, 4)
        lay = _atgpu.pcm_layout(width, True, True)
        d_bytes, d_pcm = eng.device_alloc(cap), eng.device_alloc(n_samples * isize)
        d_back = eng.device_alloc(cap)
        try:
            eng.copy_to_device(d_bytes, image)
            un, pk = [], []
            for k in range(a.calls + 2):
                _atgpu.pcm_unpack_device(d_bytes, cap, lay, table, d_pcm, fmt, n_samples)
                un.append(_atgpu.pcm_bytes_kernel_times()["unpack"])
                _atgpu.pcm_pack_device(d_pcm, fmt, n_samples, lay, table, d_back, cap)
                pk.append(_atgpu.pcm_bytes_kernel_times()["pack"])
            back = eng.copy_to_host(np.empty(cap, dtype=np.uint8), d_back)
            lo, hi = runs[0][0], runs[-1][0] + runs[-1][1] * width
            exact = bool(np.array_equal(back[lo:hi], image[lo:hi]))
        finally:
            for d in (d_bytes, d_pcm, d_back):
                eng.device_free(d)
        samples = a.tracks * RATE * a.seconds * CH
        nbytes = samples * (width + isize)
        res = {"samples": samples, "algorithmic_bytes": nbytes,
               "pack_of_unpack_restores_the_bytes": exact}
        for name, ms in (("unpack", un[2:]), ("pack", pk[2:])):
            s = stats(ms)
            s["tb_per_s"] = round(nbytes / (s["median_ms"] * 1e-3) / 1e12, 3)
            s["fraction_of_8_tb_per_s"] = round(s["tb_per_s"] / HBM_TBS, 3)
            res[name] = s
        out["%d-bit big endian" % bps] = res
    return out


def step_upload(a):
    import torch
    torch.cuda.init()
    from audiotools import _atgpu, pcm
    eng = _atgpu.engine()
    out = {}
    for bps in (16, 24):
        width = bps // 8
        image, table, runs, cap, n_samples = packed_batch(a.tracks, a.seconds, width, 100 + bps)
        lay = _atgpu.pcm_layout(width, True, True)
        n = runs[0][1]
        d_bytes, d_pcm = eng.device_alloc(cap), eng.device_alloc(n_samples * 4)
        d_old = eng.device_alloc(a.tracks * n * 4)
        new_ms, old_ms = [], []
        try:
            calls = a.calls if bps == 16 else a.parent_calls_24
            for k in range(calls + 1):
                t0 = time.perf_counter()
                eng.copy_to_device(d_bytes, image)
                _atgpu.pcm_unpack_device(d_bytes, cap, lay, table, d_pcm, _atgpu.PCM_S32, n_samples)
                new_ms.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                parts = [pcm.FrameList(image[off:off + n * width], CH, bps, True, True).samples
                         for off, _, _ in runs]
                host = np.concatenate(parts)
                eng.copy_to_device(d_old, host)
                old_ms.append((time.perf_counter() - t0) * 1e3)
            same = True
            for t in (0, 1, a.tracks // 2, a.tracks - 1):
                got = eng.copy_to_host(np.empty(n, dtype=np.int32), d_pcm + runs[t][2] * 4)
                same = same and bool(np.array_equal(got, parts[t]))
        finally:
            for d in (d_bytes, d_pcm, d_old):
                eng.device_free(d)
        out["%d-bit big endian" % bps] = {
            "packed_bytes": a.tracks * n * width, "int32_bytes": a.tracks * n * 4,
            "device_unpack": stats(new_ms[1:]), "host_framelist_then_int32_upload": stats(old_ms[1:]),
            "four_tracks_equal": same}
    return out


def step_flac(a):
    import torch
    torch.cuda.init()
    import audiotools
    import oracle_port
    import signals
    from audiotools import encoders
    from test_aiff import Reader
    preset = dict(oracle_port.PRESETS["8"])
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for bps in (16, 24):
            frames = RATE * a.seconds
            srcs = []
            for t in range(a.flac_tracks):
                p = os.path.join(tmp, "in%d_%d.wav" % (bps, t))
                x = signals.make("tone" if t % 2 else "noise", frames, CH, bps, seed=t + 1)
                audiotools.WaveAudio.from_pcm(p, Reader(x, CH, bps, RATE, step=1 << 20))
                srcs.append(audiotools.WaveAudio(p))
            new = [os.path.join(tmp, "new%d.flac" % t) for t in range(a.flac_tracks)]
            old = [os.path.join(tmp, "old%d.flac" % t) for t in range(a.flac_tracks)]
            new_ms, old_ms = [], []
            for k in range(a.flac_calls + 1):
                t0 = time.perf_counter()
                encoders.encode_flac_files_batch(new, srcs, **preset)
                new_ms.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                encoders.encode_flac_batch(old, [s.to_pcm() for s in srcs], **preset)
                old_ms.append((time.perf_counter() - t0) * 1e3)
            same = all(open(x, "rb").read() == open(y, "rb").read() for x, y in zip(new, old))
            out["%d-bit WAV" % bps] = {
                "tracks": a.flac_tracks, "seconds_each": a.seconds,
                "encode_flac_files_batch": stats(new_ms[1:]),
                "encode_flac_batch_over_WaveReaders": stats(old_ms[1:]),
                "files_identical": same}
    return out


def save(path, result):
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


STEPS = {"kernel": (step_kernel, 300), "upload": (step_upload, 900), "flac": (step_flac, 600)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1024)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--parent-calls-24", type=int, default=3,
                    help="timed calls of the 24-bit upload step (the host unpack takes "
                         "tens of seconds a call at the full size)")
    ap.add_argument("--flac-tracks", type=int, default=128)
    ap.add_argument("--flac-calls", type=int, default=4)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm_bytes_bench.json"))
    a = ap.parse_args()
    if a.step:
        print(json.dumps(STEPS[a.step][0](a)))
        return 0
    result = {"workload": "%d tracks x %d s, 44.1 kHz stereo" % (a.tracks, a.seconds),
              "arguments": {k: v for k, v in vars(a).items() if k not in ("step", "out")}}
    for name in ("kernel", "upload", "flac"):
        cmd = ["timeout", "-k", "10", str(STEPS[name][1]), sys.executable, os.path.abspath(__file__),
               "--step", name, "--tracks", str(a.tracks), "--seconds", str(a.seconds),
               "--calls", str(a.calls), "--parent-calls-24", str(a.parent_calls_24),
               "--flac-tracks", str(a.flac_tracks), "--flac-calls", str(a.flac_calls)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print("step %s failed (rc %d); stopping" % (name, p.returncode))
            result[name] = {"failed_rc": p.returncode}
            break
        result[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(name, json.dumps(result[name])[:400], flush=True)
        save(a.out, result)
    save(a.out, result)
    return 0 if "failed_rc" not in json.dumps(result) else 1


if __name__ == "__main__":
    sys.exit(main())
