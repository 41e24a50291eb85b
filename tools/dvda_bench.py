#!/usr/bin/env python3
"""Measurements of the DVD-Audio title decoder (csrc/aob_decode.hip) ->
profiles/dvda_bench.json.

    python3 tools/dvda_bench.py [--titles 64] [--seconds 10] [--out FILE]

runs three steps, each a child process under its own `timeout`, one after
the other, and stops at the first that fails:

  kernel     --titles titles x --seconds s of 24-bit 6-channel 96 kHz and of
             16-bit stereo 44.1 kHz, built on the host and uploaded once:
             the three passes' kernel times from atg_aob_kernel_times, as
             TB/s of AOB bytes read + PCM bytes written and as a fraction of
             8 TB/s; against atg_pcm_unpack_device (24-bit big endian into
             int32, 16-bit into int16) over the same sample count in the same
             process, alternating; four titles compared with the port after
             the clock
  reference  oracle/_ref/aobdec, 16 processes at a time, over the same titles
             as files (absent where the binary is not built)
  flac       dvda.tracks_to_flac_batch on a disc of --seconds s tracks
             against FlacAudio.from_pcm over decoders.DVDA_Title one track
             after another; the files compared

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
SECTOR = 2048
AOBDEC = os.path.join(ROOT, "oracle", "_ref", "aobdec")
SHAPES = [("24-bit 6-channel 96 kHz", 24, 6, 1), ("16-bit stereo 44.1 kHz", 16, 2, 8)]
RATES = {1: 96000, 8: 44100}


def stats(ms):
    ms = sorted(ms)
    return {"n": len(ms), "min_ms": round(ms[0], 3), "median_ms": round(ms[len(ms) // 2], 3),
            "max_ms": round(ms[-1], 3)}


def title_image(seed, bits, channels, rate_code, frames):
    """one title of `frames` frames: full sectors of 2000 payload bytes, the
    sector headers made once and the payload placed with numpy"""
    import dvda_build
    chunk = bits // 8 * channels * 2
    total = frames // 2 * chunk
    n = (total + 1999) // 2000
    head = dvda_build.sector(b"\x5a" * 2000, bps_code=dvda_build.BPS_CODE[bits],
                             rate_code=rate_code, assignment=dvda_build.ASSIGNMENT[channels])
    off = head.index(b"\x5a" * 2000)
    img = np.tile(np.frombuffer(head, dtype=np.uint8), n).reshape(n, SECTOR)
    rng = np.random.default_rng(seed)
    stream = rng.integers(0, 256, n * 2000, dtype=np.uint8)
    img[:, off:off + 2000] = stream.reshape(n, 2000)
    if total % 2000:      # the last sector is shorter
        last = dvda_build.sector(stream[(n - 1) * 2000:total].tobytes(),
                                 bps_code=dvda_build.BPS_CODE[bits], rate_code=rate_code,
                                 assignment=dvda_build.ASSIGNMENT[channels])
        img[n - 1] = np.frombuffer(last, dtype=np.uint8)
    return img.reshape(-1)


def step_kernel(a):
    import torch
    torch.cuda.init()
    import aob_port
    from audiotools import _atgpu
    eng = _atgpu.engine()
    out = {}
    for name, bits, ch, rate_code in SHAPES:
        frames = RATES[rate_code] * a.seconds // 2 * 2
        one = [title_image(100 + t, bits, ch, rate_code, frames) for t in range(4)]
        data = np.concatenate([one[t % 4] for t in range(a.titles)])
        n_sec = len(one[0]) // SECTOR
        titles = _atgpu.aob_titles([(t * len(one[0]), n_sec) for t in range(a.titles)])
        fmt, isize = (_atgpu.PCM_S16, 2) if bits == 16 else (_atgpu.PCM_S32, 4)
        width = bits // 8
        samples = a.titles * frames * ch
        # the yardstick: packed big-endian samples of the same count
        packed_cap = (samples * width + 15) // 16 * 16
        lay = _atgpu.pcm_layout(width, True, True)
        runs = _atgpu.pcm_runs([(0, samples, 0)])
        d_bytes = eng.device_alloc(data.nbytes)
        d_packed = eng.device_alloc(packed_cap)
        d_pcm = None
        try:
            eng.copy_to_device(d_bytes, data)
            eng.copy_to_device(d_packed, data[:packed_cap] if packed_cap <= data.nbytes else
                               np.resize(data, packed_cap))
            res, total = _atgpu.aob_scan_device(d_bytes, data.nbytes, titles, fmt)
            d_pcm = eng.device_alloc(max(total, samples) * isize)
            passes, unpack, wall = {"sectors": [], "layout": [], "pcm": []}, [], []
            for k in range(a.calls + 2):
                t0 = time.perf_counter()
                res = _atgpu.aob_decode_device(d_bytes, data.nbytes, titles, d_pcm, fmt, total)
                wall.append((time.perf_counter() - t0) * 1e3)
                for key, ms in _atgpu.aob_kernel_times().items():
                    passes[key].append(ms)
                _atgpu.pcm_unpack_device(d_packed, packed_cap, lay, runs, d_pcm, fmt, samples)
                unpack.append(_atgpu.pcm_bytes_kernel_times()["unpack"])
            res = _atgpu.aob_decode_device(d_bytes, data.nbytes, titles, d_pcm, fmt, total)
            same = all(r.good_frames == frames and r.status == 0 for r in res)
            for t in (0, 1, a.titles // 2, a.titles - 1):
                r = res[t]
                got = eng.copy_to_host(np.empty(frames * ch, dtype=np.int16 if isize == 2
                                                else np.int32), d_pcm + r.sample_offset * isize)
                want = aob_port.decode(one[t % 4].tobytes())[1]
                same = same and bool(np.array_equal(got, want))
        finally:
            for d in (d_bytes, d_packed, d_pcm):
                if d:
                    eng.device_free(d)
        aob_bytes = data.nbytes + samples * isize
        unpack_bytes = samples * (width + isize)
        three = [x + y + z for x, y, z in zip(passes["sectors"][2:], passes["layout"][2:],
                                              passes["pcm"][2:])]
        r = {"titles": a.titles, "frames_each": frames, "sectors_each": n_sec,
             "aob_bytes_read_plus_pcm_written": aob_bytes,
             "unpack_bytes_read_plus_written": unpack_bytes,
             "four_titles_equal_the_port": same,
             "call_wall": stats(wall[2:])}
        for key in ("sectors", "layout", "pcm"):
            r[key] = stats(passes[key][2:])
        s = stats(three)
        s["tb_per_s"] = round(aob_bytes / (s["median_ms"] * 1e-3) / 1e12, 3)
        s["fraction_of_8_tb_per_s"] = round(s["tb_per_s"] / HBM_TBS, 3)
        r["three_passes"] = s
        u = stats(unpack[2:])
        u["tb_per_s"] = round(unpack_bytes / (u["median_ms"] * 1e-3) / 1e12, 3)
        r["pcm_unpack_device"] = u
        r["bytes_per_s_against_unpack"] = round(s["tb_per_s"] / u["tb_per_s"], 3)
        r["target_0.7_met"] = r["bytes_per_s_against_unpack"] >= 0.7
        out[name] = r
    return out


def step_reference(a):
    if not os.path.exists(AOBDEC):
        return {"absent": "oracle/_ref/aobdec is not built"}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, bits, ch, rate_code in SHAPES:
            frames = RATES[rate_code] * a.seconds // 2 * 2
            dirs = []
            for t in range(min(a.titles, a.reference_titles)):
                d = os.path.join(tmp, "%d_%d" % (bits, t))
                os.makedirs(d)
                img = title_image(100 + t % 4, bits, ch, rate_code, frames)
                img.tofile(os.path.join(d, "ATS_01_1.AOB"))
                dirs.append((d, len(img) // SECTOR))
            pts = (frames - 2) * 90000 // RATES[rate_code]
            t0 = time.perf_counter()
            running = []
            for d, n in dirs:
                running.append(subprocess.Popen([AOBDEC, d, "1", "0", str(n), str(pts)],
                                                stdout=subprocess.DEVNULL,
                                                stderr=subprocess.DEVNULL))
                if len(running) == 16:
                    running.pop(0).wait()
            for p in running:
                p.wait()
            sec = time.perf_counter() - t0
            out[name] = {"titles": len(dirs), "processes": 16, "seconds": round(sec, 3),
                         "titles_per_s": round(len(dirs) / sec, 2),
                         "aob_mb_per_s": round(sum(n for _, n in dirs) * SECTOR / sec / 1e6, 1)}
    return out


def step_flac(a):
    import torch
    torch.cuda.init()
    import dvda_build
    import dvda_cases
    from audiotools import dvda
    from audiotools.flac import FlacAudio
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, bits, ch, rate_code in SHAPES:
            rate = RATES[rate_code]
            frames = rate * a.seconds
            path = os.path.join(tmp, "disc%d" % bits)
            chunk = bits // 8 * ch * 2
            n_sec = (frames * a.flac_tracks // 2 * chunk + 1999) // 2000
            spec = dvda_cases.spec(bits, bits, ch, [2000] * n_sec, rate=rate_code)
            dvda_build.write_disc(path, [(spec, [frames] * a.flac_tracks)])
            disc = dvda.DVDAudio(path)
            tracks = list(disc[0][0])
            new = [os.path.join(tmp, "new%d_%d.flac" % (bits, k)) for k in range(len(tracks))]
            old = [os.path.join(tmp, "old%d_%d.flac" % (bits, k)) for k in range(len(tracks))]
            new_ms, old_ms = [], []
            for k in range(a.flac_calls + 1):
                t0 = time.perf_counter()
                res = dvda.tracks_to_flac_batch(tracks, new, "8")
                new_ms.append((time.perf_counter() - t0) * 1e3)
                assert all(isinstance(r, FlacAudio) for r in res), res
                t0 = time.perf_counter()
                reader = disc[0][0].to_pcm()
                for track, target in zip(tracks, old):
                    reader.next_track(track.pts_length)
                    FlacAudio.from_pcm(target, reader, "8", total_pcm_frames=frames)
                old_ms.append((time.perf_counter() - t0) * 1e3)
            same = all(open(x, "rb").read() == open(y, "rb").read() for x, y in zip(new, old))
            out[name] = {"tracks": len(tracks), "seconds_each": a.seconds,
                         "tracks_to_flac_batch": stats(new_ms[1:]),
                         "from_pcm_over_DVDA_Title": stats(old_ms[1:]),
                         "files_identical": same}
    return out


def save(path, result):
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


STEPS = {"kernel": (step_kernel, 300), "reference": (step_reference, 300),
         "flac": (step_flac, 420)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--titles", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reference-titles", type=int, default=32)
    ap.add_argument("--flac-tracks", type=int, default=4)
    ap.add_argument("--flac-calls", type=int, default=3)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dvda_bench.json"))
    a = ap.parse_args()
    if a.step:
        print(json.dumps(STEPS[a.step][0](a)))
        return 0
    result = {"workload": "%d titles x %d s" % (a.titles, a.seconds),
              "arguments": {k: v for k, v in vars(a).items() if k not in ("step", "out")}}
    for name in ("kernel", "reference", "flac"):
        cmd = ["timeout", "-k", "10", str(STEPS[name][1]), sys.executable,
               os.path.abspath(__file__), "--step", name, "--titles", str(a.titles),
               "--seconds", str(a.seconds), "--calls", str(a.calls),
               "--reference-titles", str(a.reference_titles),
               "--flac-tracks", str(a.flac_tracks), "--flac-calls", str(a.flac_calls)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print("step %s failed (rc %d); stopping" % (name, p.returncode))
            result[name] = {"failed_rc": p.returncode}
            break
        result[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(name, json.dumps(result[name])[:600], flush=True)
        save(a.out, result)
    save(a.out, result)
    return 0 if "failed_rc" not in json.dumps(result) else 1


if __name__ == "__main__":
    sys.exit(main())
