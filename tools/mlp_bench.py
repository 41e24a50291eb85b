#!/usr/bin/env python3
"""Measurements of the MLP title decoder (csrc/mlp_decode.hip) ->
profiles/mlp_bench.json.

    python3 tools/mlp_bench.py [--titles 64] [--seconds 10] [--out FILE]

runs two steps, the second without the GPU:

  kernel     --titles titles x --seconds s of 24-bit 6-channel 96 kHz (two
             substreams, filters, a matrix, check data) and of 16-bit stereo
             48 kHz, made by tiling a stream of tests/mlp_build.py on the host
             and uploaded once: the passes' kernel times from
             atg_mlp_kernel_times, each pass's share, the filter chain's time
             per second of one title, the call's wall time; after the clock
             four titles' first sectors against tests/mlp_port.py and their
             whole PCM's MD5 for the reference step
  reference  oracle/_ref/aobdec, 16 processes at a time, over the same titles
             as files (absent where the binary is not built); its PCM's MD5
             against the kernel step's
"""
import argparse
import hashlib
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

SECTOR = 2048
PAYLOAD = 2000
AOBDEC = os.path.join(ROOT, "oracle", "_ref", "aobdec")
RATES = {0: 48000, 1: 96000}
PASSES = ["sectors", "layout", "gather", "walk", "check", "parse", "resolve", "store", "filter",
          "output"]
PORT_SECTORS = 12


def shapes():
    import mlp_cases
    return [("24-bit 6-channel 96 kHz, two substreams",
             mlp_cases.spec("bench-24-6", 201, 24, 6, plan="matrix", substreams=2, split=2,
                            check=True, rate=1, units=32, frames=40, every=8)),
            ("16-bit stereo 48 kHz",
             mlp_cases.spec("bench-16-2", 202, 16, 2, plan="fir-restart", rate=0, units=32,
                            frames=40, every=8))]


def stats(ms):
    ms = sorted(ms)
    return {"n": len(ms), "min_ms": round(ms[0], 3), "median_ms": round(ms[len(ms) // 2], 3),
            "max_ms": round(ms[-1], 3)}


def title_image(spec, seconds):
    """-> (image as uint8 array, frames): the spec's stream tiled up to
    `seconds`, in full sectors of 2000 payload bytes whose header is made once"""
    import dvda_build
    import mlp_cases
    _, stream = mlp_cases.expand(spec)
    per = spec["units"] * spec["frames"]
    reps = max(1, RATES[spec["rate"]] * seconds // per)
    data = np.tile(np.frombuffer(stream, dtype=np.uint8), reps)
    n = (len(data) + PAYLOAD - 1) // PAYLOAD
    head = dvda_build.sector(b"\x5a" * PAYLOAD, codec=0xA1, pad2=6)
    off = head.index(b"\x5a" * PAYLOAD)
    img = np.tile(np.frombuffer(head, dtype=np.uint8), n).reshape(n, SECTOR).copy()
    full = len(data) // PAYLOAD
    img[:full, off:off + PAYLOAD] = data[:full * PAYLOAD].reshape(full, PAYLOAD)
    if full < n:
        img[n - 1] = np.frombuffer(dvda_build.sector(data[full * PAYLOAD:].tobytes(), codec=0xA1,
                                                     pad2=6), dtype=np.uint8)
    return img.reshape(-1), reps * per


def step_kernel(a):
    import torch
    torch.cuda.init()
    import aob_port
    import mlp_port
    from audiotools import _atgpu
    eng = _atgpu.engine()
    out = {}
    for name, spec in shapes():
        one, frames = title_image(spec, a.seconds)
        ch = spec["channels"]
        data = np.tile(one, a.titles)
        n_sec = len(one) // SECTOR
        titles = _atgpu.aob_titles([(t * len(one), n_sec) for t in range(a.titles)])
        d_bytes = eng.device_alloc(data.nbytes)
        d_pcm = None
        try:
            eng.copy_to_device(d_bytes, data)
            res, total = _atgpu.mlp_scan_device(d_bytes, data.nbytes, titles, _atgpu.PCM_S32)
            d_pcm = eng.device_alloc(max(16, total * 4))
            passes, wall = dict((k, []) for k in PASSES), []
            for k in range(a.calls + 2):
                t0 = time.perf_counter()
                res = _atgpu.mlp_decode_device(d_bytes, data.nbytes, titles, d_pcm,
                                               _atgpu.PCM_S32, total)
                wall.append((time.perf_counter() - t0) * 1e3)
                for key, ms in _atgpu.mlp_kernel_times().items():
                    passes[key].append(ms)
            same = all(r.good_frames == frames and r.status == 0 for r in res)
            want = mlp_port.decode(one[:PORT_SECTORS * SECTOR].tobytes())[1]
            md5 = []
            for t in (0, 1, a.titles // 2, a.titles - 1):
                r = res[t]
                got = eng.copy_to_host(np.empty(frames * ch, dtype=np.int32),
                                       d_pcm + r.sample_offset * 4)
                same = same and len(want) > 0 and bool(np.array_equal(got[:len(want)], want))
                md5.append(hashlib.md5(aob_port.pcm_bytes(got, spec["bits"])).hexdigest())
        finally:
            for d in (d_bytes, d_pcm):
                if d:
                    eng.device_free(d)
        r = {"titles": a.titles, "frames_each": frames, "sectors_each": n_sec,
             "seconds_each": round(frames / RATES[spec["rate"]], 3),
             "access_units_each": res[0].access_units, "all_titles_decode": same,
             "four_titles_first_sectors_equal_the_port": same, "pcm_md5": md5,
             "call_wall": stats(wall[2:])}
        med = {}
        for key in PASSES:
            r[key] = stats(passes[key][2:])
            med[key] = r[key]["median_ms"]
        whole = sum(med.values())
        r["all_passes_median_ms"] = round(whole, 3)
        r["share"] = dict((k, round(v / whole, 4)) for k, v in med.items())
        r["bounding_pass"] = max(med, key=med.get)
        r["filter_ms_per_title_second"] = round(med["filter"] / r["seconds_each"], 4)
        r["titles_per_s"] = round(a.titles / (r["call_wall"]["median_ms"] * 1e-3), 2)
        r["audio_seconds_per_s"] = round(r["titles_per_s"] * r["seconds_each"], 1)
        out[name] = r
    return out


def step_reference(a):
    if not os.path.exists(AOBDEC):
        return {"absent": "oracle/_ref/aobdec is not built"}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, spec in shapes():
            img, frames = title_image(spec, a.seconds)
            rate = RATES[spec["rate"]]
            dirs = []
            for t in range(min(a.titles, a.reference_titles)):
                d = os.path.join(tmp, "%s_%d" % (spec["name"], t))
                os.makedirs(d)
                img.tofile(os.path.join(d, "ATS_01_1.AOB"))
                dirs.append(d)
            n = len(img) // SECTOR
            pts = frames * 90000 // rate
            while (2 * pts * rate + 90000) // 180000 > frames:
                pts -= 1
            t0 = time.perf_counter()
            running = []
            for d in dirs:
                running.append(subprocess.Popen(
                    [AOBDEC, d, "1", "0", str(n), str(pts)],
                    stdout=open(os.path.join(d, "pcm"), "wb"), stderr=subprocess.DEVNULL))
                if len(running) == 16:
                    running.pop(0).wait()
            for p in running:
                p.wait()
            sec = time.perf_counter() - t0
            raw = open(os.path.join(dirs[0], "pcm"), "rb").read()
            out[name] = {"titles": len(dirs), "processes": 16, "seconds": round(sec, 3),
                         "titles_per_s": round(len(dirs) / sec, 2),
                         "frames_written": len(raw) // (spec["bits"] // 8 * spec["channels"]),
                         "pcm_md5": hashlib.md5(raw).hexdigest(), "pcm_bytes": len(raw)}
    return out


def save(path, result):
    """indented, with the innermost dicts and lists on one line each"""
    import re
    text = re.sub(r"[\[{][^\[\]{}]*[\]}]", lambda m: " ".join(m.group(0).split()),
                  json.dumps(result, indent=1))
    with open(path, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--titles", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reference-titles", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_bench.json"))
    a = ap.parse_args()
    result = {"workload": "%d titles x %d s" % (a.titles, a.seconds),
              "arguments": {k: v for k, v in vars(a).items() if k != "out"}}
    result["kernel"] = step_kernel(a)
    save(a.out, result)
    result["reference"] = step_reference(a)
    cmp = {}
    for shape, k in result["kernel"].items():
        ref = result["reference"].get(shape)
        if isinstance(ref, dict) and "titles_per_s" in ref:
            cmp[shape] = {
                "titles_per_s_against_16_reference_processes":
                    round(k["titles_per_s"] / ref["titles_per_s"], 2),
                "pcm_equals_the_reference": ref["pcm_md5"] in k["pcm_md5"] and
                len(set(k["pcm_md5"])) == 1}
    result["against_the_reference"] = cmp
    save(a.out, result)
    print(json.dumps({k: v for k, v in result.items() if k != "kernel"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
