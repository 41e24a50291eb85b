#!/usr/bin/env python3
"""PCM comparison on the GPU: the compare pass and the offset search over a
device-resident batch, beside the AccurateRip streaming pass on the same
batch, and compare_files_batch against the host comparison of the same files.

Default shape: 1024 pairs x 10 s at 44.1 kHz, 16-bit stereo, PCM made on the
device.  Side A of a pair starts on a 16-byte boundary, side B three samples
off one, so the two streams sit at unrelated phases.

1. atg_pcm_compare_device, `--steps` timed calls each after `--warmup`:
   identical pairs int32 / int32 and int16 / int32 (the full read: the
   algorithmic bytes are both sides), and int32 pairs that differ in their
   first tile (what the early exit saves).  A call is timed with the host
   clock round it (it ends in a stream synchronise and includes the upload of
   the pair table and the copy of the results); the kernel alone comes from
   atg_pcm_compare_kernel_times (HIP events round the launch).
2. atg_pcm_offset_search_device at K = `--max-offset` on pairs that match at
   a shift of 6 frames.
3. atg_accuraterip_device at max_offset 0 over side A, the same way: the
   project's best single-stream reader, the yardstick.
4. compare_files_batch on `--files` pairs of 10-s .flac files against
   pcm_frame_cmp(FlacAudio(a).to_pcm(), FlacAudio(b).to_pcm()) per pair,
   alternating in one process, `--file-steps` timed calls each.

After the clock, `--check` pairs of every case are compared with the numpy
port.  Writes one JSON document (--out, default
profiles/pcm_compare_bench.json) and prints it.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-audio-tools_amd"), os.path.join(ROOT, "tests")]
HBM_BYTES_PER_S = 8e12  # MI355X peak


def stats(ms):
    return {"mean_ms": float(np.mean(ms)), "median_ms": float(np.median(ms)),
            "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "steps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--max-offset", type=int, default=2940)
    ap.add_argument("--check", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--file-steps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm_compare_bench.json"))
    args = ap.parse_args()

    import torch
    import oracle_port
    import pcm_compare_port as port
    import signals
    import audiotools
    from audiotools import _atgpu, accuraterip

    torch.cuda.init()
    dev = torch.device("cuda:0")
    rate, K, P = args.rate, args.max_offset, args.pairs
    n = int(args.seconds * rate)
    N = P * n * 2                      # samples per side
    check = sorted(set(int(x) for x in np.linspace(0, P - 1, args.check)))
    PHASE = 3

    g = torch.Generator(device=dev)
    g.manual_seed(1)
    a32 = torch.randint(-32768, 32768, (N + 8,), dtype=torch.int32, device=dev, generator=g)
    a16 = a32.to(torch.int16)
    b32 = torch.zeros(N + 8, dtype=torch.int32, device=dev)
    b32[PHASE:PHASE + N] = a32[:N]
    torch.cuda.synchronize()

    def view(t, fmt, ptr, phase, window=0, whole=False):
        if whole:   # the whole side as one source, the window at track t
            return _atgpu.pcm_view(ptr, fmt, P * n, phase, t * n + window)
        return _atgpu.pcm_view(ptr, fmt, n, phase + t * n * 2, window)

    def table(fmt_a, ptr_a, shift=0):
        return [_atgpu.pcm_pair(view(t, fmt_a, ptr_a, 0),
                                view(t, _atgpu.PCM_S32, b32.data_ptr(), PHASE, -shift,
                                     whole=shift != 0), n, 2) for t in range(P)]

    def timed(fn, algo_bytes):
        host, kern = [], {}
        for step in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            got = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if step >= args.warmup:
                host.append(dt)
                for name, ms in _atgpu.pcm_compare_kernel_times().items():
                    kern.setdefault(name, []).append(ms)
        row = dict(stats(host), kernel_ms={k: stats(v) for k, v in kern.items()})
        if algo_bytes:   # None where the call reads a fraction that is not known
            mean = row["mean_ms"] * 1e-3
            row["algorithmic_bytes"] = algo_bytes
            row["algorithmic_bytes_per_s"] = algo_bytes / mean
            row["fraction_of_8TBps"] = algo_bytes / mean / HBM_BYTES_PER_S
            kms = float(np.mean(kern.get("compare", [0.0]))) * 1e-3
            if kms > 0:
                row["kernel_fraction_of_8TBps"] = algo_bytes / kms / HBM_BYTES_PER_S
        return row, got

    bad = 0
    cases = {}
    # ---- 1. the compare pass
    same32 = table(_atgpu.PCM_S32, a32.data_ptr())
    cases["identical_s32_s32"], got = timed(lambda: _atgpu.pcm_compare_device(same32), 8 * N)
    bad += sum(x is not None for x in got)
    same16 = table(_atgpu.PCM_S16, a16.data_ptr())
    cases["identical_s16_s32"], got = timed(lambda: _atgpu.pcm_compare_device(same16), 6 * N)
    bad += sum(x is not None for x in got)
    # every pair differs at frame 100 + (t % 7), second channel
    spots = torch.tensor([PHASE + t * n * 2 + (100 + t % 7) * 2 + 1 for t in range(P)],
                         device=dev)
    b32[spots] ^= 1
    torch.cuda.synchronize()
    cases["differ_in_first_tile_s32_s32"], got = timed(
        lambda: _atgpu.pcm_compare_device(same32), None)
    cases["differ_in_first_tile_s32_s32"]["kernel_over_identical"] = (
        cases["differ_in_first_tile_s32_s32"]["kernel_ms"]["compare"]["mean_ms"] /
        cases["identical_s32_s32"]["kernel_ms"]["compare"]["mean_ms"])
    cases["differ_in_first_tile_s32_s32"]["note"] = (
        "the same table as identical_s32_s32 after one sample of every pair's B side changed "
        "in its first tile; no roofline fraction: the early exit reads only part of the batch")
    bad += sum(x != 100 + t % 7 for t, x in enumerate(got))
    for t in check:
        xa = a32[t * n * 2:(t + 1) * n * 2].cpu().numpy()
        xb = b32[PHASE + t * n * 2:PHASE + (t + 1) * n * 2].cpu().numpy()
        bad += port.compare(xa, 0, xb, 0, n, 2) != got[t]
    b32[spots] ^= 1
    torch.cuda.synchronize()

    # ---- 2. the offset search: A(i) == B(i + 6), B the whole side
    shifted = table(_atgpu.PCM_S32, a32.data_ptr(), shift=6)
    cases["search_K%d_shift_6" % K], got = timed(
        lambda: _atgpu.pcm_offset_search_device(shifted, K), 8 * N)
    cases["search_K%d_shift_6" % K]["note"] = (
        "launches: A against silence and A against B at shift 0 (both end early), the probe, "
        "one full verification at shift 6; algorithmic_bytes counts that verification alone, "
        "kernel_fraction_of_8TBps sets it against all compare launches of the call")
    bad += sum(x[0] != 6 for x in got)
    for t in check[:2]:   # the port's brute force, over a narrower sweep
        xa = a32[t * n * 2:(t + 1) * n * 2].cpu().numpy()
        lo, hi = max(0, t * n - 70), min(P * n, t * n + n + 70)
        xb = b32[PHASE + lo * 2:PHASE + hi * 2].cpu().numpy()
        bad += port.best_offset(xa, 0, xb, t * n - lo - 6, n, 2, 64) != got[t][0]

    # ---- 3. the yardstick: AccurateRip over side A
    tracks = [accuraterip.track(t * n, n, rate, t % 16 == 0, t % 16 == 15 or t == P - 1)
              for t in range(P)]
    ms = []
    for step in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        _atgpu.accuraterip_device(a32.data_ptr(), _atgpu.PCM_S32, tracks, 0)
        ms.append((time.perf_counter() - t0) * 1e3)
    ar = dict(stats(ms[args.warmup:]), algorithmic_bytes=4 * N)
    ar["algorithmic_bytes_per_s"] = 4 * N / (ar["mean_ms"] * 1e-3)
    ar["fraction_of_8TBps"] = ar["algorithmic_bytes_per_s"] / HBM_BYTES_PER_S
    ratio = cases["identical_s32_s32"]["algorithmic_bytes_per_s"] / ar["algorithmic_bytes_per_s"]
    del a32, a16, b32
    torch.cuda.empty_cache()

    # ---- 4. files: the device batch against the host comparison
    distinct = min(args.distinct, args.files)
    pcms = [signals.make("tone", n, 2, 16, seed=200 + k) for k in range(distinct)]
    other = pcms[0].copy()
    other[n] ^= 1                      # frame n // 2, first channel
    eng = _atgpu.engine()
    opts = _atgpu.make_options(**oracle_port.PRESETS["8"])
    out, eres, _, _ = eng.encode(opts, np.concatenate(pcms + [other]).astype(np.int16),
                                 [(k * n, n) for k in range(distinct + 1)], 2, 16, rate)
    images = [out[r.out_offset:r.out_offset + r.bytes].tobytes() for r in eres]
    files = {}
    with tempfile.TemporaryDirectory() as d:
        pairs = []
        for k in range(args.files):
            ia = k % distinct
            ib = distinct if (k % 8 == 0 and ia == 0) else ia
            pa, pb = os.path.join(d, "a%d.flac" % k), os.path.join(d, "b%d.flac" % k)
            for p, i in ((pa, ia), (pb, ib)):
                with open(p, "wb") as f:
                    f.write(images[i])
            pairs.append((pa, pb))

        def on_device():
            return audiotools.compare_files_batch(pairs)

        def on_host():
            return [audiotools.pcm_frame_cmp(audiotools.FlacAudio(a).to_pcm(),
                                             audiotools.FlacAudio(b).to_pcm())
                    for a, b in pairs]

        rows = {"compare_files_batch": [], "pcm_frame_cmp_per_pair": []}
        results = {}
        for step in range(1 + args.file_steps):   # one warm-up round
            for name, fn in (("compare_files_batch", on_device),
                             ("pcm_frame_cmp_per_pair", on_host)):
                t0 = time.perf_counter()
                results[name] = fn()
                if step >= 1:
                    rows[name].append((time.perf_counter() - t0) * 1e3)
    same = results["compare_files_batch"] == results["pcm_frame_cmp_per_pair"]
    bad += not same
    files = {
        "pairs": args.files, "seconds": args.seconds,
        "flac_images": "FLAC-8 from the GPU encoder, %d distinct signals; some pairs differ "
                       "in one sample at frame %d" % (distinct, n // 2),
        "compare_files_batch": stats(rows["compare_files_batch"]),
        "pcm_frame_cmp_per_pair": stats(rows["pcm_frame_cmp_per_pair"]),
        "results_identical": bool(same),
        "mismatching_pairs": sum(x is not None for x in results["compare_files_batch"]),
        "note": "%d timed calls each after one warm-up round, alternating; the host path "
                "takes seconds per call" % args.file_steps,
    }
    files["host_over_device"] = (files["pcm_frame_cmp_per_pair"]["mean_ms"] /
                                 files["compare_files_batch"]["mean_ms"])

    doc = {
        "shape": {"pairs": P, "seconds": args.seconds, "rate": rate, "channels": 2,
                  "pcm_frames_per_side": P * n, "max_offset": K, "b_phase_samples": PHASE,
                  "tile_frames": _atgpu.pcm_compare_tile_frames(), "warmup": args.warmup,
                  "steps": args.steps, "device": torch.cuda.get_device_name(0)},
        "timing": "host clock round each call (ends in a stream synchronise, includes the "
                  "table upload and the result copy); kernel_ms from HIP events round the "
                  "launches (atg_pcm_compare_kernel_times), no counters collected",
        "compare": cases,
        "accuraterip_same_batch": ar,
        "compare_over_accuraterip_bytes_per_s": ratio,
        "expected_ratio_at_least": 0.7,
        "files": files,
        "verify": {"pairs_checked": len(check), "mismatches": int(bad)},
    }
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
