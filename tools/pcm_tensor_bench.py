#!/usr/bin/env python3
"""PCM rows to planar float tensors and back on the GPU (csrc/pcm_tensor.hip),
and load_batch built on it.

1. Kernels: `--tracks` tracks x `--seconds` s of 44.1 kHz stereo made on the
   device, every row three samples off a 16-byte boundary, into a
   [tracks, 2, frames + 3] tensor (so the channel runs start at every phase
   of a 16-byte unit): int16 -> float32, int32 (24-bit) -> float32 and
   float32 -> int16, each alternating in one process with
   atg_pcm_chain_device over identity rows of the same PCM.  Kernel times are
   the components' own event pairs (atg_pcm_tensor_kernel_times,
   atg_pcm_chain_kernel_times); bytes are PCM bytes + tensor bytes (for the
   chain: PCM bytes read + written).
2. Files: load_batch on `--files` ten-second 16-bit 44.1 kHz stereo FLAC files
   against the host route -- to_pcm() read to its end, FrameList.to_float(),
   torch.tensor(...).cuda() -- two timed rounds each, alternating, four rows
   compared after the clock.

Writes one JSON document (--out, default profiles/pcm_tensor_bench.json) and
prints it.
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
BAR = 0.7               # of the nearest existing kernel's bytes per second


def stats(ms):
    return {"mean_ms": float(np.mean(ms)), "median_ms": float(np.median(ms)),
            "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "steps": len(ms)}


def rate(ms, nbytes):
    per_s = nbytes / (np.mean(ms) * 1e-3)
    return dict(stats(ms), bytes=int(nbytes), bytes_per_s=per_s,
                fraction_of_8TBps=per_s / HBM_BYTES_PER_S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--check", type=int, default=4)
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--file-rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm_tensor_bench.json"))
    args = ap.parse_args()

    import torch
    import oracle_port
    import pcm_tensor_port as port
    import signals
    import audiotools
    from audiotools import _atgpu, pcm, tensors  # noqa: F401  (tensors: torch comes up first)

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    bad = 0
    P, nf, PHASE, CH = args.tracks, int(args.seconds * args.rate), 3, 2
    T = nf + 3
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    picks = sorted(set(int(v) for v in np.linspace(0, P - 1, args.check)))

    def alternate(ours, ours_times, name, chain):
        own, other = [], []
        for step in range(args.warmup + args.steps):
            ours()
            a = ours_times()[name]
            chain()
            b = _atgpu.pcm_chain_kernel_times()["chain"]
            if step >= args.warmup:
                own.append(a)
                other.append(b)
        return own, other

    def case(fmt, bps, np_dtype):
        """to_tensor (and for int16 from_tensor) against the identity chain"""
        nonlocal bad
        width = np.dtype(np_dtype).itemsize
        t_dtype = torch.int16 if fmt == _atgpu.PCM_S16 else torch.int32
        stride = (nf * CH + PHASE + 7) // 8 * 8    # every track at the same phase
        lo, hi = -(1 << (bps - 1)), 1 << (bps - 1)
        src = torch.randint(lo, hi, (P * stride + 8,), dtype=t_dtype, device=dev, generator=g)
        audio = torch.empty((P, CH, T), dtype=torch.float32, device=dev)
        ostride = (nf * CH + 7) // 8 * 8
        copy = torch.empty(P * ostride, dtype=t_dtype, device=dev)
        to_rows = [_atgpu.pcm_to_tensor_row(
            _atgpu.pcm_view(src.data_ptr(), fmt, nf, PHASE + t * stride), CH, bps, T, t * CH * T, T)
            for t in range(P)]
        chain_rows = [_atgpu.pcm_chain_row(
            _atgpu.pcm_view(src.data_ptr(), fmt, nf, PHASE + t * stride), CH, CH, bps, bps,
            t * ostride) for t in range(P)]

        def to_tensor():
            _atgpu.pcm_to_tensor_device(to_rows, audio.data_ptr(), _atgpu.TENSOR_F32,
                                        audio.numel(), stream)

        def chain():
            _atgpu.pcm_chain_device(chain_rows, copy.data_ptr(), fmt, copy.numel())

        own, other = alternate(to_tensor, _atgpu.pcm_tensor_kernel_times, "to_tensor", chain)
        pcm_bytes, tensor_bytes = P * nf * CH * width, P * CH * T * 4
        doc = {"to_tensor": rate(own, pcm_bytes + tensor_bytes),
               "chain_identity": rate(other, 2 * pcm_bytes)}
        doc["to_tensor"]["over_chain_bytes_per_s"] = (doc["to_tensor"]["bytes_per_s"] /
                                                      doc["chain_identity"]["bytes_per_s"])
        for t in picks:
            xs = src[PHASE + t * stride:PHASE + t * stride + nf * CH].cpu().numpy()
            want = np.zeros((CH, T), dtype=np.float32)
            want[:, :nf] = port.to_values(xs, CH, bps, port.F32)
            bad += not np.array_equal(port.bits(audio[t].cpu().numpy()), port.bits(want))
        if fmt == _atgpu.PCM_S16:
            back = torch.zeros(P * ostride, dtype=torch.int16, device=dev)
            from_rows = [_atgpu.pcm_from_tensor_row(t * CH * T, T, nf, CH, bps, t * ostride)
                         for t in range(P)]

            def from_tensor():
                _atgpu.pcm_from_tensor_device(from_rows, audio.data_ptr(), _atgpu.TENSOR_F32,
                                              audio.numel(), back.data_ptr(), fmt, back.numel(),
                                              stream)

            own, other = alternate(from_tensor, _atgpu.pcm_tensor_kernel_times, "from_tensor",
                                   chain)
            doc["from_tensor"] = rate(own, pcm_bytes + P * CH * nf * 4)
            doc["chain_identity_beside_from_tensor"] = rate(other, 2 * pcm_bytes)
            doc["from_tensor"]["over_chain_bytes_per_s"] = (
                doc["from_tensor"]["bytes_per_s"] /
                doc["chain_identity_beside_from_tensor"]["bytes_per_s"])
            for t in picks:
                xs = src[PHASE + t * stride:PHASE + t * stride + nf * CH]
                bad += not torch.equal(back[t * ostride:t * ostride + nf * CH], xs)
        del src, audio, copy
        torch.cuda.empty_cache()
        return doc

    kernels = {"int16_float32": case(_atgpu.PCM_S16, 16, np.int16),
               "int32_24bit_float32": case(_atgpu.PCM_S32, 24, np.int32)}
    ratios = [kernels["int16_float32"]["to_tensor"]["over_chain_bytes_per_s"],
              kernels["int32_24bit_float32"]["to_tensor"]["over_chain_bytes_per_s"],
              kernels["int16_float32"]["from_tensor"]["over_chain_bytes_per_s"]]
    kernels_doc = {
        "shape": {"tracks": P, "seconds": args.seconds, "rate": args.rate, "frames": nf,
                  "channels": CH, "tensor_frames": T, "source_phase_samples": PHASE,
                  "tile_frames": _atgpu.pcm_tensor_tile_frames()},
        "cases": kernels, "bar_over_chain": BAR, "bar_met": bool(min(ratios) >= BAR),
        "note": "kernel time: each component's own event pair round its launch; bytes: PCM "
                "bytes + tensor bytes (float32, pad frames included on the way there), for the "
                "chain PCM bytes read + written; the calls alternate in one process",
    }

    files_doc = None
    if args.files:
        n_in, rate_in = 441000, 44100
        distinct = min(args.distinct, args.files)
        pcms = [signals.make("tone", n_in, 2, 16, seed=500 + k) for k in range(distinct)]
        eng = _atgpu.engine()
        opts = _atgpu.make_options(**oracle_port.PRESETS["8"])
        enc, eres, _, _ = eng.encode(opts, np.concatenate(pcms).astype(np.int16),
                                     [(k * n_in, n_in) for k in range(distinct)], 2, 16, rate_in)
        images = [enc[r.out_offset:r.out_offset + r.bytes].tobytes() for r in eres]
        with tempfile.TemporaryDirectory() as d:
            srcs = []
            for k in range(args.files):
                srcs.append(os.path.join(d, "s%d.flac" % k))
                with open(srcs[-1], "wb") as f:
                    f.write(images[k % distinct])
            kept = {}

            def on_device(m):
                kept["device"] = audiotools.load_batch(srcs[:m])
                torch.cuda.synchronize()

            def on_host(m):
                rows = []
                for s in srcs[:m]:
                    reader = audiotools.FlacAudio(s).to_pcm()
                    parts = []
                    while True:
                        fl = reader.read(4096)
                        if fl.frames == 0:
                            break
                        parts.append(fl.samples)
                    reader.close()
                    as_float = pcm.FrameList._wrap(np.concatenate(parts), 2, 16).to_float()
                    rows.append(np.stack([as_float.channel(c).samples for c in range(2)])
                                .astype(np.float32))
                kept["host"] = torch.tensor(np.stack(rows)).cuda()
                torch.cuda.synchronize()

            ms = {"load_batch": [], "host_route": []}
            for step in range(1 + args.file_rounds):   # a warm-up round of 4 files
                m = args.files if step else min(4, args.files)
                for name, fn in (("load_batch", on_device), ("host_route", on_host)):
                    t0 = time.perf_counter()
                    fn(m)
                    if step:
                        ms[name].append((time.perf_counter() - t0) * 1e3)
            same = 0
            rows = sorted(set(int(v) for v in np.linspace(0, args.files - 1, 4)))
            for k in rows:
                same += bool(torch.equal(kept["device"].audio[k], kept["host"][k]))
            bad += same != len(rows)
            bad += sum(e is not None for e in kept["device"].errors)
        files_doc = {
            "files": args.files, "distinct_signals": distinct,
            "source": "16-bit / 44.1 kHz stereo, %d frames, FLAC-8" % n_in,
            "load_batch": stats(ms["load_batch"]), "host_route": stats(ms["host_route"]),
            "rows_compared": len(rows), "rows_identical": same,
            "note": "%d timed round(s) each after a warm-up round of 4 files, alternating; the "
                    "host route is to_pcm() read to its end, FrameList.to_float(), "
                    "torch.tensor(...).cuda(), one file after another" % args.file_rounds,
        }
        files_doc["host_over_load_batch"] = (files_doc["host_route"]["mean_ms"] /
                                             files_doc["load_batch"]["mean_ms"])

    doc = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "steps": args.steps,
           "kernels": kernels_doc, "files": files_doc,
           "verify": {"tracks_checked": len(picks), "mismatches": int(bad)}}
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
