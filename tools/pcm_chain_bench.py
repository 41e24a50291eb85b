#!/usr/bin/env python3
"""The PCM converter chain on the GPU (csrc/pcm_chain.hip) and the batch file
conversion built on it.

1. Bits only, identity map: one track of the shape in k_pcm_bps's own record
   (profiles/r05_zz_convert.txt: 537 M samples, 16 -> 8 bits, int32 in and
   out), atg_pcm_chain_device against atg_pcm_convert_device on the same
   buffers, alternating in one process.  Each call is timed with HIP events
   on the default stream round it (both launch there); the chain's own event
   pair (atg_pcm_chain_kernel_times) is reported beside it.  The old entry
   has no kernel-time call of its own.
2. The headline shape: `--tracks` tracks x `--seconds` s of 24-bit 5.1 to
   16-bit stereo in the int16 container -- DOWNMIX and bits in one pass --
   every source three samples off a 16-byte boundary; the fraction of the
   8 TB/s roofline over the bytes read and written, and the time to draw
   (os.urandom) and upload the dither bytes.
3. End to end: `--files` ten-second 24-bit / 96 kHz stereo .flac files to
   16-bit / 44.1 kHz FLAC-8, convert_files_batch against the reader path
   (FlacAudio.from_pcm over PCMConverter, one file after another),
   alternating, under an all-zero dither; the files must be identical.

4. With --dither, instead of the three legs above: the headline shape's dither
   bits made on the device (csrc/dither.hip) against os.urandom + upload, and
   the fill kernel against a hipMemsetAsync of the same buffer (dither_leg;
   default --out profiles/dither_bench.json).

Writes one JSON document (--out, default profiles/pcm_chain_bench.json) and
prints it.
"""
import argparse
import ctypes
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


def zeros(n):
    return b"\0" * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits-samples", type=int, default=1024 * 262144 * 2)
    ap.add_argument("--tracks", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--check", type=int, default=3)
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--file-steps", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dither", action="store_true",
                    help="the device-side dither leg alone (profiles/dither_bench.json)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles",
                                "dither_bench.json" if args.dither else "pcm_chain_bench.json")
    if args.dither:
        return dither_leg(args)

    import torch
    import oracle_port
    import pcm_chain_port as port
    import signals
    import audiotools
    from audiotools import _atgpu, pcmconverter

    torch.cuda.init()
    dev = torch.device("cuda:0")
    lib = _atgpu.load_library()
    bad = 0

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # ---- 1. bits only: the new kernel against k_pcm_bps, one track
    n = args.bits_samples
    frames = n // 2
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.randint(-32768, 32768, (n,), dtype=torch.int32, device=dev, generator=g)
    y_old, y_new = torch.empty_like(x), torch.empty_like(x)
    dither = torch.randint(0, 256, ((n + 7) // 8,), dtype=torch.uint8, device=dev, generator=g)
    row = [_atgpu.pcm_chain_row(_atgpu.pcm_view(x.data_ptr(), _atgpu.PCM_S32, frames), 2, 2, 16, 8,
                                0)]

    def old():
        st = lib.atg_pcm_convert_device(_atgpu.CONV_BPS, x.data_ptr(), y_old.data_ptr(), frames,
                                        2, 0, 16, 8, dither.data_ptr(), 0, None)
        if st != _atgpu.ATG_OK:
            raise RuntimeError(lib.atg_pcm_convert_last_error())

    def new():
        _atgpu.pcm_chain_device(row, y_new.data_ptr(), _atgpu.PCM_S32, n, dither.data_ptr(),
                                dither.numel())

    ms = {"atg_pcm_convert_device": [], "atg_pcm_chain_device": [], "chain_own_events": []}
    for step in range(args.warmup + args.steps):
        a, b = event_ms(old), event_ms(new)
        if step >= args.warmup:
            ms["atg_pcm_convert_device"].append(a)
            ms["atg_pcm_chain_device"].append(b)
            ms["chain_own_events"].append(_atgpu.pcm_chain_kernel_times()["chain"])
    alg = 8 * n + dither.numel()
    bits = {k: dict(stats(v), bytes_per_s=alg / (np.mean(v) * 1e-3),
                    fraction_of_8TBps=alg / (np.mean(v) * 1e-3) / HBM_BYTES_PER_S)
            for k, v in ms.items()}
    same = bool(torch.equal(y_old, y_new))
    bad += not same
    bits_doc = {
        "shape": {"samples": n, "channels": 2, "frames": frames, "in_bps": 16, "out_bps": 8,
                  "format": "int32 in, int32 out, one track"},
        "algorithmic_bytes": alg, "outputs_identical": same, "timing": bits,
        "new_over_old_bytes_per_s": (bits["chain_own_events"]["bytes_per_s"] /
                                     bits["atg_pcm_convert_device"]["bytes_per_s"]),
        "note": "HIP events on the default stream round each call, the two entries alternating; "
                "the chain call also uploads its row table and ends in a stream synchronise, so "
                "chain_own_events (its event pair round the launch alone) is the kernel time and "
                "new_over_old_bytes_per_s compares that with the old call's events",
    }
    del x, y_old, y_new, dither
    torch.cuda.empty_cache()

    # ---- 2. the headline: 24-bit 5.1 -> 16-bit stereo, int16 out, off a boundary
    P, nf, PHASE = args.tracks, int(args.seconds * args.rate), 3
    stride = (nf * 6 + 3) // 4 * 4          # every track at the same phase
    src = torch.randint(-(1 << 23), 1 << 23, (P * stride + 8,), dtype=torch.int32, device=dev,
                        generator=g)
    ostride = (nf * 2 + 7) // 8 * 8
    out = torch.zeros(P * ostride, dtype=torch.int16, device=dev)
    per_track = (nf * 2 + 7) // 8
    t0 = time.perf_counter()
    drawn = os.urandom(per_track * P)
    t_draw = time.perf_counter() - t0
    t0 = time.perf_counter()
    d_bits = torch.frombuffer(bytearray(drawn), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    t_up = time.perf_counter() - t0
    rows = [_atgpu.pcm_chain_row(
        _atgpu.pcm_view(src.data_ptr(), _atgpu.PCM_S32, nf, PHASE + t * stride), 6, 2, 24, 16,
        t * ostride, _atgpu.CHAIN_DOWNMIX, None, 0x3F, 8 * per_track * t) for t in range(P)]

    def headline():
        _atgpu.pcm_chain_device(rows, out.data_ptr(), _atgpu.PCM_S16, out.numel(),
                                d_bits.data_ptr(), d_bits.numel())

    host, kern = [], []
    for step in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        headline()
        dt = (time.perf_counter() - t0) * 1e3
        if step >= args.warmup:
            host.append(dt)
            kern.append(_atgpu.pcm_chain_kernel_times()["chain"])
    alg = P * nf * (6 * 4 + 2 * 2) + P * per_track
    for t in sorted(set(int(v) for v in np.linspace(0, P - 1, args.check))):
        xs = src[PHASE + t * stride:PHASE + t * stride + nf * 6].cpu().numpy()
        want = port.convert_row(xs, 6, port.DOWNMIX, 24, 16, mask=0x3F,
                                dither=drawn[per_track * t:per_track * (t + 1)])
        got = out[t * ostride:t * ostride + nf * 2].cpu().numpy().astype(np.int32)
        bad += not np.array_equal(got, want)
    head_doc = {
        "shape": {"tracks": P, "seconds": args.seconds, "rate": args.rate, "frames": nf,
                  "in": "24-bit 5.1, int32", "out": "16-bit stereo, int16",
                  "source_phase_samples": PHASE, "tile_samples": _atgpu.pcm_chain_tile_samples()},
        "algorithmic_bytes": alg,
        "call": dict(stats(host), fraction_of_8TBps=alg / (np.mean(host) * 1e-3) / HBM_BYTES_PER_S),
        "kernel": dict(stats(kern), bytes_per_s=alg / (np.mean(kern) * 1e-3),
                       fraction_of_8TBps=alg / (np.mean(kern) * 1e-3) / HBM_BYTES_PER_S),
        "dither": {"bytes": len(drawn), "draw_ms": t_draw * 1e3, "upload_ms": t_up * 1e3},
        "note": "call: host clock round atg_pcm_chain_device (the checks, the upload of the row "
                "table, the launch, a stream synchronise); kernel: its event pair",
    }
    del src, out, d_bits
    torch.cuda.empty_cache()

    # ---- 3. end to end: files (--files 0 skips it)
    if not args.files:
        return finish(args, torch, bits_doc, head_doc, None, bad)
    rate_in, n_in = 96000, 960000
    distinct = min(args.distinct, args.files)
    pcms = [signals.make("tone", n_in, 2, 24, seed=300 + k) for k in range(distinct)]
    eng = _atgpu.engine()
    opts = _atgpu.make_options(**oracle_port.PRESETS["8"])
    enc, eres, _, _ = eng.encode(opts, np.concatenate(pcms).astype(np.int32),
                                 [(k * n_in, n_in) for k in range(distinct)], 2, 24, rate_in)
    images = [enc[r.out_offset:r.out_offset + r.bytes].tobytes() for r in eres]
    n_out = _atgpu.resample_output_frames(n_in, 2, rate_in, 44100)
    with tempfile.TemporaryDirectory() as d:
        srcs = []
        for k in range(args.files):
            srcs.append(os.path.join(d, "s%d.flac" % k))
            with open(srcs[-1], "wb") as f:
                f.write(images[k % distinct])
        dev_t = [os.path.join(d, "d%d.flac" % k) for k in range(args.files)]
        ref_t = [os.path.join(d, "r%d.flac" % k) for k in range(args.files)]

        def on_device(m):
            got = audiotools.convert_files_batch(srcs[:m], dev_t[:m], sample_rate=44100,
                                                 bits_per_sample=16, compression="8",
                                                 dither=zeros)
            return sum(not isinstance(x, audiotools.FlacAudio) for x in got)

        def on_readers(m):
            for s, t in zip(srcs[:m], ref_t[:m]):
                reader = audiotools.PCMConverter(
                    audiotools.BufferedPCMReader(audiotools.FlacAudio(s).to_pcm()), 44100, 2, 0x3,
                    16)
                assert isinstance(reader, pcmconverter.BPSConverter)
                reader._rand = zeros
                audiotools.FlacAudio.from_pcm(t, reader, "8", total_pcm_frames=n_out)
            return 0

        rows_ms = {"convert_files_batch": [], "reader_path": []}
        for step in range(1 + args.file_steps):   # a warm-up round of 4 files
            m = args.files if step else min(4, args.files)
            for name, fn in (("convert_files_batch", on_device), ("reader_path", on_readers)):
                t0 = time.perf_counter()
                bad += fn(m)
                if step:
                    rows_ms[name].append((time.perf_counter() - t0) * 1e3)
        identical = 0
        for a, b in zip(dev_t, ref_t):
            with open(a, "rb") as fa, open(b, "rb") as fb:
                identical += fa.read() == fb.read()
    bad += identical != args.files
    files_doc = {
        "files": args.files, "distinct_signals": distinct,
        "source": "24-bit / 96 kHz stereo, %d frames, FLAC-8" % n_in,
        "target": "16-bit / 44.1 kHz stereo, %d frames, FLAC-8, all-zero dither" % n_out,
        "convert_files_batch": stats(rows_ms["convert_files_batch"]),
        "reader_path": stats(rows_ms["reader_path"]),
        "files_identical": identical,
        "note": "%d timed round(s) each after a warm-up round of 4 files, alternating; the "
                "reader path is FlacAudio.from_pcm(PCMConverter(BufferedPCMReader(to_pcm()))) "
                "one file after another" % args.file_steps,
    }
    files_doc["readers_over_batch"] = (files_doc["reader_path"]["mean_ms"] /
                                       files_doc["convert_files_batch"]["mean_ms"])

    return finish(args, torch, bits_doc, head_doc, files_doc, bad)


def dither_leg(args):
    """--dither: the headline shape's dither bits made on the device
    (csrc/dither.hip) against drawing them with os.urandom and uploading them.

    a. the fill kernel alone over the batch's dither buffer, and a
       hipMemsetAsync of the same buffer as a store-only yardstick;
    b. the chain of a batch conversion (pcmconverter.run_chain_device, what
       convert_pcm_batch runs between its upload and its download) over the
       same device-resident sources with dither=DeviceDither and with the
       default os.urandom, alternating in one process."""
    import torch
    import dither_port
    from audiotools import _atgpu, pcmconverter

    torch.cuda.init()
    dev = torch.device("cuda:0")
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t,
                                   ctypes.c_void_p]
    P, nf = args.tracks, int(args.seconds * args.rate)
    blocks = ((nf * 2 + 7) // 8 + 15) // 16
    size = 16 * blocks * P
    buf = torch.zeros(size, dtype=torch.uint8, device=dev)
    runs = [(t, 0, blocks, 16 * blocks * t) for t in range(P)]
    seed = 0x0123456789ABCDEF
    bad = 0

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def memset():
        if hip.hipMemsetAsync(buf.data_ptr(), 0x5A, size, None) != 0:
            raise RuntimeError("hipMemsetAsync failed")

    fill_call, fill_kernel, memset_ms = [], [], []
    for step in range(args.warmup + args.steps):
        m = event_ms(memset)
        t0 = time.perf_counter()
        _atgpu.dither_fill_device(runs, seed, buf.data_ptr(), size)
        dt = (time.perf_counter() - t0) * 1e3
        if step >= args.warmup:
            memset_ms.append(m)
            fill_call.append(dt)
            fill_kernel.append(_atgpu.dither_kernel_times()["fill"])
    host = buf.cpu().numpy()
    for t in sorted(set(int(v) for v in np.linspace(0, P - 1, args.check))):
        want = dither_port.blocks(seed, t, 0, blocks)
        bad += not np.array_equal(host[16 * blocks * t:16 * blocks * (t + 1)], want)

    def rate(ms):
        return size / (np.mean(ms) * 1e-3)

    fill_doc = {
        "bytes": size, "runs": P, "blocks_per_run": blocks,
        "tile_blocks": _atgpu.dither_tile_blocks(),
        "fill_kernel": dict(stats(fill_kernel), bytes_per_s=rate(fill_kernel),
                            fraction_of_8TBps=rate(fill_kernel) / HBM_BYTES_PER_S),
        "fill_call": stats(fill_call),
        "hipMemsetAsync": dict(stats(memset_ms), bytes_per_s=rate(memset_ms),
                               fraction_of_8TBps=rate(memset_ms) / HBM_BYTES_PER_S),
        "fill_over_memset_bytes_per_s": rate(fill_kernel) / rate(memset_ms),
        "note": "fill_kernel: the call's own event pair round the launch; fill_call: host clock "
                "round atg_dither_fill_device (checks, table upload, launch, synchronise); "
                "hipMemsetAsync: torch events on the default stream round the call, alternating "
                "with the fill",
    }
    del buf
    torch.cuda.empty_cache()

    # ---- b. the chain with the bits made on the device against drawn and uploaded
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    stride = (nf * 6 + 3) // 4 * 4
    src = torch.randint(-(1 << 23), 1 << 23, (P * stride,), dtype=torch.int32, device=dev,
                        generator=g)
    sources = [pcmconverter.DevicePcm(src.data_ptr(), _atgpu.PCM_S32, t * stride, nf)
               for t in range(P)]
    plan = pcmconverter.plan_target((6, 0x3F, 24, args.rate), channels=2, channel_mask=0x3,
                                    bits_per_sample=16)
    plans = [plan] * P
    eng = _atgpu.engine()

    def chain(dither):
        t0 = time.perf_counter()
        done, free = pcmconverter.run_chain_device(sources, plans, dither)
        dt = (time.perf_counter() - t0) * 1e3
        kernel = _atgpu.pcm_chain_kernel_times()["chain"]
        for d in free:
            eng.device_free(d)
        return dt, kernel

    ms = {"DeviceDither": [], "os.urandom": [], "chain_kernel": []}
    for step in range(args.warmup + args.steps):
        a, k = chain(pcmconverter.DeviceDither(seed))
        b, _ = chain(None)
        if step >= args.warmup:
            ms["DeviceDither"].append(a)
            ms["os.urandom"].append(b)
            ms["chain_kernel"].append(k)
    chain_doc = {
        "shape": {"tracks": P, "seconds": args.seconds, "rate": args.rate, "frames": nf,
                  "in": "24-bit 5.1, int32, device resident", "out": "16-bit stereo, int16"},
        "run_chain_device_DeviceDither": stats(ms["DeviceDither"]),
        "run_chain_device_os_urandom": stats(ms["os.urandom"]),
        "chain_kernel": stats(ms["chain_kernel"]),
        "urandom_over_device": float(np.mean(ms["os.urandom"]) / np.mean(ms["DeviceDither"])),
        "note": "host clock round pcmconverter.run_chain_device, the part of convert_pcm_batch "
                "between its upload and its download (identical in both paths and left out: "
                "the 10.8 GB of sources stay in device memory); the two paths alternate on the "
                "same sources; each call allocates its output and dither buffers",
    }
    doc = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "steps": args.steps,
           "fill": fill_doc, "chain": chain_doc,
           "verify": {"streams_checked": args.check, "mismatches": int(bad)}}
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 1 if bad else 0


def finish(args, torch, bits_doc, head_doc, files_doc, bad):
    doc = {
        "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "steps": args.steps,
        "bits_only": bits_doc, "headline": head_doc, "files": files_doc,
        "verify": {"tracks_checked": args.check, "mismatches": int(bad)},
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
