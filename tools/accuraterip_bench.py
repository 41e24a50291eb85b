#!/usr/bin/env python3
"""AccurateRip on the GPU: the checksum pass over a device-resident batch,
and verify_flac_batch's device part against the plain FLAC decode.

Default shape: 1024 tracks x 10 s at 44.1 kHz, 16-bit stereo, PCM made on
the device.

1. atg_accuraterip_device on int32 device PCM at max_offset 0 and 2940,
   `--steps` timed calls each after `--warmup`.  A call is timed with the
   host clock around it; it ends in a stream synchronise, and it includes
   the upload of the track table and the copy of the results (at K = 2940
   the n x 5881 offset table) back to the host.
2. FLAC-8 images of `--distinct` signals from the GPU encoder, repeated
   over the batch: decode alone and decode + checksum of the decoder's
   device PCM, alternating in one process; and the alternative the
   checksum pass avoids, copying the batch's PCM to the host.

After the clock, v1 and v2 of `--check` tracks are compared with the numpy
port.  There is no reference timing: the reference's loop exists only inside
its Python 2 extension.  Writes one JSON document (--out, default
profiles/accuraterip_bench.json) and prints it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-audio-tools_amd"), os.path.join(ROOT, "tests")]
HBM_BYTES_PER_S = 8e12  # MI355X peak


def stats(ms):
    return {"mean_ms": float(np.mean(ms)), "median_ms": float(np.median(ms)),
            "min_ms": float(np.min(ms)),
            "max_ms": float(np.max(ms)), "steps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--max-offset", type=int, default=2940)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--check", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--copy-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accuraterip_bench.json"))
    args = ap.parse_args()

    import torch
    import accuraterip_port as port
    import oracle_port
    import signals
    from audiotools import _atgpu, accuraterip

    torch.cuda.init()
    dev = torch.device("cuda:0")
    rate, K = args.rate, args.max_offset
    n, T = int(args.seconds * rate), args.tracks
    check = sorted(set(int(x) for x in np.linspace(0, T - 1, args.check)))

    def flags(t):  # albums of 16 tracks
        return t % 16 == 0, t % 16 == 15 or t == T - 1

    # ---- 1. the checksum pass alone
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    pcm = torch.randint(-32768, 32768, (T * n * 2,), dtype=torch.int32, device=dev, generator=g)
    torch.cuda.synchronize()
    tracks = [accuraterip.track(t * n, n, rate, *flags(t), lo_frame=t // 16 * 16 * n,
                                hi_frame=min(T, t // 16 * 16 + 16) * n) for t in range(T)]
    passes = {}
    for k in (0, K):
        ms = []
        for step in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            res, table = _atgpu.accuraterip_device(pcm.data_ptr(), _atgpu.PCM_S32, tracks, k)
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = ms[args.warmup:]
        # 8 B per included frame is read once; the sweep reads 4k frames per
        # track round its two edges and writes the table
        algo = 8 * n * T + (4 * k * 8 + (2 * k + 1) * 4) * T * (1 if k else 0)
        mean = float(np.mean(ms))
        passes["max_offset_%d" % k] = dict(
            stats(ms), pcm_frames_per_s=n * T / (mean * 1e-3), algorithmic_bytes=algo,
            algorithmic_bytes_per_s=algo / (mean * 1e-3),
            fraction_of_8TBps=algo / (mean * 1e-3) / HBM_BYTES_PER_S,
            host_table_bytes=int(table.nbytes))
        last = (res, table)
    bad = 0
    for t in check:
        x = pcm[t * n * 2:(t + 1) * n * 2].cpu().numpy()
        bad += (last[0][t].v1, last[0][t].v2) != port.checksums(x, *flags(t), rate)
        bad += int(last[1][t, K]) != last[0][t].v1
    lo = check[0] // 16 * 16
    img = pcm[lo * n * 2:(lo + 16) * n * 2].cpu().numpy()
    want = port.sweep(img, (check[0] - lo) * n, n, 0, min(T - lo, 16) * n, *flags(check[0]),
                      rate, min(K, 64))
    mid = last[1][check[0], K - min(K, 64):K + min(K, 64) + 1]
    bad += mid.tolist() != want
    del pcm
    torch.cuda.empty_cache()

    # ---- 2. decode alone against decode + checksum, alternating
    distinct = min(args.distinct, T)
    pcms = [signals.make("tone", n, 2, 16, seed=100 + k) for k in range(distinct)]
    eng = _atgpu.engine()
    opts = _atgpu.make_options(**oracle_port.PRESETS["8"])
    out, eres, _, _ = eng.encode(opts, np.concatenate(pcms).astype(np.int16),
                                 [(k * n, n) for k in range(distinct)], 2, 16, rate)
    bodies, infos = [], []
    for r in eres:
        image = out[r.out_offset:r.out_offset + r.bytes].tobytes()
        rc, si, _ = _atgpu.read_metadata(image)
        assert rc == 0
        body = image[si.frames_offset:]
        bodies.append((body + b"\0" * ((-len(body)) % 4), len(body)))
        infos.append(si)
    dtracks, parts, pos = [], [], 0
    for t in range(T):
        body, used = bodies[t % distinct]
        dtracks.append(_atgpu.dec_track(pos, used, infos[t % distinct]))
        parts.append(body)
        pos += len(body)
    blob = torch.frombuffer(bytearray(b"".join(parts) + b"\0" * 64), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    dec = _atgpu.Decoder(0)

    def decode_only():
        return dec.decode_device(blob.data_ptr(), pos, dtracks)

    def decode_and_checksum():
        dres, d_pcm, ns = dec.decode_device(blob.data_ptr(), pos, dtracks)
        tr = [accuraterip.track(r.pcm_offset, r.pcm_frames, rate, *flags(t))
              for t, r in enumerate(dres)]
        return dres, _atgpu.accuraterip_device(d_pcm, _atgpu.PCM_S32, tr, 0)[0], d_pcm, ns

    rows = {"decode": [], "decode_and_checksum": []}
    for step in range(args.warmup + args.steps):
        for name, fn in (("decode", decode_only), ("decode_and_checksum", decode_and_checksum)):
            t0 = time.perf_counter()
            got = fn()
            if step >= args.warmup:
                rows[name].append((time.perf_counter() - t0) * 1e3)
    dres, ar, d_pcm, ns = got
    copy_ms = []
    host = np.empty(ns, dtype=np.int32)
    for _ in range(args.copy_steps):
        t0 = time.perf_counter()
        eng.copy_to_host(host, d_pcm)
        copy_ms.append((time.perf_counter() - t0) * 1e3)
    status_bad = sum(r.status != 0 for r in dres)
    for t in check:
        bad += (ar[t].v1, ar[t].v2) != port.checksums(pcms[t % distinct], *flags(t), rate)
    dec.close()

    d, dc = stats(rows["decode"]), stats(rows["decode_and_checksum"])
    doc = {
        "shape": {"tracks": T, "seconds": args.seconds, "rate": rate, "channels": 2,
                  "bits_per_sample": 16, "pcm_frames": n * T, "max_offset": K,
                  "tile_frames": _atgpu.accuraterip_tile_frames(), "warmup": args.warmup,
                  "steps": args.steps, "device": torch.cuda.get_device_name(0)},
        "timing": "host clock round each call; every call ends in a stream synchronise and "
                  "includes its table upload and result copies",
        "checksum_pass": dict(passes, sweep_over_plain=passes["max_offset_%d" % K]["mean_ms"] /
                              passes["max_offset_0"]["mean_ms"]),
        "verify_device_part": {
            "flac_images": "FLAC-8 from the GPU encoder, %d distinct signals" % distinct,
            "encoded_bytes": int(pos), "decode": d, "decode_and_checksum": dc,
            "difference_ms": dc["mean_ms"] - d["mean_ms"],
            "difference_of_medians_ms": dc["median_ms"] - d["median_ms"],
            "pcm_copy_to_host": dict(stats(copy_ms), bytes=int(ns) * 4,
                                     note="pageable host memory, the avoided alternative")},
        "verify": {"tracks_checked": len(check), "mismatches": int(bad),
                   "decode_status_nonzero": int(status_bad)},
        "reference": "none: the reference's checksum loop exists only inside its Python 2 "
                     "extension, which is not built here",
    }
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 1 if bad or status_bad else 0


if __name__ == "__main__":
    sys.exit(main())
