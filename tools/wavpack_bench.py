#!/usr/bin/env python3
"""WavPack on the GPU: batch decode of device-resident images, timed per
kernel with HIP events (atg_wv_decoder_kernel_times), every track verified,
and compared with the reference's standalone decoder where oracle/_ref/wvdec
exists.

Default shape: 1024 tracks x 10 s at 44.1 kHz, 16-bit stereo; 2 warm-up and
20 timed steps.  No encoder runs where this tool runs, and a WavPack block
carries all its state, so a track is tiled from the 22,050-sample block of
a committed image (tests/golden: the `len22050_c2` vector, two low tones and
a little noise per channel, five passes) with block_index and total_samples
rewritten and no MD5 block.  The reference's two fixtures are not used: their
blocks are near silence (28 to 80 bytes of sub-blocks for 22,050 frames) and
would flatter the walk.  The expected PCM of a
block is the vector's source samples.

Writes one JSON document (--out, default profiles/wavpack_bench.json) and
prints it.
"""
import argparse
import concurrent.futures
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-audio-tools_amd"), os.path.join(ROOT, "tests")]
REF = os.path.join(ROOT, "oracle", "_ref")
HBM_BYTES_PER_S = 8e12  # MI355X peak
BLOCK = 22050


def mean_times(rows):
    keys = rows[0].keys()
    return {k: float(np.mean([r[k] for r in rows])) for k in keys}


def tiled(block, n_blocks):
    """one stream of n_blocks copies of a block, indices and total rewritten"""
    out = []
    for k in range(n_blocks):
        b = bytearray(block)
        struct.pack_into("<II", b, 12, n_blocks * BLOCK, k * BLOCK)
        out.append(bytes(b))
    return b"".join(out)


def reference_run(images, n_tracks, procs):
    """wvdec over the same tracks, `procs` at a time -> seconds"""
    dec = os.path.join(REF, "wvdec")
    if not os.path.exists(dec):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        for k, img in enumerate(images):
            with open(os.path.join(tmp, "%d.wv" % k), "wb") as f:
                f.write(img)

        def one(k):
            subprocess.run([dec, os.path.join(tmp, "%d.wv" % (k % len(images)))],
                           stdout=subprocess.DEVNULL, check=True)

        t0 = time.perf_counter()
        with concurrent.futures.ThreadPoolExecutor(procs) as ex:
            list(ex.map(one, range(n_tracks)))
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavpack_bench.json"))
    args = ap.parse_args()

    import torch
    import wavpack_cases as cases
    import wavpack_port as port
    from audiotools import _atgpu

    ch, bps, rate = 2, 16, 44100
    n_blocks = max(1, int(round(args.seconds * rate / BLOCK)))
    n = n_blocks * BLOCK
    g, golden = cases.load_vectors()
    src = {c[0]: c[5] for c in cases.cases()}
    inputs = []   # (name, block bytes, its PCM)
    for name in ("len22050_c2",):
        img = golden[name]
        st, h = port.parse_header(img, 0)
        assert st == 0 and h["block_samples"] == BLOCK and h["final"] and h["coded"] == 2
        block = img[:8 + h["block_size"]]
        if name in src:
            pcm = src[name][:BLOCK * ch]
        else:
            h["data"] = (32, h["block_size"] - 24)
            st, chans = port.decode_block(img, h)
            assert st == 0
            pcm = np.stack([np.asarray(c, dtype=np.int32) for c in chans], 1).reshape(-1)
        inputs.append((name, block, np.asarray(pcm, dtype=np.int32)))
    images = [tiled(block, n_blocks) for _, block, _ in inputs]
    wants = [np.tile(pcm, n_blocks) for _, _, pcm in inputs]

    parts, tracks, pos = [], [], 0
    tables = [_atgpu.wv_read_info(img) for img in images]
    for k in range(args.tracks):
        img = images[k % len(images)]
        st, info, blocks = tables[k % len(images)]
        assert st == 0 and info.n_sets == n_blocks and info.end_status == 0
        pad = (-len(img)) % 4
        tracks.append(_atgpu.wv_dec_track(pos, len(img), info, blocks))
        parts.append(img + b"\0" * pad)
        pos += len(img) + pad
    blob = b"".join(parts)
    torch.cuda.init()
    dev = torch.device("cuda:0")
    d_blob = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()

    dec = _atgpu.WvDecoder(0)
    rows, walls = [], []
    for step in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        res, d_pcm, nsamp = dec.decode_device(d_blob.data_ptr(), len(blob), tracks)
        wall = time.perf_counter() - t0
        if step >= args.warmup:
            rows.append(dec.kernel_times())
            walls.append(wall * 1e3)
    ms = mean_times(rows)
    wall_ms = float(np.mean(walls))
    pcm = dec.fetch(nsamp)
    bad = 0
    for k, r in enumerate(res):
        got = pcm[r.sample_offset:r.sample_offset + r.pcm_frames * ch]
        if r.status != 0 or not np.array_equal(got, wants[k % len(wants)]):
            bad += 1
    dec.close()

    ref_s = None if args.no_reference else reference_run(images, args.tracks, args.procs)
    total = ms["wvd_total"]
    kernels = {k: v for k, v in ms.items() if k != "wvd_total"}
    algo = len(blob) + int(nsamp) * 4
    doc = {
        "shape": {"tracks": args.tracks, "seconds": n / rate, "rate": rate, "channels": ch,
                  "bits_per_sample": bps, "blocks_per_track": n_blocks,
                  "block_samples": BLOCK, "wavpack_blocks": n_blocks * args.tracks,
                  "warmup": args.warmup, "steps": args.steps,
                  "device": torch.cuda.get_device_name(0)},
        "input": {"tiled_from": [name for name, _, _ in inputs],
                  "how": "22,050-sample blocks of committed images repeated, block_index "
                         "and total_samples rewritten, no MD5 block",
                  "image_bytes": [len(i) for i in images], "batch_bytes": len(blob)},
        "decode": {"kernel_ms": ms, "wall_ms_per_batch": wall_ms,
                   "kernel_share": {k: v / total for k, v in kernels.items()},
                   "bounding_kernel": max(kernels, key=kernels.get),
                   "decorrelation_layout": "all passes per sample, one lane per block, "
                                           "histories in LDS",
                   "wavpack_blocks_per_s": n_blocks * args.tracks / (total * 1e-3),
                   "pcm_frames_per_s": n * args.tracks / (total * 1e-3),
                   "algorithmic_bytes": algo,
                   "algorithmic_bytes_per_s": algo / (total * 1e-3),
                   "fraction_of_8TBps": algo / (total * 1e-3) / HBM_BYTES_PER_S},
        "compression_ratio": len(blob) / (n * ch * 2 * args.tracks),
        "verify": {"tracks_decoded": len(res), "tracks_differing_from_source": bad},
        "reference": ("oracle/_ref/wvdec, %d processes at a time, same host" % args.procs)
        if ref_s is not None else "skipped: oracle/_ref/wvdec absent",
    }
    if ref_s is not None:
        doc["decode"]["reference_s"] = ref_s
        doc["decode"]["speedup_over_reference_kernels"] = ref_s / (total * 1e-3)
        doc["decode"]["speedup_over_reference_wall"] = ref_s / (wall_ms * 1e-3)
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
