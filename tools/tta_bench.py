#!/usr/bin/env python3
"""True Audio on the GPU: batch encode and decode of device-resident tracks,
timed per kernel with HIP events (atg_tta_encoder_kernel_times /
atg_tta_decoder_kernel_times), verified, and compared with the reference's
standalone encoder and decoder where oracle/_ref/ttaenc and ttadec exist.

Default shape: 1024 tracks x 10 s of `tone` (tests/signals.py) at 44.1 kHz,
16-bit stereo; 2 warm-up and 20 timed steps of each direction.  The tracks
are `--distinct` different signals repeated over the batch.

Every encoded image is compared with tests/tta_port.py's (all tracks, through
the `--verify` distinct signals tta_port encodes), every decoded track with
its source.  Writes one JSON document (--out, default profiles/tta_bench.json)
and prints it.
"""
import argparse
import concurrent.futures
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-audio-tools_amd"), os.path.join(ROOT, "tests")]
REF = os.path.join(ROOT, "oracle", "_ref")
HBM_BYTES_PER_S = 8e12  # MI355X peak


def mean_times(rows):
    keys = rows[0].keys()
    return {k: float(np.mean([r[k] for r in rows])) for k in keys}


def reference_run(pcms, n_tracks, ch, bps, rate, procs):
    """ttaenc then ttadec over the same tracks, `procs` at a time -> seconds"""
    enc, dec = os.path.join(REF, "ttaenc"), os.path.join(REF, "ttadec")
    if not (os.path.exists(enc) and os.path.exists(dec)):
        return None
    raws = [p.astype("<i2" if bps == 16 else np.int8).tobytes() for p in pcms]
    n = len(pcms[0]) // ch
    with tempfile.TemporaryDirectory() as tmp:
        def one_enc(k):
            subprocess.run([enc, "-c", str(ch), "-r", str(rate), "-b", str(bps), "-T", str(n),
                            os.path.join(tmp, "%d.tta" % k)], input=raws[k % len(raws)],
                           stdout=subprocess.DEVNULL, check=True)

        def one_dec(k):
            subprocess.run([dec, os.path.join(tmp, "%d.tta" % k)], stdout=subprocess.DEVNULL,
                           check=True)

        out = {}
        for name, fn in (("encode_s", one_enc), ("decode_s", one_dec)):
            t0 = time.perf_counter()
            with concurrent.futures.ThreadPoolExecutor(procs) as ex:
                list(ex.map(fn, range(n_tracks)))
            out[name] = time.perf_counter() - t0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--verify", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_bench.json"))
    args = ap.parse_args()

    import torch
    import signals
    import tta_port
    from audiotools import _atgpu

    ch, bps, rate = 2, 16, args.rate
    n = int(args.seconds * rate)
    block = tta_port.block_size(rate)
    distinct = min(args.distinct, args.tracks)
    pcms = [signals.make("tone", n, ch, bps, seed=100 + k) for k in range(distinct)]
    torch.cuda.init()
    dev = torch.device("cuda:0")
    tiles = torch.stack([torch.from_numpy(p.astype(np.int16)) for p in pcms]).to(dev)
    src = tiles[torch.arange(args.tracks, device=dev) % distinct].reshape(-1).contiguous()
    del tiles
    tracks = [(k * n, n) for k in range(args.tracks)]
    table = _atgpu.TrackTable(tracks)
    frames_per_track = (n + block - 1) // block
    n_frames = frames_per_track * args.tracks
    torch.cuda.synchronize()

    # ---- encode
    enc = _atgpu.TtaEncoder(0)
    fsb = np.zeros(n_frames, np.uint32)
    cap = src.numel() * 2
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rows, walls = [], []
    for step in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        res, need = enc.encode_device(src.data_ptr(), _atgpu.PCM_S16, table, ch, bps, rate,
                                      out.data_ptr(), cap, fsb)
        wall = time.perf_counter() - t0
        if step >= args.warmup:
            rows.append(enc.kernel_times())
            walls.append(wall * 1e3)
    enc_ms = mean_times(rows)
    enc_wall = float(np.mean(walls))
    enc_bytes = int(need)
    images = out[:enc_bytes].cpu().numpy()

    # ---- decode (frames only: the header fields are given, not parsed)
    info = _atgpu.TtaInfo()
    info.channels, info.bits_per_sample, info.sample_rate = ch, bps, rate
    info.total_pcm_frames, info.block_size, info.frames_offset = n, block, 0
    dtracks = [_atgpu.tta_dec_track(r.out_offset, r.bytes, info,
                                    fsb[r.first_frame:r.first_frame + r.n_frames])
               for r in res]
    dec = _atgpu.TtaDecoder(0)
    rows, walls = [], []
    for step in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        dres, d_pcm, nsamp = dec.decode_device(out.data_ptr(), enc_bytes, dtracks)
        wall = time.perf_counter() - t0
        if step >= args.warmup:
            rows.append(dec.kernel_times())
            walls.append(wall * 1e3)
    dec_ms = mean_times(rows)
    dec_wall = float(np.mean(walls))

    # ---- verify: every image against tta_port's, every track against its source
    nver = min(args.verify, distinct)
    want = tta_port.encode_frames_many([(pcms[k], ch, bps, rate, None) for k in range(nver)])
    want = [b"".join(w) for w in want]
    enc_checked = enc_bad = 0
    for k, r in enumerate(res):
        if k % distinct < nver:
            enc_checked += 1
            if images[r.out_offset:r.out_offset + r.bytes].tobytes() != want[k % distinct]:
                enc_bad += 1
    pcm = dec.fetch(nsamp)
    dec_bad = 0
    for k, r in enumerate(dres):
        got = pcm[r.sample_offset:r.sample_offset + r.pcm_frames * ch]
        if r.status != 0 or not np.array_equal(got, pcms[k % distinct]):
            dec_bad += 1
    enc.close()
    dec.close()

    ref = None if args.no_reference else reference_run(pcms, args.tracks, ch, bps, rate,
                                                       args.procs)
    pcm_in = src.numel() * 2
    pcm_out = int(nsamp) * 4

    def side(ms, wall, total_key, algo_bytes, ref_s):
        total = ms[total_key]
        kernels = {k: v for k, v in ms.items() if k != total_key}
        bound = max(kernels, key=kernels.get)
        d = {"kernel_ms": ms, "wall_ms_per_batch": wall,
             "kernel_share": {k: v / total for k, v in kernels.items()},
             "bounding_kernel": bound,
             "tta_frames_per_s": n_frames / (total * 1e-3),
             "pcm_frames_per_s": n * args.tracks / (total * 1e-3),
             "algorithmic_bytes": algo_bytes,
             "algorithmic_bytes_per_s": algo_bytes / (total * 1e-3),
             "fraction_of_8TBps": algo_bytes / (total * 1e-3) / HBM_BYTES_PER_S}
        if ref_s is not None:
            d["reference_s"] = ref_s
            d["speedup_over_reference_kernels"] = ref_s / (total * 1e-3)
            d["speedup_over_reference_wall"] = ref_s / (wall * 1e-3)
        return d

    doc = {
        "shape": {"tracks": args.tracks, "seconds": args.seconds, "rate": rate, "channels": ch,
                  "bits_per_sample": bps, "kind": "tone", "distinct_signals": distinct,
                  "tta_frames": n_frames, "warmup": args.warmup, "steps": args.steps,
                  "device": torch.cuda.get_device_name(0)},
        "encode": side(enc_ms, enc_wall, "tta_total", pcm_in + enc_bytes,
                       ref["encode_s"] if ref else None),
        "decode": side(dec_ms, dec_wall, "ttad_total", enc_bytes + pcm_out,
                       ref["decode_s"] if ref else None),
        "encoded_bytes": enc_bytes, "compression_ratio": enc_bytes / pcm_in,
        "verify": {"images_checked_against_tta_port": enc_checked, "images_differing": enc_bad,
                   "tracks_decoded": len(dres), "tracks_differing_from_source": dec_bad},
        "reference": ("oracle/_ref/ttaenc and ttadec, %d processes at a time, same host"
                      % args.procs) if ref else "skipped: oracle/_ref/ttaenc or ttadec absent",
    }
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 1 if enc_bad or dec_bad else 0


if __name__ == "__main__":
    sys.exit(main())
