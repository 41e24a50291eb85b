#!/usr/bin/env python3
"""Shorten on the GPU: batch encode and decode of device-resident tracks,
timed per stage with HIP events (atg_shn_encoder_kernel_times /
atg_shn_decoder_kernel_times), verified, and compared with the reference's
standalone encoder and decoder where oracle/_ref/shnenc and shndec exist.

Default shape: 1024 tracks x 10 s of `tone` (tests/signals.py) at 44.1 kHz,
16-bit stereo, block size 256; 2 warm-up and 20 timed steps of each
direction.  The tracks are `--distinct` different signals repeated over the
batch.  The decoder's index pass is timed both ways: with the
wave-cooperative code walk and with the lane-serial one.

Every image is decoded back to its source on the GPU, and `--compare` of them
are compared byte for byte with the file shnenc writes.  Writes one JSON
document (--out, default profiles/shn_bench.json) and prints it.
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
ENC, DEC = os.path.join(REF, "shnenc"), os.path.join(REF, "shndec")


def mean_times(rows):
    keys = rows[0].keys()
    return {k: float(np.mean([r[k] for r in rows])) for k in keys}


def shnenc_image(raw, ch, bps, block, tmp, name="one.shn"):
    path = os.path.join(tmp, name)
    subprocess.run([ENC, "-c", str(ch), "-b", str(bps), "-B", str(block), path], input=raw,
                   stdout=subprocess.DEVNULL, check=True)
    with open(path, "rb") as f:
        return f.read()


def reference_run(raws, n_tracks, ch, bps, block, procs):
    """shnenc then shndec over the same tracks, `procs` at a time -> seconds"""
    with tempfile.TemporaryDirectory() as tmp:
        def one_enc(k):
            subprocess.run([ENC, "-c", str(ch), "-b", str(bps), "-B", str(block),
                            os.path.join(tmp, "%d.shn" % k)], input=raws[k % len(raws)],
                           stdout=subprocess.DEVNULL, check=True)

        def one_dec(k):
            subprocess.run([DEC, os.path.join(tmp, "%d.shn" % k)], stdout=subprocess.DEVNULL,
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
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--compare", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shn_bench.json"))
    args = ap.parse_args()

    import torch
    import signals
    from audiotools import _atgpu

    ch, bps, rate, block = 2, 16, args.rate, args.block
    n = int(args.seconds * rate)
    distinct = min(args.distinct, args.tracks)
    pcms = [signals.make("tone", n, ch, bps, seed=100 + k) for k in range(distinct)]
    torch.cuda.init()
    dev = torch.device("cuda:0")
    tiles = torch.stack([torch.from_numpy(p.astype(np.int16)) for p in pcms]).to(dev)
    src = tiles[torch.arange(args.tracks, device=dev) % distinct].reshape(-1).contiguous()
    del tiles
    table = _atgpu.TrackTable([(k * n, n) for k in range(args.tracks)])
    n_blocks = ((n + block - 1) // block) * args.tracks
    torch.cuda.synchronize()

    # ---- encode
    enc = _atgpu.ShnEncoder(0)
    cap = src.numel() * 2
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rows, walls = [], []
    for step in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        res, need = enc.encode_device(src.data_ptr(), _atgpu.PCM_S16, table, ch, bps,
                                      out.data_ptr(), cap, block_size=block)
        wall = time.perf_counter() - t0
        if step >= args.warmup:
            rows.append(enc.kernel_times())
            walls.append(wall * 1e3)
    enc_ms = mean_times(rows)
    enc_wall = float(np.mean(walls))
    enc_bytes = int(need)
    image_bytes = int(sum(r.bytes for r in res))

    # ---- decode, the index pass both ways
    first = out[res[0].out_offset:res[0].out_offset + res[0].bytes].cpu().numpy().tobytes()
    st, info = _atgpu.shn_read_info(first)
    assert st == _atgpu.SHN_OK
    dtracks = [_atgpu.shn_dec_track(r.out_offset, r.bytes, info) for r in res]
    dec = _atgpu.ShnDecoder(0)
    dec_ms, dec_wall = {}, {}
    for walk, coop in (("serial", False), ("cooperative", True)):
        dec.set_index_walk(coop)
        rows, walls = [], []
        for step in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            dres, d_pcm, nsamp = dec.decode_device(out.data_ptr(), enc_bytes, dtracks)
            wall = time.perf_counter() - t0
            if step >= args.warmup:
                rows.append(dec.kernel_times())
                walls.append(wall * 1e3)
        dec_ms[walk] = mean_times(rows)
        dec_wall[walk] = float(np.mean(walls))
    default = "cooperative"

    # ---- verify: every track decoded back to its source, some images against shnenc
    pcm = dec.fetch(nsamp)
    dec_bad = 0
    for k, r in enumerate(dres):
        got = pcm[r.pcm_offset:r.pcm_offset + r.pcm_frames * ch]
        if r.status != _atgpu.SHN_END_OF_STREAM or not np.array_equal(got, pcms[k % distinct]):
            dec_bad += 1
    del pcm
    raws = [p.astype("<i2").tobytes() for p in pcms]
    have_ref = os.path.exists(ENC) and os.path.exists(DEC)
    compared = differing = 0
    if have_ref:
        with tempfile.TemporaryDirectory() as tmp:
            for k in range(min(args.compare, distinct)):
                r = res[k]
                mine = out[r.out_offset:r.out_offset + r.bytes].cpu().numpy().tobytes()
                compared += 1
                differing += mine != shnenc_image(raws[k], ch, bps, block, tmp)
    enc.close()
    dec.close()

    ref = None
    if have_ref and not args.no_reference:
        ref = reference_run(raws, args.tracks, ch, bps, block, args.procs)
    pcm_in = src.numel() * 2
    pcm_out = int(nsamp) * 4

    def side(ms, wall, total_key, algo_bytes, ref_s):
        total = ms[total_key]
        stages = {k: v for k, v in ms.items() if k != total_key}
        d = {"stage_ms": ms, "wall_ms_per_batch": wall,
             "stage_share": {k: v / total for k, v in stages.items()},
             "bounding_stage": max(stages, key=stages.get),
             "blocks_per_s": n_blocks / (total * 1e-3),
             "pcm_frames_per_s": n * args.tracks / (total * 1e-3),
             "algorithmic_bytes": algo_bytes,
             "algorithmic_bytes_per_s": algo_bytes / (total * 1e-3),
             "fraction_of_8TBps": algo_bytes / (total * 1e-3) / HBM_BYTES_PER_S}
        if ref_s is not None:
            d["reference_s"] = ref_s
            d["speedup_over_reference_stages"] = ref_s / (total * 1e-3)
            d["speedup_over_reference_wall"] = ref_s / (wall * 1e-3)
        return d

    doc = {
        "shape": {"tracks": args.tracks, "seconds": args.seconds, "rate": rate, "channels": ch,
                  "bits_per_sample": bps, "block_size": block, "kind": "tone",
                  "distinct_signals": distinct, "blocks": n_blocks, "warmup": args.warmup,
                  "steps": args.steps, "device": torch.cuda.get_device_name(0)},
        "encode": side(enc_ms, enc_wall, "shn_total", pcm_in + image_bytes,
                       ref["encode_s"] if ref else None),
        "decode": side(dec_ms[default], dec_wall[default], "shnd_total", image_bytes + pcm_out,
                       ref["decode_s"] if ref else None),
        "decode_index_walk": {
            "default": default,
            "cooperative_index_ms": dec_ms["cooperative"]["shnd_index"],
            "serial_index_ms": dec_ms["serial"]["shnd_index"],
            "cooperative_total_ms": dec_ms["cooperative"]["shnd_total"],
            "serial_total_ms": dec_ms["serial"]["shnd_total"],
            "serial_over_cooperative": dec_ms["serial"]["shnd_index"] /
            dec_ms["cooperative"]["shnd_index"]},
        "encoded_bytes": image_bytes, "compression_ratio": image_bytes / pcm_in,
        "verify": {"tracks_decoded": len(dres), "tracks_differing_from_source": dec_bad,
                   "images_compared_with_shnenc": compared, "images_differing": differing},
        "reference": ("oracle/_ref/shnenc and shndec, %d processes at a time, same host"
                      % args.procs) if ref else "skipped: oracle/_ref/shnenc or shndec absent",
    }
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 1 if dec_bad or differing else 0


if __name__ == "__main__":
    sys.exit(main())
