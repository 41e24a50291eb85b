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

--encode runs the encoder leg instead and writes profiles/wavpack_enc_bench.json:
1024 tracks x 10 s of seeded tones and noise (every 8th track dual mono, every
16th silent in its second half) made on the device, encoded with the
"standard" and the "veryhigh" options of WavPackAudio, timed per kernel with
HIP events (atg_wv_encoder_kernel_times).  Every image is decoded on the GPU
and compared with its source (that decode, over varied content, is timed as a
row of its own); the first 4 tracks are byte-compared with oracle/_ref/wvenc,
and the reference time is wvenc at 16 processes, where that binary exists.
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


def make_tracks(torch, dev, n_tracks, n, rate):
    """int16 stereo on the device, (n_tracks, n, 2): two tones per channel and
    a little noise; every 8th track dual mono, every 16th silent from its
    middle on"""
    rng = np.random.default_rng(2024)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2024)
    out = torch.empty((n_tracks, n, 2), dtype=torch.int16, device=dev)
    t = torch.arange(n, device=dev, dtype=torch.float64)[None, :, None]
    for a in range(0, n_tracks, 32):
        b = min(n_tracks, a + 32)
        f1 = torch.tensor(rng.uniform(100, 400, (b - a, 1, 2)), device=dev)
        f2 = torch.tensor(rng.uniform(400, 1500, (b - a, 1, 2)), device=dev)
        x = 9000 * torch.sin(2 * np.pi * f1 * t / rate) + 5000 * torch.sin(2 * np.pi * f2 * t / rate)
        x = x + 2.0 * torch.randn(x.shape, generator=gen, device=dev, dtype=torch.float64)
        out[a:b] = torch.round(x).to(torch.int16)
    out[0::8, :, 1] = out[0::8, :, 0]
    out[4::16, n // 2:, :] = 0
    return out


def reference_encode(pcm_of, n_tracks, procs, opts, keep):
    """wvenc over the same tracks, `procs` at a time -> (seconds, the first
    `keep` images)"""
    enc = os.path.join(REF, "wvenc")
    if not os.path.exists(enc):
        return None, []
    with tempfile.TemporaryDirectory() as tmp:
        raw = [pcm_of(k) for k in range(n_tracks)]
        t0 = time.perf_counter()
        with concurrent.futures.ThreadPoolExecutor(procs) as ex:
            list(ex.map(lambda k: subprocess.run(
                [enc] + opts + [os.path.join(tmp, "%d.wv" % k)], input=raw[k],
                stdout=subprocess.DEVNULL, check=True), range(n_tracks)))
        secs = time.perf_counter() - t0
        images = []
        for k in range(min(keep, n_tracks)):
            with open(os.path.join(tmp, "%d.wv" % k), "rb") as f:
                images.append(f.read())
        return secs, images


def encode_leg(args):
    import torch
    from audiotools import WavPackAudio, _atgpu

    ch, bps, rate = 2, 16, 44100
    n = int(round(args.seconds * rate))
    torch.cuda.init()
    dev = torch.device("cuda:0")
    d_pcm = make_tracks(torch, dev, args.tracks, n, rate)
    torch.cuda.synchronize()
    tracks = [(k * n, n) for k in range(args.tracks)]
    enc = _atgpu.WvEncoder(0)
    dec = _atgpu.WvDecoder(0)
    host_pcm = d_pcm.cpu().numpy().reshape(args.tracks, -1)
    rows = {}
    for mode in ("standard", "veryhigh"):
        o = dict(WavPackAudio.__options__[mode])
        opts = enc.options(o["block_size"], o["correlation_passes"], o["false_stereo"],
                           o["wasted_bits"], o["joint_stereo"])
        nb = enc.block_count(tracks, ch, 3, o["block_size"])
        cap = args.tracks * n * ch * 2
        d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
        bsb = np.zeros(nb, dtype=np.uint32)
        times, walls = [], []
        for step in range(args.enc_warmup + args.enc_steps):
            t0 = time.perf_counter()
            try:
                res, need = enc.encode_device(opts, d_pcm.data_ptr(), _atgpu.PCM_S16, tracks, ch, 3,
                                              bps, rate, d_out.data_ptr(), cap, block_bytes=bsb)
            except _atgpu.ATGError as err:
                if err.status != _atgpu.ATG_ERR_CAPACITY:
                    raise
                cap = err.needed
                d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
                res, need = enc.encode_device(opts, d_pcm.data_ptr(), _atgpu.PCM_S16, tracks, ch, 3,
                                              bps, rate, d_out.data_ptr(), cap, block_bytes=bsb)
            wall = time.perf_counter() - t0
            if step >= args.enc_warmup:
                times.append(enc.kernel_times())
                walls.append(wall * 1e3)
        ms = mean_times(times)
        total = ms["wv_total"]
        kernels = {k: v for k, v in ms.items() if k != "wv_total"}
        # every image through the GPU decoder, against its source
        blob = d_out[:need].cpu().numpy()
        dtracks = []
        for r in res:
            img = blob[r.out_offset:r.out_offset + r.bytes].tobytes()
            st, info, blocks = _atgpu.wv_read_info(img)
            assert st == 0 and info.end_status == 0
            dtracks.append(_atgpu.wv_dec_track(r.out_offset, r.bytes, info, blocks, check_md5=0))
        drows = []
        for step in range(1 + args.enc_steps):
            dres, _, nsamp = dec.decode_device(d_out.data_ptr(), need, dtracks)
            if step:
                drows.append(dec.kernel_times())
        dms = mean_times(drows)
        pcm = dec.fetch(nsamp)
        bad = 0
        for k, r in enumerate(dres):
            got = pcm[r.sample_offset:r.sample_offset + r.pcm_frames * ch]
            if r.status != 0 or not np.array_equal(got, host_pcm[k]):
                bad += 1
        del pcm
        wvenc_opts = ["-c", "2", "-m", "3", "-r", str(rate), "-b", "16", "-B",
                      str(o["block_size"]), "-p", str(o["correlation_passes"]), "-j", "-f", "-w"]
        ref_s, ref_images = (None, []) if args.no_reference else reference_encode(
            lambda k: host_pcm[k].tobytes(), args.tracks, args.procs, wvenc_opts, 4)
        differing = sum(
            1 for k, img in enumerate(ref_images)
            if blob[res[k].out_offset:res[k].out_offset + res[k].bytes].tobytes() != img)
        row = {"options": o, "kernel_ms": ms, "wall_ms_per_batch": float(np.mean(walls)),
               "kernel_share": {k: v / total for k, v in kernels.items()},
               "bounding_kernel": max(kernels, key=kernels.get),
               "chain_layout": "one wave per stream: a lane per pass as a pipeline, one lane for "
                               "the walk",
               "wavpack_blocks": nb, "wavpack_blocks_per_s": nb / (total * 1e-3),
               "pcm_frames_per_s": n * args.tracks / (total * 1e-3),
               "encoded_bytes": int(need),
               "compression_ratio": float(need) / (n * ch * 2 * args.tracks),
               "verify": {"tracks_decoded": len(dres), "tracks_differing_from_source": bad,
                          "compared_with_wvenc": len(ref_images),
                          "differing_from_wvenc": differing},
               "decode_of_these_images": {"kernel_ms": dms, "wavpack_blocks_per_s":
                                          nb / (dms["wvd_total"] * 1e-3)},
               "reference": ("oracle/_ref/wvenc, %d processes at a time, same host" % args.procs)
               if ref_s is not None else "skipped: oracle/_ref/wvenc absent"}
        if ref_s is not None:
            row["reference_s"] = ref_s
            row["speedup_over_reference_kernels"] = ref_s / (total * 1e-3)
            row["speedup_over_reference_wall"] = ref_s / (row["wall_ms_per_batch"] * 1e-3)
        rows[mode] = row
        del d_out
    enc.close()
    dec.close()
    doc = {"shape": {"tracks": args.tracks, "seconds": n / rate, "rate": rate, "channels": ch,
                     "bits_per_sample": bps, "warmup": args.enc_warmup, "steps": args.enc_steps,
                     "device": torch.cuda.get_device_name(0)},
           "input": "seeded tones and noise made on the device; every 8th track dual mono, "
                    "every 16th silent from its middle on",
           "encode": rows}
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles",
                                                                "wavpack_enc_bench.json")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")
    failed = any(r["verify"]["tracks_differing_from_source"] or r["verify"]["differing_from_wvenc"]
                 for r in rows.values())
    return 1 if failed else 0


DEFAULT_OUT = os.path.join(ROOT, "profiles", "wavpack_bench.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--encode", action="store_true", help="run the encoder leg instead")
    ap.add_argument("--enc-warmup", type=int, default=1)
    ap.add_argument("--enc-steps", type=int, default=3)
    args = ap.parse_args()
    if args.encode:
        return encode_leg(args)

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
