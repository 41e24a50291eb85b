#!/usr/bin/env python3
"""Windowed batch decoding (audiotools/windows.py, csrc/flac_index.hip) against
what the whole-file entry points can do for the same request.

Shape: `--files` FLAC-8 files of `--minutes` min, 44.1 kHz 16-bit stereo, made
by the GPU encoder (save_flac_batch, `--distinct` signals repeated), once with
from_pcm's SEEKTABLE (a point per 10 s) and once with the SEEKTABLE taken out;
`--per-file` one-second windows per file at seeded starts.

1. Calls: decode_windows_batch of all the windows against load_batch of the
   whole files followed by a slice per window, alternating in one process,
   `--rounds` timed rounds after a warm-up round; four rows compared after
   the clock.  The ms per call, the uploaded bytes and the decoded frames of
   both are recorded.
2. The index kernels alone: atg_flac_index_device over the whole frame regions
   of the files in device memory, its stage times from
   atg_flac_index_kernel_times, its bytes per second against the 8 TB/s
   roofline; beside it the decoder's front on the same bytes from
   atg_decoder_kernel_times: dec_scan is k_dec_sync + k_dec_hdr, dec_parse
   holds k_dec_spec together with the parse and its CRC pass (the decoder
   times them as one stage).  Sync + header are set against dec_scan, like
   for like; the confirm stage is reported on its own.

Every miss (the windowed path not faster at this shape, the index's scan more
than 1.5x the decoder's) is listed under "misses", for the documents to state
in bold.

Writes one JSON document (--out, default profiles/window_bench.json) and
prints it.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-audio-tools_amd"), os.path.join(ROOT, "tests")]
HBM_BYTES_PER_S = 8e12  # MI355X peak


def stats(ms):
    return {"mean_ms": float(np.mean(ms)), "median_ms": float(np.median(ms)),
            "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "rounds": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--per-file", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--index-steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_bench.json"))
    args = ap.parse_args()

    import torch
    import audiotools
    from audiotools import _atgpu, flac, tensors  # noqa: F401  (tensors: torch comes up first)

    rate, ch = 44100, 2
    n = int(args.minutes * 60 * rate)
    length = rate
    dev = torch.device("cuda:0")
    distinct = min(args.distinct, args.files)
    t = torch.arange(n, device=dev, dtype=torch.float64)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    audio = torch.empty((distinct, ch, n), dtype=torch.float32, device=dev)
    for k in range(distinct):
        for c in range(ch):
            tone = 0.3 * torch.sin(t * (0.02 + 0.011 * k + 0.007 * c)) + \
                0.2 * torch.sin(t * (0.31 + 0.05 * c))
            audio[k, c] = (tone + 0.002 * torch.randn(n, device=dev, generator=g,
                                                      dtype=torch.float64)).float()
    bad = 0
    misses = []  # what the README and DESIGN state in bold
    doc = {"device": torch.cuda.get_device_name(0),
           "shape": {"files": args.files, "distinct_signals": distinct, "minutes": args.minutes,
                     "frames_per_file": n, "windows": args.files * args.per_file,
                     "window_frames": length,
                     "source": "16-bit / 44.1 kHz stereo, FLAC-8, block 4096"}}
    rnd = np.random.default_rng(args.seed)
    starts = [int(s) for s in rnd.integers(0, n - length, args.files * args.per_file)]
    with tempfile.TemporaryDirectory() as d:
        first = [os.path.join(d, "d%d.flac" % k) for k in range(distinct)]
        made = audiotools.save_flac_batch(audio, [n] * distinct, first, rate, 16, compression="8")
        bad += sum(isinstance(m, Exception) for m in made)
        del audio, t
        torch.cuda.empty_cache()
        sets = {"seektable": [], "no_seektable": []}
        for k in range(args.files):
            a = os.path.join(d, "s%d.flac" % k)
            shutil.copyfile(first[k % distinct], a)
            sets["seektable"].append(a)
            data = open(a, "rb").read()
            blocks, frames_at = flac._blocks(data)
            b = os.path.join(d, "b%d.flac" % k)
            with open(b, "wb") as f:
                f.write(flac._build([x for x in blocks if x[0] != flac.SEEKTABLE]) +
                        data[frames_at:])
            sets["no_seektable"].append(b)
        for name, files in sets.items():
            rows = [files[k // args.per_file] for k in range(len(starts))]
            kept = {}

            def windowed():
                if "win" in kept:
                    kept.pop("win").close()
                kept["win"] = audiotools.decode_windows_batch(rows, starts, length)

            def whole():
                kept.pop("whole", None)
                batch = audiotools.load_batch(files, dtype=torch.int32)
                kept["whole"] = [batch.audio[k // args.per_file, :, s:s + length]
                                 for k, s in enumerate(starts)]
                torch.cuda.synchronize()

            ms = {"decode_windows_batch": [], "load_batch_then_slice": []}
            for step in range(1 + args.rounds):
                for label, fn in (("decode_windows_batch", windowed),
                                  ("load_batch_then_slice", whole)):
                    t0 = time.perf_counter()
                    fn()
                    if step:
                        ms[label].append((time.perf_counter() - t0) * 1e3)
            win = kept["win"]
            picks = sorted(set(int(v) for v in np.linspace(0, len(starts) - 1, 4)))
            same = 0
            for k in picks:
                got = win.fetch(k).reshape(length, ch).T
                same += bool(np.array_equal(got, kept["whole"][k].cpu().numpy()))
            bad += same != len(picks)
            bad += sum(e is not None for e in win.errors)
            body = sum(os.path.getsize(f) for f in files)
            entry = {
                "decode_windows_batch": dict(
                    stats(ms["decode_windows_batch"]), uploaded_bytes=int(win.uploaded_total),
                    decoded_frames=int(sum(s["decoded_frames"] for s in win.stats))),
                "load_batch_then_slice": dict(
                    stats(ms["load_batch_then_slice"]), uploaded_bytes=int(body),
                    decoded_frames=int(n * len(files))),
                "rows_compared": len(picks), "rows_identical": same,
            }
            entry["whole_over_windowed"] = (entry["load_batch_then_slice"]["mean_ms"] /
                                            entry["decode_windows_batch"]["mean_ms"])
            entry["windowed_is_faster"] = bool(entry["whole_over_windowed"] > 1.0)
            if not entry["windowed_is_faster"]:
                misses.append("%s: the windowed path is not faster at this shape (%.1f ms "
                              "against %.1f ms)" % (name, entry["decode_windows_batch"]["mean_ms"],
                                                    entry["load_batch_then_slice"]["mean_ms"]))
            doc[name] = entry
            kept.pop("win").close()
            kept.clear()
            torch.cuda.empty_cache()

        # the index kernels alone, and the decoder's front on the same bytes
        infos, bodies = [], []
        for f in sets["no_seektable"]:
            data = open(f, "rb").read()
            si = _atgpu.read_metadata(data)[1]
            infos.append(si)
            bodies.append(data[si.frames_offset:])
        blob, spans = _atgpu.pack_images(bodies)
        buf = torch.frombuffer(bytearray(blob + bytes(64)), dtype=torch.uint8).to(dev)
        ranges = [_atgpu.flac_index_range(o, nb, si) for (o, nb), si in zip(spans, infos)]
        tracks = [_atgpu.dec_track(o, nb, si) for (o, nb), si in zip(spans, infos)]
        scanned = sum(nb for _, nb in spans)
        ix = {"sync": [], "header": [], "confirm": []}
        front = {"dec_scan": [], "dec_parse": []}
        entries = 0
        for step in range(1 + args.index_steps):
            found = _atgpu.flac_index_device(buf.data_ptr(), len(blob), ranges, cap=1 << 20)
            a = _atgpu.flac_index_kernel_times()
            _atgpu.decoder().decode_device(buf.data_ptr(), len(blob), tracks)
            b = _atgpu.decoder().kernel_times()
            if step:
                entries = len(found)
                for k in ix:
                    ix[k].append(a[k])
                for k in front:
                    front[k].append(b[k])
        frames = sum((int(si.total_samples) + 4095) // 4096 for si in infos)
        bad += entries != frames
        total = [sum(v) for v in zip(*ix.values())]
        scan = [a + b for a, b in zip(ix["sync"], ix["header"])]
        per_s = scanned / (np.mean(total) * 1e-3)
        doc["index_kernels"] = {
            "bytes": int(scanned), "entries": entries, "frames_in_the_files": frames,
            "stages": {k: stats(v) for k, v in ix.items()}, "all_stages": stats(total),
            "bytes_per_s": per_s, "fraction_of_8TBps": per_s / HBM_BYTES_PER_S,
            "decoder_front_same_bytes": {k: stats(v) for k, v in front.items()},
            "sync_and_header": dict(stats(scan),
                                    bytes_per_s=scanned / (np.mean(scan) * 1e-3)),
            "sync_and_header_over_dec_scan": float(np.mean(scan) / np.mean(front["dec_scan"])),
            "confirm_over_dec_parse": float(np.mean(ix["confirm"]) / np.mean(front["dec_parse"])),
            "note": "like for like: the index's sync + header stages against dec_scan "
                    "(k_dec_sync + k_dec_hdr).  The confirm stage does what k_dec_spec does and "
                    "checks the frame numbers; the decoder times k_dec_spec inside dec_parse "
                    "together with the subframe parse and its CRC pass, so confirm_over_dec_parse "
                    "sets it against more work than its own",
        }
        ik = doc["index_kernels"]
        if ik["sync_and_header_over_dec_scan"] > 1.5:
            misses.append("the index's sync + header stages take %.2fx the decoder's dec_scan on "
                          "the same bytes" % ik["sync_and_header_over_dec_scan"])
    doc["misses"] = misses
    doc["verify"] = {"mismatches": int(bad)}
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
