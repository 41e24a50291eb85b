#!/usr/bin/env python3
"""split_image_batch and join_tracks_batch (audiotools/cdimage.py) against
the per-track reader path they replace.

Shape: `--images` FLAC-8 CD images of `--minutes` min, 44.1 kHz 16-bit stereo,
made by the GPU encoder (save_flac_batch) from seeded signals, each with a
sheet of `--tracks` tracks at seeded CD sector boundaries.

1. split_image_batch of all the images to FLAC-8 tracks, alternating with the
   reader path -- FlacAudio.from_pcm(PCMReaderWindow(image.to_pcm(), offset,
   length)) once per track -- on the first `--reader-images` images only (it
   is slow); a warm-up round and `--rounds` timed rounds.  Four files are
   compared byte for byte after the clock.
2. join_tracks_batch of every image's tracks back into one FLAC-8 image with
   the sheet embedded, the same rounds; one image is compared with the file
   the split began with (its PCM through the decoder's MD5, its sheet through
   get_cuesheet).

The call times are split into their parts by wrapping the stages the calls
go through, on the host clock: upload (Engine.copy_to_device), decode
(_Batch.decode without its uploads: every image's frames and its stream's MD5,
one serial chain per stream), chain (run_chain_device), encode (write_tracks
without the finishing), host finishing (convert._finish: the SEEKTABLE walk of
every encoded track, which decodes it once more, the metadata rewrite and the
file write; set_cuesheet in the join) and, in the join, the device copies that
lay an album's pieces end to end.  The decoder's own stage times of the last
decode call are recorded beside them.

Writes one JSON document (--out, default profiles/split_bench.json) and
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
sys.path.insert(0, os.path.join(ROOT, "python-audio-tools_amd"))
SECTOR = 588


def stats(ms):
    return {"mean_ms": float(np.mean(ms)), "median_ms": float(np.median(ms)),
            "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "rounds": len(ms)}


class Parts(object):
    """host-clock time spent inside wrapped functions, by label; a function
    wrapped with `within` counts only while the function of that label runs"""

    def __init__(self):
        self.ms, self.extra, self.inside = {}, {}, []

    def wrap(self, owner, name, label, after=None, within=None):
        real = getattr(owner, name)

        def timed(*args, **kw):
            if within is not None and within not in self.inside:
                return real(*args, **kw)
            self.inside.append(label)
            t0 = time.perf_counter()
            try:
                return real(*args, **kw)
            finally:
                self.ms[label] = self.ms.get(label, 0.0) + (time.perf_counter() - t0) * 1e3
                self.inside.remove(label)
                if after is not None:
                    after(self)
        setattr(owner, name, timed)

    def take(self):
        out, extra = self.ms, self.extra
        self.ms, self.extra = {}, {}
        return out, extra


def findings(doc):
    """what the documents state in bold, from the numbers alone"""
    out = []
    for name, call in (("split", "split_image_batch"), ("join", "join_tracks_batch")):
        entry = doc[name]
        share = entry["share_of_call"]
        top = max(share, key=share.get)
        stages = entry[call]["parts_ms"].get("decoder_stages_ms", {})
        out.append("%s: %s is %.0f%% of the call (%.0f of %.0f ms); the batch decode with its "
                   "per-stream MD5 is %.0f%%, upload %.1f%%, the chain %.2f%%, the encode %.0f%%%s"
                   % (call, top, 100 * share[top], entry[call]["parts_ms"][top],
                      entry[call]["mean_ms"], 100 * share["decode_and_md5"], 100 * share["upload"],
                      100 * share["chain"], 100 * share["encode"],
                      ", the device copies %.4f%%" % (100 * share["device_copies"])
                      if "device_copies" in share else ""))
        if stages.get("dec_total"):
            out.append("%s: inside the batch decode the MD5 stage is %.0f%% of the decoder's "
                       "kernel time (%.0f of %.0f ms)"
                       % (call, 100 * stages["dec_md5"] / stages["dec_total"], stages["dec_md5"],
                          stages["dec_total"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1)
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--tracks", type=int, default=15)
    ap.add_argument("--reader-images", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reader-rounds", type=int, default=None,
                    help="timed rounds in which the reader path runs too (default: all of them "
                         "and the warm-up; fewer: the first of them, without a warm-up)")
    ap.add_argument("--seed", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_bench.json"))
    args = ap.parse_args()
    if args.reader_rounds is None:
        args.reader_rounds = args.rounds
    args.reader_images = min(args.reader_images, args.images)

    import torch
    import audiotools
    from audiotools import _atgpu, batchfiles, cdimage, convert, tensors  # noqa: F401
    from fractions import Fraction
    from audiotools import Sheet, SheetIndex, SheetTrack

    def sheet_at(rate, starts, pregaps):
        """tracks whose index 1 are at the PCM frames `starts`; pregaps:
        {track number: PCM frame of its index 0}"""
        tracks = []
        for k, at in enumerate(starts):
            indexes = [SheetIndex(1, Fraction(at, rate))]
            if k + 1 in pregaps:
                indexes.insert(0, SheetIndex(0, Fraction(pregaps[k + 1], rate)))
            tracks.append(SheetTrack(k + 1, indexes))
        return Sheet(tracks)

    rate, ch = 44100, 2
    sectors = int(args.minutes * 60 * 75)
    n = sectors * SECTOR
    dev = torch.device("cuda:0")
    rnd = np.random.default_rng(args.seed)
    doc = {"device": torch.cuda.get_device_name(0),
           "shape": {"images": args.images, "minutes": args.minutes, "frames_per_image": n,
                     "tracks_per_image": args.tracks, "reader_path_images": args.reader_images,
                     "rounds": args.rounds, "reader_path_rounds": args.reader_rounds,
                     "source": "16-bit / 44.1 kHz stereo, FLAC-8, block 4096",
                     "targets": "FLAC-8"}}
    bad = 0
    parts = Parts()

    def decoder_times(p):
        p.extra["decoder_stages_ms"] = _atgpu.decoder().kernel_times()
    parts.wrap(_atgpu.Engine, "copy_to_device", "upload", within="decode_with_upload")
    parts.wrap(batchfiles._Batch, "decode", "decode_with_upload", after=decoder_times)
    parts.wrap(cdimage, "run_chain_device", "chain")
    parts.wrap(cdimage, "write_tracks", "write_tracks")
    parts.wrap(convert, "_finish", "host_finishing")
    parts.wrap(cdimage, "_lay_out", "device_copies")
    parts.wrap(audiotools.FlacAudio, "set_cuesheet", "set_cuesheet")

    def breakdown(ms, extra, call_ms):
        out = {"upload": ms.get("upload", 0.0),
               "decode_and_md5": ms.get("decode_with_upload", 0.0) - ms.get("upload", 0.0),
               "chain": ms.get("chain", 0.0),
               "encode": ms.get("write_tracks", 0.0) - ms.get("host_finishing", 0.0),
               "host_finishing": ms.get("host_finishing", 0.0) + ms.get("set_cuesheet", 0.0)}
        if "device_copies" in ms:
            out["device_copies"] = ms["device_copies"]
        out["other"] = call_ms - sum(out.values())
        out.update(extra)
        return out

    with tempfile.TemporaryDirectory() as d:
        images, sheets, cuts = [], [], []
        t = torch.arange(n, device=dev, dtype=torch.float64)
        g = torch.Generator(device=dev)
        g.manual_seed(args.seed)
        for k in range(args.images):
            audio = torch.empty((1, ch, n), dtype=torch.float32, device=dev)
            for c in range(ch):
                tone = 0.3 * torch.sin(t * (0.02 + 0.011 * k + 0.007 * c)) + \
                    0.2 * torch.sin(t * (0.31 + 0.05 * c))
                audio[0, c] = (tone + 0.002 * torch.randn(n, device=dev, generator=g,
                                                          dtype=torch.float64)).float()
            path = os.path.join(d, "image%02d.flac" % k)
            made = audiotools.save_flac_batch(audio, [n], [path], rate, 16, compression="8")
            bad += isinstance(made[0], Exception)
            images.append(path)
            starts = [0] + sorted(int(s) * SECTOR for s in rnd.choice(
                np.arange(150, sectors - 150), args.tracks - 1, replace=False))
            # an index 0 two seconds in front of every third track
            sheets.append(sheet_at(rate, starts, {j + 1: starts[j] - 150 * SECTOR
                                                  for j in range(2, args.tracks, 3)
                                                  if starts[j] - 150 * SECTOR > starts[j - 1]}))
            cuts.append(cdimage.plan_split(sheets[-1], n, rate))
            del audio
            print("image %d of %d written" % (k + 1, args.images), file=sys.stderr, flush=True)
        del t
        torch.cuda.empty_cache()
        doc["shape"]["image_bytes"] = int(sum(os.path.getsize(p) for p in images))

        split_to = [[os.path.join(d, "split%02d.%02d.flac" % (k, j)) for j in range(args.tracks)]
                    for k in range(args.images)]
        reader_to = [[os.path.join(d, "reader%02d.%02d.flac" % (k, j))
                      for j in range(args.tracks)] for k in range(args.reader_images)]
        joined = [os.path.join(d, "joined%02d.flac" % k) for k in range(args.images)]

        def split():
            got = audiotools.split_image_batch(images, split_to, sheets, compression="8")
            return sum(1 for r in got if not isinstance(r, cdimage.SplitResult) or
                       any(isinstance(x, Exception) for x in r.tracks))

        def reader_path():
            for k in range(args.reader_images):
                source = audiotools.FlacAudio(images[k])
                for (offset, length), target in zip(cuts[k], reader_to[k]):
                    audiotools.FlacAudio.from_pcm(
                        target, audiotools.PCMReaderWindow(source.to_pcm(), offset, length), "8",
                        total_pcm_frames=length)
            return 0

        def join():
            got = audiotools.join_tracks_batch(split_to, joined, sheets, compression="8")
            return sum(isinstance(r, Exception) for r in got)

        def rounds(calls):
            ms = {label: [] for label, _ in calls}
            detail = {label: [] for label, _ in calls}
            failed = 0
            for step in range(1 + args.rounds):
                for label, fn in calls:
                    if label == "reader_path" and args.reader_rounds < args.rounds and \
                            not 1 <= step <= args.reader_rounds:
                        continue
                    parts.take()
                    t0 = time.perf_counter()
                    failed += fn()
                    call_ms = (time.perf_counter() - t0) * 1e3
                    print("round %d %s: %.0f ms" % (step, label, call_ms), file=sys.stderr,
                          flush=True)
                    if step:
                        ms[label].append(call_ms)
                        detail[label].append(breakdown(*parts.take(), call_ms=call_ms))
            return ms, detail, failed

        def mean_parts(rows):
            keys = [k for k in rows[0] if not isinstance(rows[0][k], dict)]
            out = {k: float(np.mean([r[k] for r in rows])) for k in keys}
            for k in rows[0]:
                if isinstance(rows[0][k], dict):
                    out[k] = {s: float(np.mean([r[k].get(s, 0.0) for r in rows]))
                              for s in rows[0][k]}
            return out

        ms, detail, failed = rounds([("split_image_batch", split), ("reader_path", reader_path)])
        bad += failed
        n_tracks = args.images * args.tracks
        entry = {"split_image_batch": dict(stats(ms["split_image_batch"]), tracks=n_tracks,
                                           parts_ms=mean_parts(detail["split_image_batch"])),
                 "reader_path": dict(stats(ms["reader_path"]),
                                     tracks=args.reader_images * args.tracks)}
        per_track = entry["split_image_batch"]["mean_ms"] / n_tracks
        per_track_reader = entry["reader_path"]["mean_ms"] / (args.reader_images * args.tracks)
        entry["ms_per_track"] = {"split_image_batch": per_track, "reader_path": per_track_reader}
        entry["reader_over_batch_per_track"] = per_track_reader / per_track
        picks = [(k, j) for k in range(args.reader_images)
                 for j in sorted(set([0, args.tracks // 3, 2 * args.tracks // 3,
                                      args.tracks - 1]))][:4]
        same = 0
        for k, j in picks:
            with open(split_to[k][j], "rb") as a, open(reader_to[k][j], "rb") as b:
                same += a.read() == b.read()
        entry["files_compared"], entry["files_identical"] = len(picks), same
        bad += same != len(picks)
        call = entry["split_image_batch"]["mean_ms"]
        p = entry["split_image_batch"]["parts_ms"]
        entry["share_of_call"] = {k: v / call for k, v in p.items() if not isinstance(v, dict)}
        doc["split"] = entry

        ms, detail, failed = rounds([("join_tracks_batch", join)])
        bad += failed
        entry = {"join_tracks_batch": dict(stats(ms["join_tracks_batch"]), albums=args.images,
                                           pieces=n_tracks,
                                           parts_ms=mean_parts(detail["join_tracks_batch"]))}
        call = entry["join_tracks_batch"]["mean_ms"]
        p = entry["join_tracks_batch"]["parts_ms"]
        entry["share_of_call"] = {k: v / call for k, v in p.items() if not isinstance(v, dict)}
        back = audiotools.FlacAudio(joined[0])
        first = audiotools.FlacAudio(images[0])
        entry["joined_image_equals_source"] = bool(
            bytes(back._si.md5) == bytes(first._si.md5) and back.total_frames() == n and
            back.get_cuesheet() == sheets[0] and back.verify())
        bad += not entry["joined_image_equals_source"]
        doc["join"] = entry

    doc["verify"] = {"mismatches": int(bad)}
    doc["findings"] = findings(doc)
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
