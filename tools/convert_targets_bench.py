#!/usr/bin/env python3
"""convert_files_batch to every target type against the reader path.

`--files` ten-second 24-bit / 96 kHz stereo .flac files (README's shape) to
16-bit / 44.1 kHz, once per target type: audiotools.convert_files_batch with
target_types=<type> against cls.from_pcm over PCMConverter, one file after
another, under an all-zero dither, one timed round each after a warm-up round
of 4 files; the files must be identical (an Ogg FLAC reference is given the
serial number the batch drew, and the clock an .m4a is stamped with stands
still).  Then the FLAC target once more with dither=DeviceDither against the
default os.urandom.

Writes one JSON document (--out, default profiles/convert_targets_bench.json)
and prints it.
"""
import argparse
import functools
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-audio-tools_amd"), os.path.join(ROOT, "tests")]

TYPES = ["flac", "oga", "m4a", "tta", "wv", "shn", "wav", "aiff", "au"]


def zeros(n):
    return b"\0" * n


def read(path):
    with open(path, "rb") as f:
        return f.read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--types", default=",".join(TYPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_targets_bench.json"))
    args = ap.parse_args()

    import torch
    import oracle_port
    import signals
    import audiotools
    from audiotools import _atgpu, encoders, pcmconverter
    from audiotools.targets import SUFFIXES

    torch.cuda.init()
    audiotools.m4a.time = types.SimpleNamespace(time=lambda: 1.7e9)
    rate_in, n_in = 96000, 960000
    distinct = min(args.distinct, args.files)
    pcms = [signals.make("tone", n_in, 2, 24, seed=300 + k) for k in range(distinct)]
    eng = _atgpu.engine()
    opts = _atgpu.make_options(**oracle_port.PRESETS["8"])
    enc, eres, _, _ = eng.encode(opts, np.concatenate(pcms).astype(np.int32),
                                 [(k * n_in, n_in) for k in range(distinct)], 2, 24, rate_in)
    images = [enc[r.out_offset:r.out_offset + r.bytes].tobytes() for r in eres]
    n_out = _atgpu.resample_output_frames(n_in, 2, rate_in, 44100)
    target = dict(sample_rate=44100, bits_per_sample=16)
    bad, rows = 0, {}
    with tempfile.TemporaryDirectory() as d:
        srcs = []
        for k in range(args.files):
            srcs.append(os.path.join(d, "s%d.flac" % k))
            with open(srcs[-1], "wb") as f:
                f.write(images[k % distinct])

        def on_readers(suffix, m, dev_t, ref_t):
            cls = SUFFIXES[suffix]
            for s, got, t in zip(srcs[:m], dev_t[:m], ref_t[:m]):
                reader = audiotools.PCMConverter(
                    audiotools.BufferedPCMReader(audiotools.FlacAudio(s).to_pcm()), 44100, 2, 0x3,
                    16)
                reader._rand = zeros
                kw = {}
                if suffix == "oga":
                    kw = dict(encoding_function=functools.partial(
                        encoders.encode_oggflac,
                        serial_number=int.from_bytes(read(got)[14:18], "little")))
                elif suffix == "wv":
                    kw = dict(encoding_function=encoders.encode_wavpack)
                cls.from_pcm(t, reader, None, total_pcm_frames=n_out, **kw)

        for suffix in args.types.split(","):
            dev_t = [os.path.join(d, "d%d.%s" % (k, suffix)) for k in range(args.files)]
            ref_t = [os.path.join(d, "r%d.%s" % (k, suffix)) for k in range(args.files)]
            ms = {}
            for step, m in enumerate((min(4, args.files), args.files)):
                t0 = time.perf_counter()
                got = audiotools.convert_files_batch(srcs[:m], dev_t[:m], dither=zeros,
                                                     target_types=suffix, **target)
                ms["convert_files_batch"] = (time.perf_counter() - t0) * 1e3
                bad += sum(not isinstance(x, SUFFIXES[suffix]) for x in got)
                t0 = time.perf_counter()
                on_readers(suffix, m, dev_t, ref_t)
                ms["reader_path"] = (time.perf_counter() - t0) * 1e3
            identical = sum(read(a) == read(b) for a, b in zip(dev_t, ref_t))
            bad += identical != args.files
            rows[suffix] = dict(convert_files_batch_ms=ms["convert_files_batch"],
                                reader_path_ms=ms["reader_path"],
                                readers_over_batch=ms["reader_path"] / ms["convert_files_batch"],
                                files_identical=identical,
                                bytes_written=sum(os.path.getsize(t) for t in dev_t))
            for t in dev_t + ref_t:
                os.unlink(t)

        # FLAC once more: the bits made on the device against os.urandom
        dev_t = [os.path.join(d, "x%d.flac" % k) for k in range(args.files)]
        dith = {}
        for name, make in (("DeviceDither", lambda: pcmconverter.DeviceDither(7)),
                           ("os.urandom", lambda: None)):
            for m in (min(4, args.files), args.files):
                t0 = time.perf_counter()
                got = audiotools.convert_files_batch(srcs[:m], dev_t[:m], dither=make(), **target)
                dith[name + "_ms"] = (time.perf_counter() - t0) * 1e3
                bad += sum(not isinstance(x, audiotools.FlacAudio) for x in got)
    dith["urandom_over_device"] = dith["os.urandom_ms"] / dith["DeviceDither_ms"]
    doc = {
        "device": torch.cuda.get_device_name(0), "files": args.files,
        "distinct_signals": distinct,
        "source": "24-bit / 96 kHz stereo, %d frames, FLAC-8" % n_in,
        "target": "16-bit / 44.1 kHz stereo, %d frames, all-zero dither, each type's default "
                  "compression" % n_out,
        "types": rows, "flac_dither": dith, "verify": {"mismatches": int(bad)},
        "note": "one timed round per path and type after a warm-up round of 4 files; the reader "
                "path is cls.from_pcm(PCMConverter(BufferedPCMReader(FlacAudio.to_pcm()))), one "
                "file after another, with encode_oggflac / encode_wavpack as the encoding "
                "function of those two classes",
    }
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
