#!/usr/bin/env python3
"""Generate tests/golden/dvda_vectors.json with the REFERENCE DVD-Audio
title decoder.

The reference's src/decoders/aob.c carries a -DSTANDALONE main (aobdec
<AUDIO_TS> <titleset> <start sector> <end sector> <PTS ticks>, little-endian
signed PCM on stdout); this script compiles it into oracle/_ref/aobdec (which
is outside git) with the flags of oracle/Makefile, where the reference tree
is present.

Vectors: the cases of tests/dvda_cases.py, and every single-bit flip of the
non-payload bytes of its two 5-sector images -> aobdec's return code (or the
negated signal, or "timeout"), its stderr without the frame count line, and
the length and MD5 of the PCM it wrote.  Images are rebuilt from the specs
by the tests (tests/dvda_build.py), so no AOB file is kept.  aobdec runs
under a time limit and an address-space limit.  A flip on which it dies or
runs into a limit, or which types the title MLP (decoded by the reference,
not built here yet), is set aside from the comparison with the reference and
counted; the script fails if more than 2 % of a sweep is.  A flip after
which the second request passes the end of the sectors (it changed the
layout, the rate or a pad size) is listed under "replay": the reference
replays its last packet there, which is not reproduced, so only the frames
present are compared.

tests/aob_port.py is run over every vector; the script exits non-zero where
it disagrees with the reference outside the deviations DESIGN 4p lists.
"""
import hashlib
import json
import os
import resource
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [TESTS]
import aob_port  # noqa: E402
import dvda_build  # noqa: E402
import dvda_cases  # noqa: E402

REF = os.environ.get("DVDA_REFERENCE", "/root/reference")
REF_BIN = os.path.join(ROOT, "oracle", "_ref")
AOBDEC = os.path.join(REF_BIN, "aobdec")
OUT = os.path.join(HERE, "dvda_vectors.json")
CFLAGS = ["-O2", "-ffp-contract=off", "-w", "-DSTANDALONE", "-DVERSION=2.22alpha1"]
SOURCES = ["decoders/aob.c", "decoders/mlp.c", "decoders/aobpcm.c", "array.c", "pcm.c",
           "pcmconv.c", "bitstream.c", "huffman.c", "buffer.c", "func_io.c"]
TIME_LIMIT = 10
ADDRESS_SPACE = 1 << 30
# every flip is asked twice: for fewer frames than the first sector alone
# holds, and for what the undamaged image holds less FLIP_MARGIN bytes: one
# flipped bit of a pad size takes 128 bytes of payload at the most, so the
# sectors never run out (the reference would replay its last packet)
FLIP_PTS_FRAMES = 100
FLIP_MARGIN = 256


def build_reference():
    src = os.path.join(REF, "src")
    if not os.path.isdir(src):
        return os.path.exists(AOBDEC)
    os.makedirs(REF_BIN, exist_ok=True)
    if not os.path.exists(AOBDEC):
        subprocess.check_call(["gcc"] + CFLAGS + ["-I" + src, "-o", AOBDEC] +
                              [os.path.join(src, c) for c in SOURCES] + ["-lm"])
    return True


def limits():
    resource.setrlimit(resource.RLIMIT_AS, (ADDRESS_SPACE, ADDRESS_SPACE))


def write_aobs(tmp, image, split):
    for name in os.listdir(tmp):
        os.unlink(os.path.join(tmp, name))
    cut = len(image) if split is None else split * dvda_build.SECTOR
    for i, part in enumerate([image[:cut], image[cut:]]):
        if part:
            with open(os.path.join(tmp, "ATS_01_%d.AOB" % (i + 1)), "wb") as f:
                f.write(part)


def ref_decode(tmp, image, first, pts, split=None):
    """-> (return code, or the negated signal, or "timeout"; stderr; PCM)"""
    write_aobs(tmp, image, split)
    n = len(image) // dvda_build.SECTOR
    try:
        p = subprocess.run([AOBDEC, tmp, "1", str(first), str(n), str(pts)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIME_LIMIT,
                           preexec_fn=limits)
    except subprocess.TimeoutExpired:
        return "timeout", "", b""
    err = "".join(l for l in p.stderr.decode("ascii", "replace").splitlines(True)
                  if not l.startswith("frames remaining"))
    return p.returncode, err, p.stdout


def record(rc, err, pcm):
    return {"returncode": rc, "stderr": err, "md5": hashlib.md5(pcm).hexdigest(),
            "bytes": len(pcm)}


def agrees(rc, err, pcm, image, first, pts):
    """the port's answer in aobdec's terms against the reference's"""
    raw, text, _ = aob_port.reference_answer(image, pts, first)
    return rc == 0 and raw == pcm and text == err


def main():
    if not build_reference():
        print("reference sources absent: nothing generated")
        return 1
    bad = 0
    titles, sweeps = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, spec, first, frames, split in dvda_cases.title_cases():
            image, _ = dvda_cases.case_image(spec, first)
            pts = dvda_cases.pts_for(frames, dvda_build.SAMPLE_RATE[spec["rate"]])
            rc, err, pcm = ref_decode(tmp, image, first, pts, split)
            titles[name] = dict(record(rc, err, pcm), spec=spec, first=first, pts=pts,
                                split=split)
            if not agrees(rc, err, pcm, image, first, pts):
                print("aob_port differs from the reference:", name, rc, repr(err), len(pcm))
                bad += 1
        for name, spec in sorted(dvda_cases.flip_specs().items()):
            image, _ = dvda_build.aob_image(spec)
            rate = dvda_build.SAMPLE_RATE[spec["rate"]]
            ptss = [dvda_cases.pts_for(FLIP_PTS_FRAMES, rate),
                    dvda_cases.pts_for(dvda_cases.frames_of(spec) - 2 * (
                        FLIP_MARGIN // (dvda_cases.frames_of(spec) and
                                        sum(spec["payloads"]) * 2 //
                                        dvda_cases.frames_of(spec))), rate)]
            bits = dvda_build.header_bits(spec)
            rows, aside, replay = [], {}, {}
            counts = {"flips": len(bits), "reference_died": 0, "reference_limits": 0,
                      "mlp": 0, "signals": {}}
            for bit in bits:
                img = dvda_build.flip(image, bit)
                row, why = [], None
                for pts in ptss:
                    rc, err, pcm = ref_decode(tmp, img, 0, pts)
                    row.append([rc, err, hashlib.md5(pcm).hexdigest()[:16], len(pcm)])
                    status = aob_port.decode(img)[0]["status"]
                    if rc == "timeout":
                        why = "reference: timeout"
                    elif rc != 0:
                        why = "reference: %s" % rc
                    elif status == aob_port.MLP:
                        why = "mlp"
                    elif aob_port.reference_answer(img, pts)[2] == aob_port.EOF:
                        # the flip changed the layout or a pad size so that the
                        # request passes the sectors: the reference replays its
                        # last packet, the port stops with the frames present
                        raw = aob_port.reference_answer(img, pts)[0]
                        if err or pcm[:len(raw)] != raw:
                            print("aob_port differs before a replay:", name, bit, pts)
                            bad += 1
                        replay[str(bit)] = "replay"
                    elif not agrees(rc, err, pcm, img, 0, pts):
                        print("aob_port differs on a flip:", name, bit, pts, rc, repr(err),
                              len(pcm))
                        bad += 1
                if why:
                    aside[str(bit)] = why
                    key = ("reference_limits" if "timeout" in why else
                           "mlp" if why == "mlp" else "reference_died")
                    counts[key] += 1
                    if key == "reference_died":
                        counts["signals"][why[11:]] = counts["signals"].get(why[11:], 0) + 1
                rows.append(row)
            counts["set_aside"] = len(aside)
            counts["replay"] = len(replay)
            if len(aside) * 50 > len(bits):
                print("more than 2 %% of the sweep set aside: %s %d of %d" %
                      (name, len(aside), len(bits)))
                bad += 1
            sweeps[name] = {"spec": spec, "pts": ptss, "bits": bits, "flips": rows,
                            "set_aside": aside, "replay": replay, "counts": counts}
    with open(OUT, "w") as f:
        json.dump(dvda_cases.pack_golden(titles, sweeps), f, separators=(",", ":"),
                  sort_keys=True)
        f.write("\n")
    print("%d title vectors, sweeps %s, %d disagreements" %
          (len(titles), json.dumps({k: v["counts"] for k, v in sweeps.items()}, sort_keys=True),
           bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
