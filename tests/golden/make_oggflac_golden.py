#!/usr/bin/env python3
"""Generate tests/golden/oggflac_vectors.json with the REFERENCE Ogg FLAC
decoder.

The reference's src/decoders/oggflac.c carries a -DSTANDALONE main; this
script compiles it into oracle/_ref/oggflacdec (which is outside git) with the
flags of oracle/Makefile -- src/decoders/flac.c beside it without -DEXECUTABLE,
so that it contributes no main -- where the reference tree is present.

Every case of tests/oggflac_cases.py goes through oggflacdec: the image's
sha256, the return code, a message class (what it printed), and the byte count
and md5 of the PCM it wrote.  The sweeps (every single-bit flip and truncation
of a small image, every single-bit flip of its packets under valid page
checksums, 4,000 flips of one tone8.flac packet) are stored under the sha256 of
the undamaged image as their distinct rows and one index per case.

A case on which oggflacdec dies of a signal -- a frame whose subframes end
within the last two bytes of its packet makes it read the CRC-16 outside its
error handler and abort -- is set aside by reason; tests/oggflac_port.py gives
FD_EOF there.  The script fails if more than 5 % of a sweep is set aside, or
if the port disagrees with the reference on any other case.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [TESTS]
import oggflac_cases as cases  # noqa: E402
import oggflac_port as op  # noqa: E402
import oracle_port  # noqa: E402

REF = os.environ.get("OGGFLAC_REFERENCE", "/root/reference")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "oggflacdec")
OUT = os.path.join(HERE, "oggflac_vectors.json")
CFLAGS = ["-O2", "-ffp-contract=off", "-w", "-DSTANDALONE", "-DVERSION=2.22alpha1"]
SOURCES = ["decoders/oggflac.c", "decoders/flac.c", "ogg.c", "ogg_crc.c", "array.c", "pcm.c",
           "pcmconv.c", "bitstream.c", "huffman.c", "buffer.c", "func_io.c", "common/md5.c",
           "common/flac_crc.c"]
TIME_LIMIT = 10


def build_reference():
    src = os.path.join(REF, "src")
    if not os.path.isdir(src):
        return os.path.exists(REF_BIN)
    os.makedirs(os.path.dirname(REF_BIN), exist_ok=True)
    if not os.path.exists(REF_BIN):
        subprocess.check_call(["gcc"] + CFLAGS + ["-I" + src, "-o", REF_BIN] +
                              [os.path.join(src, c) for c in SOURCES] + ["-lm"])
    return True


def classify(rc, err):
    """oggflacdec's words -> "", "header", "ogg:<n>", "flac:<n>", "signal:<n>" """
    if rc == "timeout":
        return "timeout"
    if rc < 0:
        return "signal:%d" % rc
    if rc == 0:
        return ""
    text = err.decode("latin-1").strip()
    if not text:
        return "header"
    if "I/O Error reading FLAC frame" in text:
        return "flac:15"
    if "MD5 mismatch" in text:
        return "flac:16"
    text = text.split("Error: ", 1)[-1].strip()
    for n, m in op.OGG_MESSAGES.items():
        if text == m:
            return "ogg:%d" % n
    for n, m in oracle_port.FD_MESSAGES.items():
        if text == m:
            return "flac:%d" % n
    return "other:" + text


def ref_decode(image, tmp):
    path = os.path.join(tmp, "d.oga")
    with open(path, "wb") as f:
        f.write(image)
    try:
        p = subprocess.run([REF_BIN, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=TIME_LIMIT)
    except subprocess.TimeoutExpired:
        return "timeout", "timeout", b""
    return p.returncode, classify(p.returncode, p.stderr), p.stdout


def row(rc, cls, pcm):
    return [rc, cls, len(pcm), hashlib.md5(pcm).hexdigest()[:16]]


def compact(rows):
    """a sweep has few distinct outcomes: the distinct rows in order of first
    appearance, and each case's index into them (oggflac_cases.load_golden
    expands them again)"""
    unique, index = [], []
    for r in rows:
        if r not in unique:
            unique.append(r)
        index.append(unique.index(r))
    return {"unique": unique, "index": index}


def main():
    if not build_reference():
        print("reference sources absent: nothing generated")
        return 1
    bad = 0
    single, sweeps, counts = {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, img in sorted(cases.single_cases().items()):
            rc, cls, pcm = ref_decode(img, tmp)
            rec = {"sha256": hashlib.sha256(img).hexdigest(), "returncode": rc, "class": cls,
                   "bytes": len(pcm), "md5": hashlib.md5(pcm).hexdigest()}
            d = op.decode(img)
            if cls.startswith("signal") or cls == "timeout":
                rec["set_aside"] = "reference: " + cls
                if d["status"] != op.FD_EOF:
                    print("set-aside case is not the port's FD_EOF:", name, cls)
                    bad += 1
            elif (op.returncode(d), op.golden_class(d), d["pcm"]) != (rc, cls, pcm):
                print("oggflac_port differs from the reference:", name, rc, cls,
                      op.returncode(d), op.golden_class(d), len(pcm), len(d["pcm"]))
                bad += 1
            single[name] = rec
        for sname, make in sorted(cases.SWEEPS.items()):
            rows, aside, classes = [], {}, {}
            images = make()
            for k, img in enumerate(images):
                rc, cls, pcm = ref_decode(img, tmp)
                rows.append(row(rc, cls, pcm))
                classes[cls] = classes.get(cls, 0) + 1
                d = op.decode(img)
                if cls.startswith("signal") or cls == "timeout":
                    aside[str(k)] = "reference: " + cls
                    if d["status"] != op.FD_EOF:
                        print("set-aside case is not the port's FD_EOF:", sname, k, cls)
                        bad += 1
                elif (op.returncode(d), op.golden_class(d), d["pcm"]) != (rc, cls, pcm):
                    print("oggflac_port differs from the reference:", sname, k, rc, cls,
                          op.returncode(d), op.golden_class(d))
                    bad += 1
            if len(aside) * 20 > len(images):
                print("more than 5 %% of %s set aside: %d of %d" % (sname, len(aside), len(images)))
                bad += 1
            sweeps[sname] = dict(compact(rows), set_aside=aside)
            counts[sname] = {"cases": len(images), "set_aside": len(aside), "classes": classes}
    base = {"damage_base": hashlib.sha256(cases.damage_base()[1]).hexdigest(),
            "damage_base_bytes": len(cases.damage_base()[1]),
            "tone8_base": hashlib.sha256(op.mux(list(cases.tone8_base()[0]))).hexdigest()}
    with open(OUT, "w") as f:
        json.dump({"single": single, "sweeps": sweeps, "counts": counts, "bases": base}, f,
                  separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%d single cases, %s, %d disagreements" % (len(single), json.dumps(counts, sort_keys=True),
                                                     bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
