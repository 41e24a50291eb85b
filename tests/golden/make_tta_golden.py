#!/usr/bin/env python3
"""Generate tests/golden/tta_vectors.json with the REFERENCE True Audio
encoder and decoder.

The reference's src/encoders/tta.c and src/decoders/tta.c each carry a
-DSTANDALONE main; this script compiles them into oracle/_ref/ttaenc and
oracle/_ref/ttadec (which is outside git) with the flags of oracle/Makefile,
where the reference tree is present.

Encoder vectors: the inputs of tests/tta_cases.py -> sha256 and length of the
whole file ttaenc wrote, and its frame sizes (the seektable).  Decoder
vectors: some of those files and the reference's two .tta fixtures (copied
to tests/golden/fixtures; the ID3v2 prefix of the second is stripped before
ttadec sees it) -> ttadec's return code and the md5 and length of the PCM it
wrote.

tests/tta_port.py is run over every vector; the script exits non-zero if it
disagrees with the reference anywhere.
"""
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [TESTS]
import tta_cases  # noqa: E402
import tta_port  # noqa: E402

REF = os.environ.get("TTA_REFERENCE", "/root/reference")
REF_BIN = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(HERE, "tta_vectors.json")
CFLAGS = ["-O2", "-ffp-contract=off", "-w", "-DSTANDALONE", "-DVERSION=2.22alpha1"]
COMMON = ["array.c", "pcm.c", "pcmconv.c", "bitstream.c", "huffman.c", "buffer.c", "func_io.c"]


def build_reference():
    src = os.path.join(REF, "src")
    if not os.path.isdir(src):
        return False
    os.makedirs(REF_BIN, exist_ok=True)
    for name, codec in (("ttaenc", "encoders/tta.c"), ("ttadec", "decoders/tta.c")):
        out = os.path.join(REF_BIN, name)
        if os.path.exists(out):
            continue
        subprocess.check_call(["gcc"] + CFLAGS + ["-I" + src, "-o", out] +
                              [os.path.join(src, c) for c in COMMON] +
                              [os.path.join(src, codec), "-lm"])
    return True


def ref_encode(samples, channels, bps, rate, tmp):
    path = os.path.join(tmp, "e.tta")
    subprocess.run([os.path.join(REF_BIN, "ttaenc"), "-c", str(channels), "-r", str(rate),
                    "-b", str(bps), "-T", str(len(samples) // channels), path],
                   input=tta_cases.pcm_bytes(samples, bps), stdout=subprocess.DEVNULL,
                   check=True)
    with open(path, "rb") as f:
        return f.read()


def ref_decode(image, tmp):
    path = os.path.join(tmp, "d.tta")
    with open(path, "wb") as f:
        f.write(image)
    p = subprocess.run([os.path.join(REF_BIN, "ttadec"), path], stdout=subprocess.PIPE,
                       stderr=subprocess.DEVNULL)
    return p.returncode, p.stdout


def main():
    if not build_reference():
        print("reference sources absent: nothing generated")
        return 1
    os.makedirs(os.path.join(HERE, "fixtures"), exist_ok=True)
    for name in tta_cases.FIXTURES:
        shutil.copyfile(os.path.join(REF, "test", name), os.path.join(HERE, "fixtures", name))
    cases = tta_cases.encoder_cases()
    bad = 0
    enc, dec, images = {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, ch, bps, rate, x in cases:
            img = ref_encode(x, ch, bps, rate, tmp)
            nf = (len(x) // ch + tta_port.block_size(rate) - 1) // tta_port.block_size(rate)
            sizes = list(struct.unpack("<%dI" % nf, img[22:22 + 4 * nf]))
            enc[name] = {"sha256": hashlib.sha256(img).hexdigest(), "bytes": len(img),
                         "frame_sizes": sizes}
            images[name] = img
        todo = [(n, images[n], None) for n in tta_cases.DECODER_CASES]
        for name in tta_cases.FIXTURES:
            with open(os.path.join(HERE, "fixtures", name), "rb") as f:
                data = f.read()
            todo.append((name, data[tta_port.skip_id3v2(data):], None))
        for name, img, _ in todo:
            rc, pcm = ref_decode(img, tmp)
            dec[name] = {"returncode": rc, "md5": hashlib.md5(pcm).hexdigest(),
                         "bytes": len(pcm)}
    # tta_port against the record; the long 44.1 kHz chains in a call of
    # their own so that the others are not padded to their length
    for group in ([c for c in cases if c[3] == tta_cases.RATE],
                  [c for c in cases if c[3] != tta_cases.RATE]):
        got = tta_port.encode_many([(x, ch, bps, rate) for _, ch, bps, rate, x in group])
        for (name, ch, bps, rate, x), (img, sizes) in zip(group, got):
            if hashlib.sha256(img).hexdigest() != enc[name]["sha256"] or \
                    sizes != enc[name]["frame_sizes"]:
                print("tta_port encode differs from the reference:", name)
                bad += 1
    names = [t[0] for t in todo]
    for name, res in zip(names, tta_port.decode_many([t[1] for t in todo])):
        status, _, _, pcm, info = res
        raw = tta_cases.pcm_bytes(pcm, info["bits_per_sample"]) if status == 0 else b""
        if (status != 0) != (dec[name]["returncode"] != 0) or \
                (status == 0 and hashlib.md5(raw).hexdigest() != dec[name]["md5"]):
            print("tta_port decode differs from the reference:", name)
            bad += 1
    with open(OUT, "w") as f:
        json.dump({"encoder": enc, "decoder": dec}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d encoder vectors, %d decoder vectors, %d disagreements" % (len(enc), len(dec), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
