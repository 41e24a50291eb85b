#!/usr/bin/env python3
"""Generate tests/golden/wavpack_vectors.json and wavpack_images.bin with the
REFERENCE WavPack encoder and decoder.

The reference's src/encoders/wavpack.c and src/decoders/wavpack.c each carry
a -DSTANDALONE main; this script compiles them into oracle/_ref/wvenc and
oracle/_ref/wvdec (outside git) with the flags of oracle/Makefile, where the
reference tree is present.

Good vectors: the inputs of tests/wavpack_cases.py encoded by wvenc, three
images patched from them (one-bits / duplicate-bits) and the reference's two
.wv fixtures (copied to tests/golden/fixtures) -> wvdec's return code, its
message, and the md5 and length of the PCM it wrote.  The images are stored in
wavpack_images.bin, since nothing else can make them where the tests run.

Damage vectors: single-bit flips and truncations of two of the images, each
stored as 8 * byte + bit or as a length, grouped by the reference's outcome:
its status and an index into the table of distinct (PCM length, md5) it wrote.  A case is
left out only when wvdec ends abnormally (signal, timeout) or when its
outcome rests on behaviour C leaves undefined, which tests/wavpack_port.py
cannot reproduce; every such case is listed with its reason, and the script
fails if they exceed 2 % of the damage cases.  Cases that the GPU decoder's
host layout checks refuse (status 17, INCONSISTENT_BLOCK, where the reference
trusts the headers) are the flagged ones: there the PCM before the refused set must be a
prefix of what wvdec wrote.

tests/wavpack_port.py is run over every vector; the script exits non-zero if
it disagrees with the reference anywhere.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [TESTS]
import wavpack_cases as cases  # noqa: E402
import wavpack_port as port  # noqa: E402

REF = os.environ.get("WAVPACK_REFERENCE", "/root/reference")
REF_BIN = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(HERE, "wavpack_vectors.json")
IMAGES = os.path.join(HERE, "wavpack_images.bin")
CFLAGS = ["-O2", "-ffp-contract=off", "-w", "-DSTANDALONE", "-DVERSION=2.22alpha1"]
COMMON = ["array.c", "pcm.c", "pcmconv.c", "bitstream.c", "huffman.c", "buffer.c", "func_io.c",
          "common/md5.c"]
INIT_MESSAGE = "Error initializing WavPack decoder"


def build_reference():
    src = os.path.join(REF, "src")
    if not os.path.isdir(src):
        return False
    os.makedirs(REF_BIN, exist_ok=True)
    for name, codec in (("wvenc", "encoders/wavpack.c"), ("wvdec", "decoders/wavpack.c")):
        out = os.path.join(REF_BIN, name)
        if os.path.exists(out):
            continue
        subprocess.check_call(["gcc"] + CFLAGS + ["-I" + src, "-o", out] +
                              [os.path.join(src, c) for c in COMMON] +
                              [os.path.join(src, codec), "-lm"])
    return True


def ref_encode(opts, samples, bps, tmp):
    path = os.path.join(tmp, "e.wv")
    subprocess.run([os.path.join(REF_BIN, "wvenc")] + opts + [path],
                   input=cases.pcm_bytes(samples, bps), stdout=subprocess.DEVNULL, check=True)
    with open(path, "rb") as f:
        return f.read()


def ref_decode(image, tmp):
    """-> (return code or None when wvdec ended abnormally, message, PCM)"""
    path = os.path.join(tmp, "d.wv")
    with open(path, "wb") as f:
        f.write(image)
    try:
        p = subprocess.run([os.path.join(REF_BIN, "wvdec"), path], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=20)
    except subprocess.TimeoutExpired:
        return None, "timeout", b""
    if p.returncode < 0:
        return None, "signal %d" % -p.returncode, p.stdout
    msg = p.stderr.decode("latin-1").strip()
    for lead in ("*** Error: ", "*** "):
        if msg.startswith(lead):
            msg = msg[len(lead):]
            break
    return p.returncode, msg, p.stdout


def port_outcome(image):
    """-> (status, message as wvdec would print it, PCM bytes)"""
    st, info, pcm, _ = port.decode(image)
    if info is None:
        return st, INIT_MESSAGE, b""
    return st, port.MESSAGES.get(st, ""), port.pcm_bytes(pcm, info["bits_per_sample"])


def patch_int32_info(image, values):
    """rewrite every int32-info sub-block and drop the trailing MD5 block"""
    img = bytearray(image)
    st, info, sets, end = port.read_info(image)
    assert st == 0 and end == 0
    for blocks in sets:
        for h in blocks:
            off, size = h["data"]
            pos = off
            while pos < off + size:
                b = img[pos]
                hdr = 4 if b >> 7 else 2
                words = img[pos + 1] if hdr == 2 else int.from_bytes(img[pos + 1:pos + 4],
                                                                      "little")
                if (b & 63) == 9:
                    img[pos + hdr:pos + hdr + 4] = bytes(values)
                pos += hdr + 2 * words
    return bytes(img[:info["end_offset"]])


def compare(name, image, tmp, record):
    """run reference and port over one image -> 'ok', 'flagged', or a reason
    the case is left out; a disagreement returns None"""
    rc, msg, pcm = ref_decode(image, tmp)
    st, pmsg, ppcm = port_outcome(image)
    record.update({"returncode": rc, "message": msg, "md5": hashlib.md5(pcm).hexdigest(),
                   "bytes": len(pcm), "status": st})
    if st == port.INCONSISTENT_BLOCK:
        # the reference trusts the headers; whatever it does, the sets before
        # the refused one are what both must have written
        if rc is not None and not pcm.startswith(ppcm):
            return None
        record.update({"md5": hashlib.md5(ppcm).hexdigest(), "bytes": len(ppcm)})
        return "flagged"
    if rc is None:
        return "wvdec ended abnormally: " + msg
    if (rc != 0) == (st != 0) and (rc == 0 or msg == pmsg) and pcm == ppcm:
        return "ok"
    return None


def main():
    if not build_reference():
        print("reference sources absent: nothing generated")
        return 1
    os.makedirs(os.path.join(HERE, "fixtures"), exist_ok=True)
    for name in cases.FIXTURES:
        shutil.copyfile(os.path.join(REF, "test", name), os.path.join(HERE, "fixtures", name))
    bad = 0
    images, good, blob = {}, {}, bytearray()
    damage = {"flips": {}, "cuts": {}, "left_out": [], "pcm": []}
    keys = {}

    def pcm_key(rec):
        k = (rec["bytes"], rec["md5"])
        if k not in keys:
            keys[k] = len(damage["pcm"])
            damage["pcm"].append(list(k))
        return keys[k]
    with tempfile.TemporaryDirectory() as tmp:
        for name, opts, ch, bps, rate, x in cases.cases():
            images[name] = (ref_encode(opts, x, bps, tmp), cases.pcm_bytes(x, bps))
        for name, base, values in cases.PATCHED:
            images[name] = (patch_int32_info(images[base][0], values), None)
        for name in cases.FIXTURES:
            with open(os.path.join(HERE, "fixtures", name), "rb") as f:
                images[name] = (f.read(), None)
        for name, (img, source) in images.items():
            rec = {}
            how = compare(name, img, tmp, rec)
            if how != "ok" or (source is not None and
                               hashlib.md5(source).hexdigest() != rec["md5"]):
                print("wavpack_port differs from the reference (or the source):", name, rec)
                bad += 1
            rec["source"] = source is not None
            if name not in cases.FIXTURES:
                rec["offset"] = len(blob)
                blob += img
            rec["image_bytes"] = len(img)
            del rec["message"]
            good[name] = rec
        total = 0
        todo = [(cases.DAMAGE_STEREO, None), (cases.DAMAGE_3CH, "first block")]
        for name, limit in todo:
            img = images[name][0]
            if limit:
                limit = 8 + port.parse_header(img, 0)[1]["block_size"]
            rows = {}
            for byte, bit in cases.flip_cases(len(img), limit):
                d = bytearray(img)
                d[byte] ^= 1 << bit
                rec = {}
                how = compare(name, bytes(d), tmp, rec)
                total += 1
                if how is None:
                    # the port and the reference disagree: undefined behaviour
                    # in the reference is the only accepted reason, and it is
                    # looked at by hand before it is listed below
                    print("damage disagreement:", name, byte, bit, rec)
                    bad += 1
                elif how in ("ok", "flagged"):
                    rows.setdefault("%d,%d" % (rec["status"], pcm_key(rec)),
                                    []).append(8 * byte + bit)
                else:
                    damage["left_out"].append({"image": name, "byte": byte, "bit": bit,
                                               "reason": how})
            damage["flips"][name] = rows
        img = images[cases.DAMAGE_STEREO][0]
        rows = {}
        for n in range(0, len(img), 7):
            rec = {}
            how = compare("cut", img[:n], tmp, rec)
            total += 1
            if how in ("ok", "flagged"):
                rows.setdefault("%d,%d" % (rec["status"], pcm_key(rec)), []).append(n)
            else:
                print("cut disagreement:", n, rec, how)
                bad += 1
        damage["cuts"][cases.DAMAGE_STEREO] = rows
    damage["cases"] = total
    damage["left_out_count"] = len(damage["left_out"])
    if len(damage["left_out"]) * 50 > total:
        print("more than 2 %% of the damage cases left out: %d of %d" %
              (len(damage["left_out"]), total))
        bad += 1
    with open(IMAGES, "wb") as f:
        f.write(blob)
    with open(OUT, "w") as f:
        json.dump({"images": good, "damage": damage}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    flagged = sum(len(v) for kind in ("flips", "cuts") for groups in damage[kind].values()
                  for k, v in groups.items() if k.startswith("%d," % port.INCONSISTENT_BLOCK))
    print("%d images (%d bytes), %d damage cases (%d flagged, %d left out), %d disagreements" %
          (len(good), len(blob), total, flagged, len(damage["left_out"]), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
