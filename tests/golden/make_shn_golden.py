#!/usr/bin/env python3
"""Generate tests/golden/shn_vectors.json with the REFERENCE Shorten encoder
and decoder.

The reference's src/encoders/shn.c and src/decoders/shn.c each carry a
-DSTANDALONE main; this script compiles them into oracle/_ref/shnenc and
oracle/_ref/shndec (which is outside git) with the flags of oracle/Makefile,
where the reference tree is present, and copies the reference's two .shn
fixtures to tests/golden/fixtures.

Encoder vectors: the inputs of tests/shn_cases.py -> sha256 and length of the
file shnenc wrote.  shnenc is always signed and little-endian, so the other
file types and explicit frame sizes are checked the other way round: shndec
must decode shn_port's file back to the source.

Decoder vectors: shnenc's files, the fixtures, the builder's streams, every
truncation and every single-bit flip of the fixtures -> shndec's return code
and the md5 and length of the PCM it wrote.  shndec runs under a time limit
and an address-space limit.  A flip on which it dies or runs into a limit, on
which its sample arithmetic overflows a C int (undefined there; shn_port
wraps at 32 bits) and the samples differ, or which only the limits of
include/atgpu.h refuse, is set aside and counted;
the script fails if more than 5 % of the flips are.

tests/shn_port.py is run over every vector; the script exits non-zero if it
disagrees with the reference anywhere.
"""
import hashlib
import json
import os
import resource
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [TESTS]
import shn_cases  # noqa: E402
import shn_port  # noqa: E402

REF = os.environ.get("SHN_REFERENCE", "/root/reference")
REF_BIN = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(HERE, "shn_vectors.json")
CFLAGS = ["-O2", "-ffp-contract=off", "-w", "-DSTANDALONE", "-DVERSION=2.22alpha1"]
COMMON = ["array.c", "pcm.c", "pcmconv.c", "bitstream.c", "huffman.c", "buffer.c", "func_io.c"]
TIME_LIMIT = 10
ADDRESS_SPACE = 1 << 30


def build_reference():
    src = os.path.join(REF, "src")
    if not os.path.isdir(src):
        return False
    os.makedirs(REF_BIN, exist_ok=True)
    for name, codec in (("shnenc", "encoders/shn.c"), ("shndec", "decoders/shn.c")):
        out = os.path.join(REF_BIN, name)
        if os.path.exists(out):
            continue
        subprocess.check_call(["gcc"] + CFLAGS + ["-I" + src, "-o", out] +
                              [os.path.join(src, c) for c in COMMON] +
                              [os.path.join(src, codec), "-lm"])
    return True


def ref_encode(samples, channels, bps, block, header, footer, tmp):
    path = os.path.join(tmp, "e.shn")
    cmd = [os.path.join(REF_BIN, "shnenc"), "-c", str(channels), "-r", "44100", "-b", str(bps),
           "-B", str(block)]
    for flag, data in (("-H", header), ("-F", footer)):
        if data:
            p = os.path.join(tmp, "verbatim" + flag)
            with open(p, "wb") as f:
                f.write(data)
            cmd += [flag, p]
    subprocess.run(cmd + [path], input=shn_cases.pcm_bytes(samples, bps),
                   stdout=subprocess.DEVNULL, check=True)
    with open(path, "rb") as f:
        return f.read()


def limits():
    resource.setrlimit(resource.RLIMIT_AS, (ADDRESS_SPACE, ADDRESS_SPACE))


def ref_decode(image, tmp):
    """-> (return code, or the negated signal, or "timeout"; PCM bytes)"""
    path = os.path.join(tmp, "d.shn")
    with open(path, "wb") as f:
        f.write(image)
    try:
        p = subprocess.run([os.path.join(REF_BIN, "shndec"), path], stdout=subprocess.PIPE,
                           stderr=subprocess.DEVNULL, timeout=TIME_LIMIT, preexec_fn=limits)
    except subprocess.TimeoutExpired:
        return "timeout", b""
    return p.returncode, p.stdout


def port_decode(image):
    """shn_port's answer in shndec's terms -> (status, return code, PCM bytes)"""
    status, pcm, info, _, _ = shn_port.decode(image)
    raw = shn_cases.pcm_bytes(pcm, info["bits_per_sample"]) if info else b""
    return status, 0 if status == shn_port.END_OF_STREAM else 1, raw


def record(rc, pcm):
    return {"returncode": rc, "md5": hashlib.md5(pcm).hexdigest(), "bytes": len(pcm)}


def bit_string(image):
    return bin(int.from_bytes(b"\x01" + image, "big"))[3:]


def prefix_bits(ftype, channels, block, header):
    w = shn_port.BitWriter()
    shn_port.write_prefix(w, ftype, channels, block)
    shn_port.write_verbatim(w, header)
    return w.bits


def main():
    if not build_reference():
        print("reference sources absent: nothing generated")
        return 1
    os.makedirs(os.path.join(HERE, "fixtures"), exist_ok=True)
    fixtures = {}
    for name in shn_cases.FIXTURES:
        shutil.copyfile(os.path.join(REF, "test", name), os.path.join(HERE, "fixtures", name))
        with open(os.path.join(HERE, "fixtures", name), "rb") as f:
            fixtures[name] = f.read()
    bad = 0
    enc, dec, bulk = {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        todo = []
        for name, ch, bps, block, x, header, footer in shn_cases.encoder_cases():
            img = ref_encode(x, ch, bps, block, header, footer, tmp)
            enc[name] = {"sha256": hashlib.sha256(img).hexdigest(), "bytes": len(img)}
            mine = shn_port.encode(x, ch, bps, block, False, True, header, footer)
            if mine != img:
                print("shn_port encode differs from the reference:", name)
                bad += 1
            todo.append(("enc:" + name, img))
        for name, ch, bps, block, x, header, footer, be, sgn, sizes in shn_cases.port_cases():
            img = shn_port.encode(x, ch, bps, block, be, sgn, header, footer, sizes)
            rc, pcm = ref_decode(img, tmp)
            if rc != 0 or pcm != shn_cases.pcm_bytes(x, bps):
                print("shndec does not decode shn_port's file to its source:", name)
                bad += 1
            # the audio commands do not depend on the endianness the type names
            if sizes is None:
                other = shn_port.encode(x, ch, bps, block, not be, sgn, header, footer)
                a, b = bit_string(img), bit_string(other)
                pa = prefix_bits(shn_port.file_type(bps, be, sgn), ch, block, header)
                pb = prefix_bits(shn_port.file_type(bps, not be, sgn), ch, block, header)
                n = min(len(a) - pa, len(b) - pb) - 40
                if a[pa:pa + n] != b[pb:pb + n]:
                    print("shn_port's audio commands depend on the file type:", name)
                    bad += 1
            todo.append(("port:" + name, img))
        todo += [(n, d) for n, d in fixtures.items()]
        todo += [("built:" + n, d) for n, d in sorted(shn_cases.builder_streams().items())]
        for name, img in todo:
            rc, pcm = ref_decode(img, tmp)
            dec[name] = record(rc, pcm)
            status, prc, raw = port_decode(img)
            if prc != rc or raw != pcm:
                print("shn_port decode differs from the reference:", name, rc, status)
                bad += 1
        for name, img in sorted(shn_cases.unsupported_streams().items()):
            status = shn_port.decode(img)[0]
            if status != shn_port.UNSUPPORTED:
                print("shn_port does not refuse:", name, status)
                bad += 1
        # every truncation and every single-bit flip of the fixtures
        counts = {"flips": 0, "reference_died": 0, "reference_limits": 0, "limits_only": 0,
                  "reference_overflow": 0, "signals": {}}
        for name, img in sorted(fixtures.items()):
            cuts = []
            for n in range(len(img)):
                rc, pcm = ref_decode(img[:n], tmp)
                cuts.append([rc, hashlib.md5(pcm).hexdigest()[:16], len(pcm)])
                status, prc, raw = port_decode(img[:n])
                if prc != rc or raw != pcm:
                    print("shn_port differs on a truncation:", name, n, rc, status)
                    bad += 1
            flips, aside = [], {}
            for bit in range(8 * len(img)):
                b = bytearray(img)
                b[bit >> 3] ^= 0x80 >> (bit & 7)
                rc, pcm = ref_decode(bytes(b), tmp)
                wraps = shn_port.WRAPS[0]
                status, prc, raw = port_decode(bytes(b))
                wraps = shn_port.WRAPS[0] - wraps
                counts["flips"] += 1
                flips.append([rc, hashlib.md5(pcm).hexdigest()[:16], len(pcm)])
                if rc == "timeout" or (isinstance(rc, int) and rc < 0) or rc not in (0, 1):
                    if rc == "timeout":
                        counts["reference_limits"] += 1
                    else:
                        counts["reference_died"] += 1
                        counts["signals"][str(rc)] = counts["signals"].get(str(rc), 0) + 1
                    aside[str(bit)] = "reference: %s" % rc
                elif status == shn_port.UNSUPPORTED:
                    counts["limits_only"] += 1
                    aside[str(bit)] = "limits"
                elif wraps and prc == rc and len(raw) == len(pcm) and raw != pcm:
                    # signed overflow: undefined in the reference's C
                    counts["reference_overflow"] += 1
                    aside[str(bit)] = "reference: signed overflow"
                elif prc != rc or raw != pcm:
                    print("shn_port differs on a flip:", name, bit, rc, status)
                    bad += 1
            bulk[name] = {"truncations": cuts, "flips": flips, "set_aside": aside}
        counts["max_flip_output_bytes"] = max(f[2] for v in bulk.values() for f in v["flips"])
    aside = counts["reference_died"] + counts["reference_limits"] + counts["limits_only"] + \
        counts["reference_overflow"]
    counts["set_aside"] = aside
    if aside * 20 > counts["flips"]:
        print("more than 5 %% of the flips set aside: %d of %d" % (aside, counts["flips"]))
        bad += 1
    with open(OUT, "w") as f:
        json.dump({"encoder": enc, "decoder": dec, "damaged": bulk, "counts": counts}, f,
                  separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%d encoder vectors, %d decoder vectors, %s, %d disagreements" %
          (len(enc), len(dec), json.dumps(counts, sort_keys=True), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
