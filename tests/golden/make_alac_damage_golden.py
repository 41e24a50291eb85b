#!/usr/bin/env python3
"""Generate tests/golden/alac_damage_<image>.json with the REFERENCE ALAC
decoder (oracle/_ref/alacdec: src/decoders/alac.c built standalone by
`make -C oracle ref`, where the reference tree is present).

ALAC carries no checksum, so a damaged stream is decoded, not refused.  For
each image of tests/alac_cases.py DAMAGE_IMAGES (rebuilt from a seeded
signal, never committed; its sha256 is recorded) this records alacdec's
outcome -- return code, length and the first 12 hex digits of the md5 of the
PCM bytes it wrote -- on

  * every single-bit flip of the mdat atom,
  * every truncation of the image,
  * every single-bit flip of the header (all before the mdat atom) whose
    outcome differs from the clean image's; the rest change nothing the
    decoder reads and are only counted.  The 3-channel image records no
    header flips.

alacdec runs under a time limit and an address-space limit.  Set aside, by
name, are the cases on which it dies (signal or time-out, recorded as such)
and the cases on which oracle/alac_port.c differs and met a residual block
no longer than its subframe's order: the reference's decode_subframe
(alac.c:1157-1173) then writes order + 1 samples from residuals it never
read (whatever its buffer held), so its result is not defined by the
stream.  oracle/alac_port.c is run over every case; the script exits
non-zero if it disagrees with the reference on one that is not set aside.

The record is packed: for the truncations and the header flips one table of
distinct outcomes per image and an index into it per case, for the mdat
flips (nearly all distinct) parallel arrays.
"""
import hashlib
import json
import os
import resource
import signal
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [TESTS, os.path.join(ROOT, "python-audio-tools_amd")]
import alac_cases  # noqa: E402
import oracle_port  # noqa: E402

TIME_LIMIT = 10
ADDRESS_SPACE = 1 << 33
MD5_DIGITS = 12
WORKERS = min(8, os.cpu_count() or 1)


def limits():
    resource.setrlimit(resource.RLIMIT_AS, (ADDRESS_SPACE, ADDRESS_SPACE))


def ref_decode(job):
    """-> [return code, or the signal's name, or "timeout"; bytes; md5]"""
    path, image = job
    with open(path, "wb") as f:
        f.write(image)
    try:
        p = subprocess.run([oracle_port.REF_ALACDEC, path], stdout=subprocess.PIPE,
                           stderr=subprocess.DEVNULL, timeout=TIME_LIMIT, preexec_fn=limits)
    except subprocess.TimeoutExpired:
        return ["timeout", 0, ""]
    if p.returncode < 0:
        return [signal.Signals(-p.returncode).name, 0, ""]
    return [p.returncode, len(p.stdout), hashlib.md5(p.stdout).hexdigest()[:MD5_DIGITS]]


def run_reference(images, tmp):
    jobs = [(os.path.join(tmp, "%d.m4a" % (i % (4 * WORKERS))), im) for i, im in enumerate(images)]
    # a file name is reused only 4 * WORKERS jobs later: map() keeps the order
    # and at most WORKERS run at once
    out = []
    with ThreadPoolExecutor(WORKERS) as ex:
        for k in range(0, len(jobs), WORKERS):
            out += list(ex.map(ref_decode, jobs[k:k + WORKERS]))
    return out


def pack(outs):
    """nearly every mdat flip has an outcome of its own: a character, a
    number and MD5_DIGITS digits per case instead of the table ("x": the
    reference died, how is in set_aside)"""
    assert all(o[0] in (0, 1) or isinstance(o[0], str) for o in outs)
    return {"rc": "".join("x" if isinstance(o[0], str) else str(o[0]) for o in outs),
            "bytes": [o[1] for o in outs],
            "md5": "".join(o[2].ljust(MD5_DIGITS, "-") for o in outs)}


def sweep(name, tmp):
    img, start, x = alac_cases.damage_image(name)
    p = alac_cases.DAMAGE_IMAGES[name]
    clean = ref_decode((os.path.join(tmp, "clean.m4a"), img))
    if clean[0] != 0 or clean[1] != len(oracle_port.pcm_bytes(x, p["bps"])) or \
            clean[2] != hashlib.md5(oracle_port.pcm_bytes(x, p["bps"])).hexdigest()[:MD5_DIGITS]:
        print("%s: the reference does not decode the clean image to its source" % name)
        return None, 1
    table, index = [], {}

    def intern(o):
        k = json.dumps(o)
        if k not in index:
            index[k] = len(table)
            table.append(o)
        return index[k]

    aside = {c: {} for c in alac_cases.DAMAGE_SET_ASIDE}
    bad = 0
    mismatch = 0

    def hold(key, image, o):
        """the port against the reference's outcome on one case"""
        nonlocal bad, mismatch
        before = oracle_port.alac_short_blocks()
        status, pcm, bps = alac_cases.port_outcome(image)
        short = oracle_port.alac_short_blocks() - before
        mismatch += status == 10
        if o[0] not in (0, 1):
            aside["reference_died"][key] = o[0]
        elif status == 10:
            pass  # the standalone has no such check; the Python path raises
        elif not alac_cases.matches_reference(status, pcm, bps, o):
            if short:
                aside["reference_short_block"][key] = "alacdec %d, %d bytes; port %d, %d samples" \
                    % (o[0], o[1], status, len(pcm))
            else:
                print("%s %s: reference %r, port status %d with %d samples"
                      % (name, key, o, status, len(pcm)))
                bad += 1

    rec = {"generator": "tests/golden/make_alac_damage_golden.py", "image": dict(p),
           "image_sha256": hashlib.sha256(img).hexdigest(), "image_bytes": len(img),
           "mdat_start": start, "clean": clean, "md5_digits": MD5_DIGITS}
    bits = list(range(8 * start, 8 * len(img)))
    images = [alac_cases.flip(img, b) for b in bits]
    outs = run_reference(images, tmp)
    mm0 = mismatch
    for b, im, o in zip(bits, images, outs):
        hold("f%d" % b, im, o)
    mdat_mismatch = mismatch - mm0
    bits_mdat = bits
    rec["mdat_flips"] = pack(outs)
    images = [img[:n] for n in range(len(img))]
    outs = run_reference(images, tmp)
    for n, (im, o) in enumerate(zip(images, outs)):
        hold("t%d" % n, im, o)
    rec["truncations"] = [intern(o) for o in outs]
    hb, ho, same = [], [], 0
    if name != "three16":
        bits = list(range(8 * start))
        images = [alac_cases.flip(img, b) for b in bits]
        outs = run_reference(images, tmp)
        for b, im, o in zip(bits, images, outs):
            if o == clean:
                same += 1
                continue
            hold("f%d" % b, im, o)
            hb.append(b)
            ho.append(intern(o))
    rec["header_flips"] = {"bits": hb, "outcomes": ho, "unchanged": same}
    rec["outcomes"] = table
    rec["set_aside"] = aside
    cases = len(bits_mdat) + len(rec["truncations"]) + len(hb)
    rec["counts"] = {"cases": cases, "mdat_flips": len(bits_mdat),
                     "truncations": len(rec["truncations"]), "header_flips": len(hb),
                     "header_flips_unchanged": same,
                     "channel_mismatch_mdat_flips": mdat_mismatch,
                     "channel_mismatch": mismatch,
                     "max_output_bytes": max([o[1] for o in table] +
                                             rec["mdat_flips"]["bytes"])}
    for c in alac_cases.DAMAGE_SET_ASIDE:
        rec["counts"][c] = len(aside[c])
    # the caps the tests assert again from these counts
    if 200 * len(aside["reference_died"]) > cases:
        print("%s: the reference dies on more than 0.5 %% of the cases" % name)
        bad += 1
    if 10 * mdat_mismatch > len(bits_mdat):
        print("%s: more than 10 %% of the mdat flips are channel mismatches" % name)
        bad += 1
    print(name, json.dumps(rec["counts"], sort_keys=True))
    print(name, "set aside:", json.dumps(aside, sort_keys=True), flush=True)
    return rec, bad


def main():
    if not os.path.exists(oracle_port.REF_ALACDEC):
        print("oracle/_ref/alacdec missing: run `make -C oracle ref` where the reference "
              "tree exists")
        return 1
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in (sys.argv[1:] or sorted(alac_cases.DAMAGE_IMAGES)):
            rec, b = sweep(name, tmp)
            bad += b
            if rec is None:
                continue
            with open(alac_cases.damage_golden(name), "w") as f:
                json.dump(rec, f, separators=(",", ":"), sort_keys=True)
                f.write("\n")
    print("%d disagreements" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
