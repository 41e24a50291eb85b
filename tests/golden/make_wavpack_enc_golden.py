#!/usr/bin/env python3
"""Generate tests/golden/wavpack_enc_vectors.json with the REFERENCE WavPack
encoder, and check tests/wavpack_enc_port.py against it.

oracle/_ref/wvenc is built exactly as make_wavpack_golden.py builds it.  The
inputs of tests/wavpack_enc_cases.py are encoded by it and each image's length
and MD5 recorded: no images, the port regenerates one where a diff is wanted.

The port is then run over the 98 cases of tests/wavpack_cases.py (whose
committed images wvenc is required to reproduce here) and the new ones; every
new image is decoded with wavpack_port.decode and must give the source PCM
back (an 8-bit image with the MD5 mismatch the reference's own decoder
reports on it).  The script exits non-zero on any difference; no case is
left out.
"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [TESTS, HERE]
import wavpack_cases  # noqa: E402
import wavpack_enc_cases  # noqa: E402
import wavpack_enc_port as enc  # noqa: E402
import wavpack_port as dec  # noqa: E402
from make_wavpack_golden import build_reference, ref_encode  # noqa: E402

OUT = os.path.join(HERE, "wavpack_enc_vectors.json")


def port_encode(opts, x):
    kw = enc.parse_options(opts)
    return enc.encode(x, kw["channels"], kw["mask"], kw["bps"], kw["rate"], kw["block_size"],
                      kw["passes"], kw["joint"], kw["false"], kw["wasted"])


def main():
    if not build_reference():
        print("reference sources absent: nothing generated")
        return 1
    bad = 0
    _, committed = wavpack_cases.load_vectors()
    vectors = {}
    old, new = wavpack_cases.cases(), wavpack_enc_cases.cases()
    with tempfile.TemporaryDirectory() as tmp:
        for name, opts, ch, bps, rate, x in old:
            ref = ref_encode(opts, x, bps, tmp)
            if ref != committed[name]:
                print("wvenc no longer reproduces the committed image:", name)
                bad += 1
            if port_encode(opts, x) != ref:
                print("wavpack_enc_port differs from the reference:", name)
                bad += 1
        for name, opts, ch, bps, rate, x in new:
            ref = ref_encode(opts, x, bps, tmp)
            vectors[name] = {"bytes": len(ref), "md5": hashlib.md5(ref).hexdigest()}
            if port_encode(opts, x) != ref:
                print("wavpack_enc_port differs from the reference:", name)
                bad += 1
            st, info, pcm, _ = dec.decode(ref)
            # the reference encoder hashes 8-bit samples unsigned and its
            # decoder signed: its own 8-bit files end in MD5_MISMATCH with
            # every sample right (so do the 8-bit images of wavpack_vectors)
            want = dec.MD5_MISMATCH if bps == 8 else dec.OK
            if st != want or pcm != [int(v) for v in x]:
                print("the reference image does not decode to its source:", name, st)
                bad += 1
    if len(vectors) != len(new):
        print("duplicate case names")
        bad += 1
    with open(OUT, "w") as f:
        json.dump({"images": vectors}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d + %d cases, %d left out, %d differences" % (len(old), len(new), 0, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
