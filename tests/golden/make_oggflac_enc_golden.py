#!/usr/bin/env python3
"""Generate tests/golden/oggflac_enc_vectors.json: the Ogg FLAC encoder's page
layout, accepted by the REFERENCE decoder.

There is no reference Ogg FLAC encoder to compare with (the reference pipes
PCM into the external `flac --ogg` program), so the contract is the layout of
DESIGN.md section 4k as tests/oggflac_mux_port.py restates it, and that the
reference's own decoder takes every image: this script builds
oracle/_ref/oggflacdec (make_oggflac_golden.build_reference), muxes every case
of tests/oggflac_enc_cases.py with the port and runs oggflacdec on it.  It
FAILS unless every case returns 0 and writes exactly the source PCM; no case is
set aside.  Recorded per case: sha256 and length of the image, its page
count, and the md5 of the PCM.  The seed of the "one frame of exactly 255 k
bytes" case is searched here and recorded.
"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [TESTS, HERE]
import make_oggflac_golden as ref  # noqa: E402
import oggflac_enc_cases as cases  # noqa: E402
import oggflac_mux_port as mp  # noqa: E402
import oracle_port  # noqa: E402
import signals  # noqa: E402


def find_mult255_seed(limit=20000):
    m = cases.MULT255
    opts = dict(oracle_port.PRESETS["8"], block_size=m["block"], padding_size=4096)
    for seed in range(limit):
        x = signals.make(m["kind"], m["frames"], m["ch"], m["bps"], seed=seed)
        flac, frames = oracle_port.encode(x, m["ch"], m["bps"], cases.RATE, **opts)
        assert len(frames) == 1
        _, body = oracle_port.split_flac(flac)
        if len(body) % 255 == 0:
            return seed
    raise SystemExit("no seed below %d gives a 255 k frame" % limit)


def main():
    if not ref.build_reference():
        raise SystemExit("the reference tree is not present: cannot build oggflacdec")
    seed = find_mult255_seed()
    out = {"mult255_seed": seed, "cases": {}}
    bad = []
    with tempfile.TemporaryDirectory() as tmp:
        for c in cases.all_cases(seed):
            d = c.port()
            want = oracle_port.pcm_bytes(c.pcm(), c.bps)
            rc, cls, pcm = ref.ref_decode(d["image"], tmp)
            if rc != 0 or pcm != want:
                bad.append((c.name, rc, cls, len(pcm), len(want)))
            out["cases"][c.name] = {
                "sha256": hashlib.sha256(d["image"]).hexdigest(), "bytes": len(d["image"]),
                "pages": d["pages"], "pcm_md5": hashlib.md5(want).hexdigest()}
    if bad:
        for b in bad:
            print("REFUSED by oggflacdec: %s rc=%s %s pcm %d/%d" % b)
        raise SystemExit(1)
    with open(cases.GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases accepted by oggflacdec, seed %d -> %s" % (len(out["cases"]), seed,
                                                              cases.GOLDEN))


if __name__ == "__main__":
    main()
