#!/usr/bin/env python3
"""Generate tests/golden/mlp_vectors.json with the REFERENCE DVD-Audio title
decoder on MLP titles.

oracle/_ref/aobdec is the binary golden/make_dvda_golden.py builds (aob.c's
-DSTANDALONE main with mlp.c); it is built here the same way where it is
missing.  There is no MLP encoder, so the streams come from tests/mlp_build.py.

Vectors: the cases of tests/mlp_cases.py, and every single-bit flip of the
stream bytes of the first two access units and of all sector header bytes of
its two small images -> aobdec's return code (or the negated signal, or
"timeout"), its stderr without the frame count line, and the length and MD5
of the PCM it wrote; for a sweep one short digest of all that per distinct
answer (mlp_cases.outcome).  No stream file is kept, and of a spec only a
digest: the tests rebuild the images from the case list.  aobdec runs under
a time limit and an address-space limit.

Every vector is asked for more frames than the title holds when the title
fails, and for exactly its frames when it does not (past the end of the
sectors the reference replays its last packet, which is not reproduced).
A vector on which the reference dies or runs into a limit, or whose title
tests/mlp_port.py refuses under one of the limits include/atgpu_mlp.h states,
is set aside from the comparison with the reference and counted; the port's
own answer is recorded for it all the same, and the GPU is held to it.  The
script fails if more than 2 % of a sweep is set aside, and wherever the port
disagrees with the reference on a vector that is not.
"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [TESTS, HERE]
import dvda_build  # noqa: E402
import make_dvda_golden as G  # noqa: E402
import mlp_cases  # noqa: E402
import mlp_port  # noqa: E402

OUT = os.path.join(HERE, "mlp_vectors.json")


def port_record(res, x):
    """mlp_cases.PORT_KEYS' values, then whether a sample leaves the title's
    bits (the ABI wraps, the reference clips) and the samples' MD5"""
    return [res[k] for k in mlp_cases.PORT_KEYS] + [
        bool(len(x) and (res["full"] != x).any()),
        hashlib.md5(x.astype("<i4").tobytes()).hexdigest()[:16]]


def one(tmp, img, first, split):
    """-> (record, why set aside or None, disagreement or None)"""
    res, x, _ = mlp_port.decode(img, first)
    pts = mlp_cases.ask_pts(res)
    want = mlp_port.answer_from(res, x, pts)
    rc, err, pcm = G.ref_decode(tmp, img, first, pts, split)
    # the reference's bit reader complains about the marks an error return leaves
    err = "".join(l for l in err.splitlines(True) if not l.startswith("*** Warning"))
    rec = {"ref": [rc, err, hashlib.md5(pcm).hexdigest()[:16], len(pcm)],
           "port": port_record(res, x)}
    flag = "c" if rec["port"][-2] else "n" if res["status"] == mlp_port.NOT_MLP else "p"
    if rc != 0 or want is None:
        flag = "a"
    rec["outcome"] = mlp_cases.outcome(res, x, flag, (pcm, err))
    if rc == "timeout":
        return rec, "reference: timeout", None
    if rc != 0:
        return rec, "reference: %s" % rc, None
    if want is None:
        return rec, "limit: status %d" % res["status"], None
    if (pcm, err) != want:
        return rec, None, "port %d bytes %r, reference %d bytes %r" % (
            len(want[0]), want[1], len(pcm), err)
    return rec, None, None


def main():
    if not G.build_reference():
        print("reference sources absent: nothing generated")
        return 1
    bad = 0
    titles, sweeps = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for s in mlp_cases.title_cases():
            img, first = mlp_cases.image_of(s)
            rec, aside, wrong = one(tmp, img, first, s.get("aobs"))
            rec["spec"] = mlp_cases.spec_digest(s)
            del rec["outcome"]
            if aside:
                rec["set_aside"] = aside
            if wrong:
                print("mlp_port differs from the reference:", s["name"], wrong)
                bad += 1
            titles[s["name"]] = rec
        for name, s in sorted(mlp_cases.flip_specs().items()):
            img, _ = mlp_cases.image_of(s)
            bits = mlp_cases.flip_bits(s)
            outcomes, rows, aside = [], [], {}
            changed = 0
            clean = one(tmp, img, 0, None)[0]
            for bit in bits:
                rec, why, wrong = one(tmp, dvda_build.flip(img, bit), 0, None)
                if wrong:
                    print("mlp_port differs on a flip:", name, bit, wrong)
                    bad += 1
                if why:
                    aside[str(bit)] = why
                changed += rec["ref"][2] != clean["ref"][2]
                key = rec["outcome"]
                if key not in outcomes:
                    outcomes.append(key)
                i = outcomes.index(key)
                if rows and rows[-1][0] == i:
                    rows[-1][1] += 1
                else:
                    rows.append([i, 1])
            counts = {"flips": len(bits), "set_aside": len(aside), "changed_pcm": changed}
            for why in aside.values():
                counts[why.split(":")[0]] = counts.get(why.split(":")[0], 0) + 1
            if len(aside) * 50 > len(bits):
                print("more than 2 %% of the sweep set aside: %s %d of %d" %
                      (name, len(aside), len(bits)))
                bad += 1
            rows = [i if n == 1 else [i, n] for i, n in rows]
            sweeps[name] = {"spec": mlp_cases.spec_digest(s), "n_bits": len(bits),
                            "outcomes": outcomes, "flips": rows, "counts": counts}
    with open(OUT, "w") as f:
        json.dump({"titles": titles, "sweeps": sweeps}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%d title vectors (%d set aside), sweeps %s, %d disagreements" % (
        len(titles), sum("set_aside" in t for t in titles.values()),
        json.dumps({k: v["counts"] for k, v in sweeps.items()}, sort_keys=True), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
