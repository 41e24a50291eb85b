#!/usr/bin/env python3
"""Is a kernel file's device code the same in two trees?  No GPU needed.

    tools/isa_diff.py PARENT_TREE PRODUCT_TREE pcm_chain.hip pcm_tensor.hip ...

Each file of csrc/ is compiled device-only to gfx950 assembly in both trees
with the Makefile's flags.  Per kernel, in the file's order, the instruction
streams are compared line by line after dropping comments, directives and
labels; a reference to a label becomes the label's number within the kernel
and a mangled name becomes SYM, since both change when a struct or a helper
moves.  The register counts, the LDS and the scratch size come from the code
object's metadata.  The table goes to stdout; the exit status is 1 when a
kernel differs.
"""
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
         "--cuda-device-only", "-S"]
CSRC = os.path.join("python-audio-tools_amd", "csrc")
META = {"vgpr": ".vgpr_count", "sgpr": ".sgpr_count", "lds": ".group_segment_fixed_size",
        "scratch": ".private_segment_fixed_size"}


def assembly(tree, name, tmp):
    out = os.path.join(tmp, "%s.%d.s" % (name, len(os.listdir(tmp))))
    subprocess.run([HIPCC] + FLAGS + ["-o", out, os.path.join(tree, CSRC, name)], check=True)
    with open(out) as f:
        return f.read().splitlines()


def demangle(names):
    try:
        p = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True)
        return p.stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return names


def kernels(lines):
    """[(mangled name, metadata dict, [instruction lines])] in metadata order"""
    meta, cur = [], None
    for ln in lines:
        if re.match(r"^  - \.", ln):
            cur = {}
            meta.append(cur)
        m = re.match(r"^  (?:- |  )(\.\w+):\s*(\S+)\s*$", ln)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    meta = [k for k in meta if ".vgpr_count" in k]
    out = []
    for k in meta:
        name = k[".name"]
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        body, labels = [], {}
        for ln in lines[start + 1:]:
            ln = ln.split(";")[0].strip()
            if ln.startswith(".Lfunc_end"):
                break
            if ln.endswith(":"):
                labels[ln[:-1]] = len(labels)
            elif ln and not ln.startswith("."):
                body.append(ln)
        body = [re.sub(r"\.LBB\d+_\d+", lambda m: "L%d" % labels.get(m.group(0), -1), ln)
                for ln in body]
        body = [re.sub(r"\b_Z\w+", "SYM", ln) for ln in body]
        out.append((name, {key: k.get(field, "?") for key, field in META.items()}, body))
    return out


def main(argv):
    if len(argv) < 4:
        sys.exit(__doc__)
    parent, product, files = argv[1], argv[2], argv[3:]
    differ = 0
    print("kernel | instructions vgpr sgpr lds scratch: parent -> product | identical")
    with tempfile.TemporaryDirectory() as tmp:
        for name in files:
            a = kernels(assembly(parent, name, tmp))
            b = kernels(assembly(product, name, tmp))
            print("%s: %d kernels, %d -> %d instructions" %
                  (name, len(b), sum(len(k[2]) for k in a), sum(len(k[2]) for k in b)))
            if len(a) != len(b):
                print("  kernel count differs: %d -> %d" % (len(a), len(b)))
                differ += 1
            shown = demangle([k[0] for k in b])
            for (_, ma, ia), (_, mb, ib), title in zip(a, b, shown):
                same = ia == ib and ma == mb
                differ += not same
                print("  %s | %d %s %s %s %s -> %d %s %s %s %s | %s" %
                      (title, len(ia), ma["vgpr"], ma["sgpr"], ma["lds"], ma["scratch"],
                       len(ib), mb["vgpr"], mb["sgpr"], mb["lds"], mb["scratch"],
                       "yes" if same else "NO"))
    print("kernels that differ: %d" % differ)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
