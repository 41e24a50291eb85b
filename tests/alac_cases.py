"""ALAC parity cases shared by the CPU oracle tests and the GPU tests: the
vectors of tests/golden/alac_vectors.json (recorded with the reference ALAC
encoder/decoder by tests/golden/make_alac_golden.py) and the inputs they
are defined on."""
import json
import os

import signals

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "alac_vectors.json")
FIX = os.path.join(HERE, "golden", "fixtures")
CREATE_DATE, VERSION = 0x7A11C0DE, "2.22alpha1"


def load():
    with open(GOLDEN) as f:
        return json.load(f)


def enc_pcm(v):
    return signals.make(v["kind"], v["n"], v["channels"], v["bps"], seed=v["seed"])


def dec_image(stream, mdat, frame_sizes):
    """the clean m4a image of a decoder stream around `mdat`"""
    from audiotools import m4a
    return m4a.m4a_file(stream["channels"], stream["bps"], 44100, 4096, stream["n"], mdat,
                        frame_sizes, create_date=CREATE_DATE, version=VERSION)


def mutate(img, case):
    b = bytearray(img)
    for pos, v in case["xor"]:
        b[pos] ^= v
    if case["cut"] is not None:
        b = b[:case["cut"]]
    return bytes(b)


# ---------------------------------------------------------------- damage sweep
# Every single-bit flip and every truncation of three small images, recorded
# with the reference decoder by tests/golden/make_alac_damage_golden.py into
# tests/golden/alac_damage_<name>.json.  The images are not committed: they
# are rebuilt here and checked against the recorded sha256.
DAMAGE_IMAGES = {
    # 64, 64, 64 and a verbatim frameset of 8 samples
    "mono16": dict(kind="tone", n=200, channels=1, bps=16, block=64, seed=1),
    # 48, 48 and a verbatim frameset of 4; uncompressed LSBs
    "stereo24": dict(kind="noise", n=100, channels=2, bps=24, block=48, seed=2),
    # a stereo and a mono element per frameset: 32 samples, then 8 verbatim
    "three16": dict(kind="tone", n=40, channels=3, bps=16, block=32, seed=23),
}
DAMAGE_SET_ASIDE = ("reference_died", "reference_short_block")


def damage_golden(name):
    return os.path.join(HERE, "golden", "alac_damage_%s.json" % name)


def damage_load(name):
    with open(damage_golden(name)) as f:
        return json.load(f)


def damage_image(name):
    """-> (m4a image, byte at which its mdat atom starts, source PCM)"""
    import oracle_port as op
    from audiotools import m4a
    p = DAMAGE_IMAGES[name]
    x = signals.make(p["kind"], p["n"], p["channels"], p["bps"], seed=p["seed"])
    mdat, fs = op.alac_encode(x, p["channels"], p["bps"], block_size=p["block"])
    img = m4a.m4a_file(p["channels"], p["bps"], 44100, p["block"], p["n"], mdat, fs,
                       create_date=1)
    return img, len(img) - len(mdat), x


def flip(img, bit):
    """bit 0 is the top bit of byte 0"""
    b = bytearray(img)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


def damage_cases(name, rec=None, img=None):
    """-> {"mdat": [...], "cut": [...], "header": [...]}, each a list of
    (key, image bytes, recorded outcome or None); the key is "f<bit>" for a
    flip of that bit of the image and "t<length>" for a truncation.  The
    recorded outcome is [return code, PCM bytes, md5 prefix]; a return code
    that is no integer 0 or 1 tells how the reference died."""
    rec = rec or damage_load(name)
    if img is None:
        img = damage_image(name)[0]
    start = rec["mdat_start"]
    table = rec["outcomes"]
    out = {"mdat": [], "cut": [], "header": []}
    m, d = rec["mdat_flips"], rec["md5_digits"]
    for i, (rc, nbytes) in enumerate(zip(m["rc"], m["bytes"])):
        key = "f%d" % (8 * start + i)
        o = [rec["set_aside"]["reference_died"][key], 0, ""] if rc == "x" else \
            [int(rc), nbytes, m["md5"][d * i:d * (i + 1)]]
        out["mdat"].append((key, flip(img, 8 * start + i), o))
    for n, o in enumerate(rec["truncations"]):
        out["cut"].append(("t%d" % n, img[:n], table[o]))
    for bit, o in zip(rec["header_flips"]["bits"], rec["header_flips"]["outcomes"]):
        out["header"].append(("f%d" % bit, flip(img, bit), table[o]))
    return out


_PORT_PCM_CAP = 1 << 16


def port_outcome(data):
    """oracle/alac_port.c on one image -> (status, int32 PCM, bits per
    sample): status 100 + the header's status when the header is refused"""
    import ctypes

    import numpy as np
    import oracle_port as op
    lib = op._alac_lib()
    info = op.AlacInfo()
    st = lib.alacport_read_info(data, len(data), ctypes.byref(info), None, 0)
    if st:
        return 100 + st, np.zeros(0, np.int32), info.bits_per_sample
    pcm = np.empty(_PORT_PCM_CAP, dtype=np.int32)
    got = ctypes.c_uint64()
    code = lib.alacport_decode(data, len(data), ctypes.byref(info), info.mdat_offset,
                               info.total_frames, pcm.ctypes.data_as(ctypes.c_void_p),
                               _PORT_PCM_CAP, ctypes.byref(got), None, None, 0, None)
    if code == -1:  # more output than the buffer here holds
        r = op.alac_decode(data, info)
        return r["code"], r["pcm"], info.bits_per_sample
    return code, pcm[:got.value * max(1, info.channels)].copy(), info.bits_per_sample


def matches_reference(status, pcm, bps, outcome):
    """the mapping of test_decoder_vectors_batch: a header the port refuses
    is return code 1 and no bytes; otherwise the same success class and the
    same PCM bytes"""
    import hashlib

    import oracle_port as op
    rc, nbytes, md5 = outcome
    if status >= 100:
        return rc == 1 and nbytes == 0
    if bps not in (8, 16, 24) and len(pcm):
        return False  # no sample format of the reference's: nothing to compare
    b = op.pcm_bytes(pcm, bps) if len(pcm) else b""
    return (status == 0) == (rc == 0) and len(b) == nbytes and \
        hashlib.md5(b).hexdigest()[:len(md5)] == md5
