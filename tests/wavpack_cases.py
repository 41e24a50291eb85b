"""The WavPack test inputs, shared by tests/golden/make_wavpack_golden.py
(which encodes them with the reference encoder and records what the reference
decoder makes of every image) and the WavPack tests.

A case is (name, encoder options, channels, bits, rate, interleaved samples).
The shapes are the smallest at which each decoder path can still go wrong:
last blocks shorter than every term's history (8 for term 8, 2 for 17/18),
blocks of 1 to 9 samples without passes, every pass count the encoder knows, with and without joint
stereo, every channel split, zero runs and the unary escape."""
import numpy as np

import signals

MASKS = {1: "4", 2: "3", 3: "7", 6: "3F", 8: "FF"}


def _opts(ch, bps, rate=44100, block=50, passes=5, joint=False, false=False, wasted=False):
    o = ["-c", str(ch), "-m", MASKS[ch], "-r", str(rate), "-b", str(bps), "-B", str(block),
         "-p", str(passes)]
    return o + (["-j"] if joint else []) + (["-f"] if false else []) + \
        (["-w"] if wasted else [])


def impulse(n, ch, bps, at):
    x = np.zeros((n, ch), dtype=np.int32)
    x[at, :] = (1 << (bps - 1)) - 1
    if ch > 1:
        x[at, 1] = -(1 << (bps - 1))
    return x.reshape(-1)


def low_tones(n, ch, seed):
    """two low tones per channel and a little noise: a long block that the
    predictor follows, so that its image stays small"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    out = []
    for c in range(ch):
        f1, f2 = rng.uniform(100, 400), rng.uniform(400, 1500)
        x = 9000 * np.sin(2 * np.pi * f1 * t / 44100) + 5000 * np.sin(2 * np.pi * f2 * t / 44100)
        out.append(np.round(x + rng.normal(0, 2.0, n)))
    return np.stack(out, 1).reshape(-1).astype(np.int32)


N = 120  # frames of most cases: blocks of 50, 50 and 20


def cases():
    out = []

    def add(name, ch, bps, x, **kw):
        out.append((name, _opts(ch, bps, **kw), ch, bps, kw.get("rate", 44100),
                    np.asarray(x, dtype=np.int32)))

    # block lengths below and at the history depths
    for L in (1, 2, 3, 7, 8, 9, 200):
        for ch in (1, 2):
            # the reference encoder needs a whole history from the block
            # before, so with passes a short block can only come last
            B = 200 if L == 200 else 50
            add("len%d_c%d_p16" % (L, ch), ch, 16,
                signals.make("tone", B + L, ch, 16, seed=L * 10 + ch), block=B,
                passes=16, joint=(ch == 2))
            n = 2 * L + (L + 1) // 2
            add("len%d_c%d_p0" % (L, ch), ch, 16,
                signals.make("tone", n, ch, 16, seed=L * 10 + ch + 5), block=L, passes=0)
    add("len22050_c2", 2, 16, low_tones(22050 + 100, 2, seed=5), block=22050)
    add("empty_c2", 2, 16, np.zeros(0, dtype=np.int32))
    # channel splits
    for ch in (1, 2, 3, 6, 8):
        add("chan%d" % ch, ch, 16, signals.make("tone", N, ch, 16, seed=70 + ch))
    add("chan6_b24_j", 6, 24, signals.make("tone", N, 6, 24, seed=76), joint=True)
    # sample widths and signals
    for bps in (8, 16, 24):
        for ch in (1, 2):
            for kind in ("tone", "noise", "silence"):
                add("%s_c%d_b%d" % (kind, ch, bps), ch, bps,
                    signals.make(kind, N, ch, bps, seed=bps + ch))
            add("impulse_c%d_b%d" % (ch, bps), ch, bps, impulse(200, ch, bps, 80), block=200)
            add("constant_c%d_b%d" % (ch, bps), ch, bps, np.full(N * ch, 57, dtype=np.int32))
    # passes, with and without joint stereo
    for p in (0, 1, 2, 5, 10, 16):
        for j in (False, True):
            add("passes%d_j%d" % (p, j), 2, 16, signals.make("tone", N, 2, 16, seed=p),
                passes=p, joint=j)
        add("passes%d_mono" % p, 1, 16, signals.make("tone", N, 1, 16, seed=p + 20), passes=p)
    add("noise_p16_j_b24", 2, 24, signals.make("noise", N, 2, 24, seed=3), passes=16,
        joint=True)
    # false stereo: identical channels
    x = signals.make("tone", N, 1, 16, seed=9)
    add("false_stereo", 2, 16, np.repeat(x, 2), false=True)
    add("false_stereo_w", 2, 24, np.repeat(signals.make("tone", N, 1, 16, seed=10), 2) << 3,
        false=True, wasted=True, joint=True)
    # extended integers: 1 and 5 zero low bits
    for z in (1, 5):
        for ch in (1, 2):
            add("wasted%d_c%d" % (z, ch), ch, 16,
                (signals.make("tone", N, ch, 16, seed=z) >> z) << z, wasted=True)
    add("wasted5_c2_b24_j", 2, 24, (signals.make("tone", N, 2, 24, seed=8) >> 5) << 5, wasted=True,
        joint=True)
    # sample rates; 12345 needs the sample-rate sub-block
    for rate in (48000, 96000, 12345):
        add("rate%d" % rate, 2, 16, signals.make("tone", N, 2, 16, seed=rate % 97), rate=rate)
    add("rate12345_c3", 3, 16, signals.make("tone", N, 3, 16, seed=12), rate=12345)
    # the images the damage cases are cut from
    add(DAMAGE_STEREO, 2, 16, (signals.make("tone", 600, 2, 16, seed=31) >> 2) << 2, passes=5,
        joint=True, wasted=True, false=True, block=200)
    add(DAMAGE_3CH, 3, 16, signals.make("tone", 400, 3, 16, seed=32), block=200)
    return out


DAMAGE_STEREO = "damage_stereo"
DAMAGE_3CH = "damage_c3"
# images patched from a -w image: the four int32-info bytes rewritten to
# one-bits / duplicate-bits, which the reference encoder never writes
PATCHED = (("wasted5_c2_onebits", "wasted5_c2", (0, 0, 5, 0)),
           ("wasted5_c2_dupbits", "wasted5_c2", (0, 0, 0, 5)),
           ("wasted1_c1_dupbits", "wasted1_c1", (0, 0, 0, 1)))
FIXTURES = ("silence.wv", "wavpack-combo.wv")
# all eight bits of every byte of the first block header are flipped, one bit
# of every byte after it
DENSE_BYTES = 32


def flip_cases(nbytes, limit=None):
    """(byte, bit) of the single-bit flips over an image (its first `limit`
    bytes)"""
    out = []
    for i in range(nbytes if limit is None else min(limit, nbytes)):
        if i < DENSE_BYTES:
            out.extend((i, b) for b in range(8))
        else:
            out.append((i, (i * 5 + 3) % 8))
    return out


def pcm_bytes(samples, bps):
    """little-endian signed PCM at every width, as wvenc reads and wvdec
    writes it"""
    a = np.asarray(samples)
    if bps == 8:
        return a.astype(np.int8).tobytes()
    if bps == 16:
        return a.astype("<i2").tobytes()
    return np.ascontiguousarray(a.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()


def load_vectors():
    """-> (the recorded vectors, {name: image bytes}) from tests/golden"""
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "wavpack_vectors.json")) as f:
        g = json.load(f)
    with open(os.path.join(here, "wavpack_images.bin"), "rb") as f:
        blob = f.read()
    images = {}
    for name, v in g["images"].items():
        if name in FIXTURES:
            with open(os.path.join(here, "fixtures", name), "rb") as f:
                images[name] = f.read()
        else:
            images[name] = blob[v["offset"]:v["offset"] + v["image_bytes"]]
    return g, images


INCONSISTENT_BLOCK = 17  # ATG_WVD_INCONSISTENT_BLOCK: the flagged damage cases


def damage_cases(g, images):
    """[(label, image, status, PCM bytes, PCM md5, flagged)] of the recorded
    flips and cuts.  They are grouped by outcome, "status,pcm" -> the flips as
    8 * byte + bit, the cuts as lengths; pcm indexes the table of distinct
    (length, md5) of the PCM written"""
    out = []
    pcm = g["damage"]["pcm"]
    for kind in ("flips", "cuts"):
        for name, groups in sorted(g["damage"][kind].items()):
            rows = sorted((v, k) for k, vs in groups.items() for v in vs)
            for v, k in rows:
                status, key = (int(x) for x in k.split(","))
                if kind == "flips":
                    d = bytearray(images[name])
                    d[v >> 3] ^= 1 << (v & 7)
                    label, img = "%s flip %d.%d" % (name, v >> 3, v & 7), bytes(d)
                else:
                    label, img = "%s cut %d" % (name, v), images[name][:v]
                out.append((label, img, status, pcm[key][0], pcm[key][1],
                            status == INCONSISTENT_BLOCK))
    return out


def hostile_images(images):
    """two images no single-bit flip reaches: [(label, image)].  A
    channel-info sub-block that declares 0 channels, and a first block that
    claims 2^31 frames of a stream of 2^32 - 1"""
    img = bytearray(images["chan3"])
    pos = 32
    while img[pos] & 0x3F != 0xD:                 # the channel-info sub-block
        pos += (4 if img[pos] & 0x80 else 2) + 2 * img[pos + 1]
    img[pos + 2] = 0
    big = bytearray(images[DAMAGE_STEREO])
    big[12:16] = (0xFFFFFFFF).to_bytes(4, "little")
    big[20:24] = (0x80000000).to_bytes(4, "little")
    return [("zero channels", bytes(img)), ("2^31 frames in a block", bytes(big))]
