"""WavPack encoder inputs beyond tests/wavpack_cases.py, shared by
tests/golden/make_wavpack_enc_golden.py (which encodes them with the reference
encoder and records each image's length and MD5) and the encoder tests.

A case is (name, encoder options, channels, bits, rate, interleaved samples),
as in wavpack_cases.py.  The 98 cases there exercise every decoder path; these
are the smallest shapes at which the encoder's carried state can still go
wrong: parameters reset where false stereo toggles, wasted bits that change
from block to block, ten and more round trips of the state, medians decaying
into zero runs and being cleared, length edges, the remaining channel splits
and the unsigned MD5 of 8-bit samples."""
import functools

import numpy as np

import signals
from wavpack_cases import low_tones

B = 56  # frames per block of most cases


def _opts(ch, mask, bps, block=B, passes=5, joint=False, false=False, wasted=False, rate=44100):
    o = ["-c", str(ch), "-m", "%X" % mask, "-r", str(rate), "-b", str(bps), "-B", str(block),
         "-p", str(passes)]
    return o + (["-j"] if joint else []) + (["-f"] if false else []) + \
        (["-w"] if wasted else [])


def _stereo(blocks):
    """blocks: list of (left, right) arrays -> interleaved"""
    left = np.concatenate([b[0] for b in blocks])
    right = np.concatenate([b[1] for b in blocks])
    return np.stack([left, right], 1).reshape(-1).astype(np.int32)


def cases():
    out = []

    def add(name, ch, mask, bps, x, **kw):
        out.append((name, _opts(ch, mask, bps, **kw), ch, bps, kw.get("rate", 44100),
                    np.asarray(x, dtype=np.int32)))

    # false stereo toggling: the parameters are reset at both kinds of edge
    t = signals.make("tone", 3 * B, 2, 16, seed=41).reshape(-1, 2)
    eq = [(t[k * B:(k + 1) * B, 0], t[k * B:(k + 1) * B, 0]) for k in range(3)]
    df = [(t[k * B:(k + 1) * B, 0], t[k * B:(k + 1) * B, 1]) for k in range(3)]
    for p in (5, 16):
        add("false_ede_p%d" % p, 2, 3, 16, _stereo([eq[0], df[1], eq[2]]), passes=p, joint=True,
            false=True, wasted=True)
        add("false_ded_p%d" % p, 2, 3, 16, _stereo([df[0], eq[1], df[2]]), passes=p, joint=True,
            false=True, wasted=True)
    # wasted bits 3, 0, 3, then an all-zero block
    t = signals.make("tone", 4 * B, 2, 16, seed=42).reshape(-1, 2).copy()
    t[:B] = (t[:B] >> 3) << 3
    t[2 * B:3 * B] = (t[2 * B:3 * B] >> 3) << 3
    t[3 * B:] = 0
    add("wasted_303z", 2, 3, 16, t.reshape(-1), wasted=True, joint=True)
    t1 = t[:, 0].copy()
    add("wasted_303z_mono", 1, 4, 16, t1, wasted=True)
    # ten and more blocks: the state is round-tripped again and again
    n = 11 * B + 17
    for p in (10, 16):
        for j in (False, True):
            add("long_p%d_j%d" % (p, j), 2, 3, 16, signals.make("tone", n, 2, 16, seed=43 + p),
                passes=p, joint=j)
    add("long_p5_mono", 1, 4, 16, signals.make("tone", n, 1, 16, seed=44), passes=5)
    add("long_noise_b24_p16", 2, 3, 24, signals.make("noise", n, 2, 24, seed=45), passes=16,
        joint=True)
    add("long_noise_b24_p10", 2, 3, 24, signals.make("noise", n, 2, 24, seed=46), passes=10)
    # silent, loud, silent: medians decay into zero-run mode inside a block, a
    # zero run ends with the block, both channels' medians are cleared
    loud = signals.make("noise", B, 2, 16, seed=47)
    quiet = np.zeros(2 * B, dtype=np.int32)
    for p in (0, 5, 16):
        add("silent_loud_silent_p%d" % p, 2, 3, 16, np.concatenate([quiet, loud, quiet, quiet]),
            passes=p, joint=(p == 16))
    add("silent_loud_silent_mono", 1, 4, 16,
        np.concatenate([quiet[:B], loud[:B], quiet[:B], quiet[:B]]), passes=5)
    decay = signals.make("tone", 2 * B, 2, 16, seed=48).reshape(-1, 2).copy()
    decay[B // 2:] = 0        # the run starts mid-block and goes on into the next
    add("decay_mid_block", 2, 3, 16, decay.reshape(-1), passes=5)
    # length edges
    add("exact_multiple", 2, 3, 16, signals.make("tone", 3 * B, 2, 16, seed=49), passes=16,
        joint=True)
    add("one_frame", 2, 3, 16, np.array([1234, -4321]), passes=16, joint=True)
    add("one_frame_mono", 1, 4, 16, np.array([-7]), passes=5)
    add("one_block", 2, 3, 16, signals.make("tone", B, 2, 16, seed=50), passes=10)
    # the channel splits the decoder's cases do not reach
    add("chan4_33", 4, 0x33, 16, signals.make("tone", 2 * B + 5, 4, 16, seed=51), joint=True)
    add("chan4_107", 4, 0x107, 16, signals.make("tone", 2 * B + 5, 4, 16, seed=52))
    add("chan5_37", 5, 0x37, 16, signals.make("tone", 2 * B + 5, 5, 16, seed=53), passes=10,
        joint=True)
    x = signals.make("tone", 3 * B + 5, 6, 16, seed=54).reshape(-1, 6).copy()
    x[B:2 * B, 1] = x[B:2 * B, 0]            # front pair false stereo in the middle block
    x[:, 5] = x[:, 4]                        # back pair false stereo throughout
    x[:, 2] = (x[:, 2] >> 2) << 2
    add("chan6_3F_fjw_p16", 6, 0x3F, 16, x.reshape(-1), passes=16, joint=True, false=True,
        wasted=True)
    add("stereo_b8_blocks", 2, 3, 8, signals.make("tone", 3 * B + 9, 2, 8, seed=55), passes=5,
        joint=True)
    # the "standard" mode of WavPackAudio on a real-length read, and its deepest
    for p in (5, 16):
        add("std_44100" if p == 5 else "std_44100_p16", 2, 3, 16, low_tones(44137, 2, seed=56),
            block=44100, passes=p, joint=True, false=True, wasted=True)
    return out


def load_vectors():
    """{name: {"bytes": image length, "md5": hex digest}} from tests/golden"""
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "wavpack_enc_vectors.json")) as f:
        return json.load(f)["images"]


@functools.lru_cache(maxsize=None)
def by_name():
    return {c[0]: c for c in cases()}


@functools.lru_cache(maxsize=None)
def port_image(name):
    """the image tests/wavpack_enc_port.py makes of a case: computed once,
    shared by the tests that compare against it"""
    import wavpack_enc_port as port
    _, opts, ch, bps, rate, x = by_name()[name]
    kw = port.parse_options(opts)
    return port.encode(x, kw["channels"], kw["mask"], kw["bps"], kw["rate"], kw["block_size"],
                       kw["passes"], kw["joint"], kw["false"], kw["wasted"])
