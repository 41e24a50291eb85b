"""The True Audio test inputs, shared by tests/golden/make_tta_golden.py (which
records what the reference encoder and decoder make of them) and the TTA
tests (which hold tta_port and the GPU codec to the record)."""
import numpy as np

import signals

RATE = 8000
BLOCK = (RATE * 256) // 245  # 8359


def quiet_then_full_scale(channels, bps, loud):
    """2000 samples of +-1, `loud` alternating full-scale samples, +-1 up to
    3000 samples: after the quiet passage both Rice parameters sit at 0, so
    every loud sample costs a unary run about as long as its value"""
    n = 3000
    x = np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int64)
    hi, lo = (1 << (bps - 1)) - 1, -(1 << (bps - 1))
    x[2000:2000 + loud] = np.where(np.arange(loud) % 2 == 0, hi, lo)
    return np.repeat(x[:, None], channels, 1).reshape(-1).astype(np.int32)


def odd_correlated(n):
    """three channels whose differences are negative and odd, so that the
    halving toward zero differs from an arithmetic shift"""
    i = np.arange(n, dtype=np.int64)
    a = (i * 37) % 2001 - 1000
    b = a - (2 * (i % 50) + 1)          # b - a odd and negative
    c = b - (2 * ((i * 7) % 90) + 3)    # c - b odd and negative
    return np.stack([a, b, c], 1).reshape(-1).astype(np.int32)


def encoder_cases():
    """[(name, channels, bps, rate, samples)]"""
    out = []
    for ch in (1, 2, 3, 6):
        for bps in (8, 16, 24):
            for kind in ("tone", "noise", "silence", "chirp"):
                for n in (1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 100):
                    seed = ch * 1000 + bps * 10 + n % 7
                    out.append(("%s_c%d_b%d_n%d" % (kind, ch, bps, n), ch, bps, RATE,
                                signals.make(kind, n, ch, bps, seed=seed)))
    n = (44100 * 256) // 245 + 7
    out.append(("tone_c2_b16_r44100", 2, 16, 44100, signals.make("tone", n, 2, 16, seed=44)))
    for ch in (1, 2):
        out.append(("quiet_loud_c%d_b16" % ch, ch, 16, RATE, quiet_then_full_scale(ch, 16, 32)))
        out.append(("quiet_loud_c%d_b24" % ch, ch, 24, RATE, quiet_then_full_scale(ch, 24, 4)))
    out.append(("odd_correlated_c3_b16", 3, 16, RATE, odd_correlated(BLOCK + 11)))
    return out


# the encoder cases whose reference output is also decoded by the reference
DECODER_CASES = (
    "tone_c1_b8_n%d" % (2 * BLOCK + 100), "noise_c1_b16_n%d" % (BLOCK + 1),
    "tone_c2_b16_n%d" % (2 * BLOCK + 100), "noise_c2_b24_n%d" % (2 * BLOCK + 100),
    "chirp_c2_b16_n%d" % BLOCK, "silence_c2_b16_n%d" % (BLOCK - 1), "tone_c2_b8_n1",
    "tone_c3_b16_n%d" % (BLOCK + 1), "noise_c3_b24_n%d" % (BLOCK - 1),
    "tone_c6_b24_n%d" % (2 * BLOCK + 100), "noise_c6_b8_n%d" % BLOCK,
    "tone_c2_b16_r44100", "quiet_loud_c1_b16", "quiet_loud_c2_b24", "odd_correlated_c3_b16",
)

FIXTURES = ("trueaudio.tta", "tta-id3-2.tta")


def pcm_bytes(samples, bps):
    """little-endian signed PCM, as the reference's tools read and write it"""
    a = np.asarray(samples)
    if bps == 8:
        return a.astype(np.int8).tobytes()
    if bps == 16:
        return a.astype("<i2").tobytes()
    return np.ascontiguousarray(a.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
