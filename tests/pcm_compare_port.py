"""numpy restatement of what csrc/pcm_compare.hip computes: the view rule, the
first differing frame of two views, and the offset search by brute force.
A checker only: nothing on the product path imports it."""
import numpy as np


def view(src, channels, window_offset, frames):
    """`frames` frames of the view over `src` (interleaved samples, any
    integer dtype): view frame i is source frame window_offset + i, silence
    outside the source.  -> int64 array [frames, channels]"""
    src = np.asarray(src).astype(np.int64).reshape(-1, channels)
    out = np.zeros((frames, channels), dtype=np.int64)
    lo = max(0, -window_offset)                       # first view frame inside
    hi = min(frames, len(src) - window_offset)        # one past the last
    if lo < hi:
        out[lo:hi] = src[window_offset + lo:window_offset + hi]
    return out


def first_mismatch(a, b):
    """smallest frame at which two [frames, channels] arrays differ, or None"""
    bad = np.nonzero((a != b).any(axis=1))[0]
    return int(bad[0]) if len(bad) else None


def compare(src_a, wo_a, src_b, wo_b, frames, channels):
    return first_mismatch(view(src_a, channels, wo_a, frames),
                          view(src_b, channels, wo_b, frames))


def best_offset(src_a, wo_a, src_b, wo_b, frames, channels, max_offset):
    """the k of smallest |k| in [-max_offset, max_offset] with
    A(i) == B(i + k) for every i in [0, frames), +k before -k; None if none"""
    a = view(src_a, channels, wo_a, frames)
    # B over view frames [-K, frames + K)
    wide = view(src_b, channels, wo_b - max_offset, frames + 2 * max_offset)
    for m in range(max_offset + 1):
        for k in ((m, -m) if m else (0,)):
            if np.array_equal(a, wide[max_offset + k:max_offset + k + frames]):
                return k
    return None
