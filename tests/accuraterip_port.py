"""Plain numpy restatement of the AccurateRip checksums (test aid, CPU).

A track is stereo 16-bit; frame i (from 1) has the value
(uint16(right) << 16) | uint16(left) and counts when
start <= index0 + i <= end (the reference's ChecksumV1 / ChecksumV2 rule,
its uint32 wrap of the end included).  `sweep` recomputes the whole sum for
every offset, reading silence outside the region -- the brute force the GPU
sweep is checked against."""
import numpy as np

M32 = 0xFFFFFFFF


def offsets(is_first, is_last, sample_rate, total_pcm_frames):
    """(start_offset, end_offset) of the range rule"""
    skip = (sample_rate // 75) * 5
    start = skip if is_first else 0
    end = (total_pcm_frames - skip) & M32 if is_last else total_pcm_frames & M32
    return start, end


def values(pcm):
    """interleaved stereo samples (any integer dtype) -> uint64 frame values"""
    a = np.asarray(pcm).astype(np.int64).reshape(-1, 2)
    return (((a[:, 1] & 0xFFFF) << 16) | (a[:, 0] & 0xFFFF)).astype(np.uint64)


def checksums(pcm, is_first, is_last, sample_rate, total_pcm_frames=None, index0=0):
    """(v1, v2) of the frames in `pcm`, indexed from index0 + 1"""
    w = values(pcm)
    n = len(w)
    start, end = offsets(is_first, is_last, sample_rate,
                         n if total_pcm_frames is None else total_pcm_frames)
    idx = np.arange(index0 + 1, index0 + n + 1, dtype=np.uint64)
    keep = (idx >= start) & (idx <= end)
    prod = w[keep] * idx[keep]  # below 2^64: both factors below 2^32
    v1 = int((prod & np.uint64(M32)).sum(dtype=np.uint64)) & M32
    hi = int((prod >> np.uint64(32)).sum(dtype=np.uint64))
    return v1, (v1 + hi) & M32


def window(image, pcm_offset, pcm_frames, lo_frame, hi_frame):
    """interleaved samples of frames [pcm_offset, pcm_offset + pcm_frames) of
    the interleaved stereo `image`, silence outside [lo_frame, hi_frame)"""
    img = np.asarray(image).reshape(-1, 2)
    out = np.zeros((pcm_frames, 2), dtype=np.int64)
    a = max(pcm_offset, lo_frame, 0)
    b = min(pcm_offset + pcm_frames, hi_frame, len(img))
    if a < b:
        out[a - pcm_offset:b - pcm_offset] = img[a:b]
    return out.reshape(-1)


def sweep(image, pcm_offset, pcm_frames, lo_frame, hi_frame, is_first, is_last,
          sample_rate, max_offset, total_pcm_frames=None, index0=0):
    """brute force: v1 at every offset k in [-max_offset, max_offset], one
    whole recomputation each -> list of 2 * max_offset + 1 values.  The
    offsets are taken 32 at a time as rows of one matrix (row k is the
    window at offset k); every row is still summed in full."""
    K = max_offset
    ext = values(window(image, pcm_offset - K, pcm_frames + 2 * K, lo_frame, hi_frame))
    rows = np.lib.stride_tricks.sliding_window_view(ext, pcm_frames)  # rows[k + K]
    start, end = offsets(is_first, is_last, sample_rate,
                         pcm_frames if total_pcm_frames is None else total_pcm_frames)
    idx = np.arange(index0 + 1, index0 + pcm_frames + 1, dtype=np.uint64)
    weight = np.where((idx >= start) & (idx <= end), idx, np.uint64(0))
    out = []
    for r in range(0, 2 * K + 1, 32):
        # uint64 sums wrap mod 2^64, which keeps them right mod 2^32
        s = (rows[r:r + 32] * weight).sum(axis=1, dtype=np.uint64)
        out.extend(int(x) & M32 for x in s)
    return out
