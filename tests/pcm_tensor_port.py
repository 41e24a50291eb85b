"""The numpy port of csrc/pcm_tensor.hip, over audiotools/pcm.py itself:
FrameList.to_float / channel for the way to a tensor, FloatFrameList.to_int
for the way back, numpy astype for the narrower float types.  A row is laid
out as the kernel lays it out: channel runs channel_stride apart, zeros from
the row's length to pad_frames, everything else left alone.

Floats are compared as bit patterns (bits()), so -0.0 and subnormals count.
"""
import numpy as np

from audiotools import pcm

F16, F32, F64, I32 = range(4)
DTYPES = {F16: np.float16, F32: np.float32, F64: np.float64, I32: np.int32}
UINTS = {2: np.uint16, 4: np.uint32, 8: np.uint64}


def bits(a):
    """the bit patterns of an array"""
    a = np.ascontiguousarray(a)
    return a.view(UINTS[a.dtype.itemsize])


def to_values(samples, channels, bits_per_sample, dtype):
    """interleaved samples -> [channels, frames] elements of `dtype`"""
    fl = pcm.FrameList._wrap(np.asarray(samples, dtype=np.int32), channels, bits_per_sample)
    if dtype == I32:
        return np.stack([fl.channel(c).samples for c in range(channels)])
    as_float = fl.to_float()
    planes = np.stack([as_float.channel(c).samples for c in range(channels)])
    if dtype == F16:
        # float64 -> float32 -> float16, each nearest even
        return planes.astype(np.float32).astype(np.float16)
    return planes.astype(DTYPES[dtype])


def to_tensor_row(out, samples, channels, bits_per_sample, dtype, pad_frames, out_offset,
                  channel_stride):
    """one row into the flat element buffer `out`, in place"""
    values = to_values(samples, channels, bits_per_sample, dtype)
    frames = values.shape[1]
    for c in range(channels):
        at = out_offset + c * channel_stride
        out[at:at + frames] = values[c]
        out[at + frames:at + pad_frames] = 0


def from_values(planes, bits_per_sample):
    """[channels, frames] elements -> interleaved int32 samples"""
    planes = np.asarray(planes)
    channels = planes.shape[0]
    if planes.dtype == np.int32:
        lo, hi = -(1 << (bits_per_sample - 1)), (1 << (bits_per_sample - 1)) - 1
        return np.clip(planes.astype(np.int64), lo, hi).T.reshape(-1).astype(np.int32)
    # the widening is exact
    runs = [pcm.FloatFrameList._wrap(planes[c].astype(np.float64), 1) for c in range(channels)]
    return pcm.from_float_channels(runs).to_int(bits_per_sample).samples


def from_tensor_row(buf, in_offset, channel_stride, frames, channels, bits_per_sample):
    """one row out of the flat element buffer `buf` -> interleaved samples"""
    planes = np.stack([buf[in_offset + c * channel_stride:in_offset + c * channel_stride + frames]
                       for c in range(channels)])
    return from_values(planes, bits_per_sample)
