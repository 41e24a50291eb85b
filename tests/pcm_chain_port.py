"""A numpy port of one row of the converter chain (csrc/pcm_chain.hip): the
channel map in numpy; downmix, average and bits per sample through
oracle_port.convert, the C port that already checks pcm_convert.hip; the
fused DOWNMIX_AVERAGE as the composition of the two."""
import numpy as np

import oracle_port

MAP, DOWNMIX, AVERAGE, DOWNMIX_AVERAGE = range(4)


def out_channels(op, in_channels, channel_map=None):
    if op == MAP:
        return in_channels if channel_map is None else len(channel_map)
    return 2 if op == DOWNMIX else 1


def dither_from(dither, bit0):
    """the dither stream from bit bit0 on, as bytes that start at bit 0"""
    bits = np.unpackbits(np.frombuffer(bytes(dither), dtype=np.uint8))[bit0:]
    return np.packbits(bits).tobytes() + b"\0"


def channel_stage(pcm, in_channels, op, bps, channel_map=None, mask=0):
    x = np.ascontiguousarray(pcm, dtype=np.int32)
    if op == MAP:
        frames = x.reshape(-1, in_channels)
        if channel_map is None:
            channel_map = list(range(in_channels))
        out = np.zeros((len(frames), len(channel_map)), dtype=np.int32)
        for k, m in enumerate(channel_map):
            if m is not None:
                out[:, k] = frames[:, m]
        return out.reshape(-1)
    if op == DOWNMIX:
        return oracle_port.convert(oracle_port.CONV_DOWNMIX, x, in_channels, bps, mask=mask)
    if op == AVERAGE:
        return oracle_port.convert(oracle_port.CONV_AVERAGE, x, in_channels, bps)
    two = oracle_port.convert(oracle_port.CONV_DOWNMIX, x, in_channels, bps, mask=mask)
    return oracle_port.convert(oracle_port.CONV_AVERAGE, two, 2, bps)


def bits_stage(pcm, channels, in_bps, out_bps, dither=b"", bit0=0):
    if in_bps == out_bps:
        return np.ascontiguousarray(pcm, dtype=np.int32)
    d = dither_from(dither, bit0) if out_bps < in_bps else b""
    return oracle_port.convert(oracle_port.CONV_BPS, pcm, channels, in_bps, out_bps, dither=d)


def convert_row(pcm, in_channels, op, in_bps, out_bps, channel_map=None, mask=0, dither=b"",
                bit0=0):
    """interleaved samples of one track -> the row's int32 output"""
    x = channel_stage(pcm, in_channels, op, in_bps, channel_map, mask)
    return bits_stage(x, out_channels(op, in_channels, channel_map), in_bps, out_bps, dither,
                      bit0)
