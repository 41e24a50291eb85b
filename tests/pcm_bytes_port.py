"""numpy restatement of the reference's ten packed-PCM converters and their
inverses (FrameList_*_char_to_int / FrameList_int_to_*_char, reference
src/pcm.c:1599-1960, picked by FrameList_get_char_to_int_converter): 1, 2 or
3 bytes per sample, little or big endian, signed or unsigned.  Written from
the C, byte by byte, without audiotools.pcm, so that the two can be compared
with each other and with the GPU kernels.

One difference from the C, on purpose: for a value outside the layout's range
the reference's signed writers clamp, this package's FrameList.to_bytes (and
so the kernels) keeps the low bits.  `pack` keeps the low bits; values in
range are written identically either way."""
import numpy as np

# (bytes per sample, big endian, signed); one byte has no order
LAYOUTS = [(1, False, True), (1, False, False),
           (2, False, True), (2, False, False), (2, True, True), (2, True, False),
           (3, False, True), (3, False, False), (3, True, True), (3, True, False)]


def layout_id(layout):
    b, be, sg = layout
    return "%s%s%d" % ("S" if sg else "U", "" if b == 1 else ("B" if be else "L"), 8 * b)


def unpack(data, layout):
    """packed bytes -> int32 values"""
    b, be, sg = layout
    s = np.frombuffer(bytes(data), dtype=np.uint8).reshape(-1, b).astype(np.int64)
    order = range(b) if be else range(b - 1, -1, -1)   # most significant first
    u = np.zeros(len(s), dtype=np.int64)
    for k in order:
        u = (u << 8) | s[:, k]
    if sg:
        # "if (s[msb] & 0x80) return -(int)(0x1000000 - u)"
        neg = u >= (1 << (8 * b - 1))
        u = np.where(neg, -((1 << (8 * b)) - u), u)
    else:
        u = u - (1 << (8 * b - 1))
    return u.astype(np.int32)


def pack(values, layout):
    """int values -> packed bytes, the low 8 * bytes bits kept"""
    b, be, sg = layout
    i = np.asarray(values).astype(np.int64)
    if not sg:
        i = i + (1 << (8 * b - 1))
    out = np.empty((len(i), b), dtype=np.uint8)
    for k in range(b):                       # k-th least significant byte
        out[:, (b - 1 - k) if be else k] = (i >> (8 * k)) & 0xFF
    return out.tobytes()


def value_range(layout):
    b = layout[0]
    return -(1 << (8 * b - 1)), (1 << (8 * b - 1)) - 1
