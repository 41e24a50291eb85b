"""Shorten (.shn) in plain Python: the checker the GPU codec is held to.

Restates the reference's src/encoders/shn.c and src/decoders/shn.c (and the
header walk of audiotools/shn.py) command for command, quirks included:

* the encoder's history accumulates (tail(history + shifted, 3)), the
  decoder's is the tail of the last block alone, so blocks shorter than 3 in
  mid-stream do not round-trip;
* all sample arithmetic wraps at 32 bits, shnmean() truncates toward zero.

Where the reference's behaviour is undefined or unbounded the decoder stops
with ATG_SHN_UNSUPPORTED; the caps are those of include/atgpu.h.

A Builder writes any command sequence, which the reference encoder cannot.
"""
import struct

import numpy as np

OK, END_OF_STREAM, IOERROR, UNKNOWN_COMMAND, INVALID_MAGIC_NUMBER, \
    INVALID_SHORTEN_VERSION, UNSUPPORTED_FILE_TYPE, UNSUPPORTED = range(8)

# the limits declared in include/atgpu.h
MAX_CHANNELS = 256
MAX_LPC_COUNT = 32
MAX_MEAN_COUNT = 64
MAX_TRACK_SAMPLES = 1 << 28
MAX_ENCODE_BLOCK = 4096

(FN_DIFF0, FN_DIFF1, FN_DIFF2, FN_DIFF3, FN_QUIT, FN_BLOCKSIZE, FN_BITSHIFT, FN_QLPC, FN_ZERO,
 FN_VERBATIM) = range(10)


# how often sample arithmetic left the 32-bit range: signed overflow, which
# is undefined in the reference's C and wraps here
WRAPS = [0]


def i32(x):
    if not -0x80000000 <= x <= 0x7FFFFFFF:
        WRAPS[0] += 1
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


def cdiv(a, b):
    """C integer division: truncates toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


# ---------------------------------------------------------------- bit output
class BitWriter(object):
    def __init__(self):
        self.chunks = []
        self.acc = 0
        self.n = 0
        self.bits = 0

    def write(self, count, value):
        if count == 0:
            return
        self.acc = (self.acc << count) | (value & ((1 << count) - 1))
        self.n += count
        self.bits += count
        if self.n >= 4096:
            keep = self.n & 7
            whole = self.acc >> keep
            self.chunks.append(whole.to_bytes((self.n - keep) // 8, "big"))
            self.acc &= (1 << keep) - 1
            self.n = keep

    def unsigned(self, c, value):
        msb = value >> c
        self.write(msb, 0)
        self.write(1, 1)
        self.write(c, value)

    def signed(self, c, value):
        self.unsigned(c + 1, (value << 1) if value >= 0 else (((-value - 1) << 1) + 1))

    def long(self, value):
        if value == 0:
            self.unsigned(2, 0)
            self.unsigned(0, 0)
        else:
            n = value.bit_length()
            self.unsigned(2, n)
            self.unsigned(n, value)

    def byte_align(self):
        if self.bits & 7:
            self.write(8 - (self.bits & 7), 0)

    def getvalue(self):
        assert self.n % 8 == 0
        tail = self.acc.to_bytes(self.n // 8, "big") if self.n else b""
        return b"".join(self.chunks) + tail


def file_type(bps, is_big_endian, signed_samples):
    if bps == 8:
        return 1 if signed_samples else 2
    if signed_samples:
        return 3 if is_big_endian else 5
    return 4 if is_big_endian else 6


def write_prefix(w, ftype, channels, block_size, max_lpc=0, mean_count=0, skip=0):
    w.write(32, struct.unpack(">I", b"ajkg")[0])
    w.write(8, 2)
    for v in (ftype, channels, block_size, max_lpc, mean_count, skip):
        w.long(v)


def write_verbatim(w, data):
    w.unsigned(2, FN_VERBATIM)
    w.unsigned(5, len(data))
    for b in bytearray(data):
        w.unsigned(8, b)


def finish(w):
    """QUIT, byte-align, pad until the count after the 5-byte magic and
    version is a multiple of 4"""
    w.unsigned(2, FN_QUIT)
    w.byte_align()
    while (w.bits // 8 - 5) % 4:
        w.write(8, 0)
    return w.getvalue()


# ------------------------------------------------------------------- encoder
def wasted_bits(ch):
    acc = 0
    for s in ch:
        acc |= s
    if acc == 0:
        return 0
    acc &= 0xFFFFFFFF
    return (acc & -acc).bit_length() - 1


def best_diff(samples, prev):
    """calculate_best_diff -> (diff, energy, residuals)"""
    p = [0] * (3 - len(prev)) + list(prev[-3:]) if len(prev) < 3 else list(prev[-3:])
    full = np.array(p + list(samples), dtype=np.int64)
    d1 = np.diff(full)           # len + 2
    d2 = np.diff(d1)             # len + 1
    d3 = np.diff(d2)             # len
    s1 = int(np.abs(d1[2:]).sum()) & 0xFFFFFFFF
    s2 = int(np.abs(d2[1:]).sum()) & 0xFFFFFFFF
    s3 = int(np.abs(d3).sum()) & 0xFFFFFFFF
    if s1 < min(s2, s3):
        diff, s, r = 1, s1, d1[2:]
    elif s2 < s3:
        diff, s, r = 2, s2, d2[1:]
    else:
        diff, s, r = 3, s3, d3
    energy = 0
    while ((len(samples) << energy) & 0xFFFFFFFF) < s:
        energy += 1
    return diff, energy, [int(v) for v in r]


def encode(samples, channels, bps, block_size=256, is_big_endian=False, signed_samples=True,
           header=b"", footer=b"", frame_sizes=None):
    """interleaved int samples -> the bytes encode_shn writes; frame_sizes
    are the lengths the reader's read() calls returned (default: block_size
    until the data runs out)"""
    if bps not in (8, 16):
        raise ValueError("unsupported bits per sample")
    x = np.asarray(samples, dtype=np.int64).reshape(-1, channels)
    total = len(x)
    if frame_sizes is None:
        frame_sizes = [min(block_size, total - p) for p in range(0, total, block_size)]
    assert sum(frame_sizes) == total
    w = BitWriter()
    write_prefix(w, file_type(bps, is_big_endian, signed_samples), channels, block_size)
    write_verbatim(w, header)
    encode_audio(w, x, frame_sizes, block_size, 0 if signed_samples else 1 << (bps - 1))
    if footer:
        write_verbatim(w, footer)
    return finish(w)


def encode_audio(w, x, frame_sizes, block_size, adjust):
    channels = x.shape[1]
    wrapped = [[] for _ in range(channels)]
    left_shift = 0
    pos = 0
    for n in frame_sizes:
        if n != block_size:
            block_size = n
            w.unsigned(2, FN_BLOCKSIZE)
            w.long(block_size)
        for c in range(channels):
            ch = [int(v) + adjust for v in x[pos:pos + n, c]]
            if not any(ch):
                w.unsigned(2, FN_ZERO)
                wrapped[c] = (wrapped[c] + ch)[-3:]
                continue
            wb = wasted_bits(ch)
            if wb != left_shift:
                left_shift = wb
                w.unsigned(2, FN_BITSHIFT)
                w.unsigned(2, left_shift)
            shifted = [v >> left_shift for v in ch]
            diff, energy, res = best_diff(shifted, wrapped[c])
            w.unsigned(2, diff)
            w.unsigned(3, energy)
            for r in res:
                w.signed(energy, r)
            wrapped[c] = (wrapped[c] + shifted)[-3:]
        pos += n


# ------------------------------------------------------------ stream builder
class Builder(object):
    """writes any Shorten command sequence"""

    def __init__(self, ftype=5, channels=1, block_length=256, max_lpc=0, mean_count=0, skip=0):
        self.w = BitWriter()
        write_prefix(self.w, ftype, channels, block_length, max_lpc, mean_count, skip)
        self.w.write(8 * skip, 0)

    def diff(self, order, energy, residuals):
        self.w.unsigned(2, order)
        self.w.unsigned(3, energy)
        for r in residuals:
            self.w.signed(energy, int(r))
        return self

    def qlpc(self, energy, coeffs, residuals):
        self.w.unsigned(2, FN_QLPC)
        self.w.unsigned(3, energy)
        self.w.unsigned(2, len(coeffs))
        for c in coeffs:
            self.w.signed(5, int(c))
        for r in residuals:
            self.w.signed(energy, int(r))
        return self

    def zero(self):
        self.w.unsigned(2, FN_ZERO)
        return self

    def blocksize(self, n):
        self.w.unsigned(2, FN_BLOCKSIZE)
        self.w.long(n)
        return self

    def bitshift(self, s):
        self.w.unsigned(2, FN_BITSHIFT)
        self.w.unsigned(2, s)
        return self

    def verbatim(self, data):
        write_verbatim(self.w, data)
        return self

    def command(self, value):
        self.w.unsigned(2, value)
        return self

    def quit(self):
        return finish(self.w)

    def unfinished(self):
        """the stream so far, byte-aligned, with no QUIT"""
        self.w.byte_align()
        return self.w.getvalue()


# ---------------------------------------------------------------- bit input
class EndOfStream(Exception):
    pass


class Unsupported(Exception):
    pass


class BitReader(object):
    def __init__(self, data):
        self.data = bytes(data)
        self.nbits = 8 * len(self.data)
        self.pos = 0

    def read(self, count):
        if count == 0:
            return 0
        if self.pos + count > self.nbits:
            self.pos = self.nbits
            raise EndOfStream()
        a, b = self.pos >> 3, (self.pos + count + 7) >> 3
        v = int.from_bytes(self.data[a:b], "big")
        v >>= (8 * b - self.pos - count)
        self.pos += count
        return v & ((1 << count) - 1)

    def unary(self):
        run = 0
        while True:
            if self.pos >= self.nbits:
                raise EndOfStream()
            byte = self.data[self.pos >> 3]
            rest = 8 - (self.pos & 7)
            v = byte & ((1 << rest) - 1)
            if v == 0:
                run += rest
                self.pos += rest
                continue
            lead = rest - v.bit_length()
            self.pos += lead + 1
            return run + lead

    def unsigned(self, c):
        """read_unsigned: (run << c | low), wrapped to 32 bits; c <= 32"""
        msb = self.unary()
        lsb = self.read(c)
        return ((msb << c) | lsb) & 0xFFFFFFFF

    def signed(self, c):
        u = self.unsigned(c + 1)
        return i32(-(u >> 1) - 1) if u & 1 else (u >> 1)

    def long(self):
        c = self.unsigned(2)
        if c > 32:
            raise Unsupported()
        return self.unsigned(c)


# ----------------------------------------------------------------- read_info
def ieee_extended(b):
    sign = b[0] >> 7
    exponent = ((b[0] & 0x7F) << 8) | b[1]
    mantissa = int.from_bytes(b[2:10], "big")
    if exponent == 0 and mantissa == 0:
        return 0
    if exponent == 0x7FFF:
        return 0x7FFFFFFF
    f = float(mantissa) * 2.0 ** (exponent - 16383 - 63)
    if not f < 2147483648.0:
        return 0x7FFFFFFF
    return -int(f) if sign else int(f)


WAVE_MASKS = {1: 0x4, 2: 0x3, 3: 0x7, 4: 0x33, 5: 0x37, 6: 0x3F}
SUBFORMAT_PCM = b"\x01\x00\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"


def wave_fmt(v):
    """read_wave_header -> (rate, mask) or None"""
    if len(v) < 12 or v[0:4] != b"RIFF" or v[8:12] != b"WAVE":
        return None
    p, left = 12, len(v) - 12
    while left > 0:
        if p + 8 > len(v):
            return None
        cid, size = v[p:p + 4], struct.unpack("<I", v[p + 4:p + 8])[0]
        p += 8
        left -= 8
        if cid == b"fmt ":
            if p + 16 > len(v):
                return None
            comp, ch, rate = struct.unpack("<HHI", v[p:p + 8])
            if comp == 1:
                return rate, WAVE_MASKS.get(ch, 0)
            if comp == 0xFFFE:
                if p + 40 > len(v):
                    return None
                mask = struct.unpack("<I", v[p + 20:p + 24])[0]
                return (rate, mask) if v[p + 24:p + 40] == SUBFORMAT_PCM else None
            return None
        size += size & 1
        if p + size > len(v):
            return None
        p += size
        left -= size
    return None


def aiff_comm(v):
    if len(v) < 12 or v[0:4] != b"FORM" or v[8:12] != b"AIFF":
        return None
    p, left = 12, len(v) - 12
    while left > 0:
        if p + 8 > len(v):
            return None
        cid, size = v[p:p + 4], struct.unpack(">I", v[p + 4:p + 8])[0]
        p += 8
        left -= 8
        if cid == b"COMM":
            if p + 18 > len(v):
                return None
            ch = struct.unpack(">H", v[p:p + 2])[0]
            return ieee_extended(v[p + 8:p + 18]) & 0xFFFFFFFF, {1: 0x4, 2: 0x3}.get(ch, 0)
        size += size & 1
        if p + size > len(v):
            return None
        p += size
        left -= size
    return None


def total_frames(v, channels, bps):
    """the frame count audiotools/shn.py takes from a data / SSND chunk"""
    total = 0
    per = channels * (bps // 8)
    for magic, form, end, cid_audio, sub in ((b"RIFF", b"WAVE", "<", b"data", 0),
                                             (b"FORM", b"AIFF", ">", b"SSND", 8)):
        if len(v) < 12 or v[0:4] != magic or v[8:12] != form:
            continue
        p, left = 12, len(v) - 12
        while left >= 8 and p + 8 <= len(v):
            cid, size = v[p:p + 4], struct.unpack(end + "I", v[p + 4:p + 8])[0]
            p += 8
            left -= 8
            if cid == cid_audio:
                if per and size >= sub:
                    total = (size - sub) // per
                continue
            size += size & 1
            if p + size > len(v):
                break
            p += size
            left -= size
    return total


def read_info(data):
    """read_shn_header -> (status, info dict or None)"""
    r = BitReader(data)
    try:
        magic = bytes(bytearray(r.read(8) for _ in range(4)))
        version = r.read(8)
        if magic != b"ajkg":
            return INVALID_MAGIC_NUMBER, None
        if version != 2:
            return INVALID_SHORTEN_VERSION, None
        ftype, channels, block, max_lpc, means, skip = [r.long() for _ in range(6)]
        r.read(0)
        if r.pos + 8 * skip > r.nbits:
            return IOERROR, None
        r.pos += 8 * skip
        if 1 <= ftype <= 2:
            bps, signed = 8, ftype == 1
        elif 3 <= ftype <= 6:
            bps, signed = 16, ftype in (3, 5)
        else:
            return UNSUPPORTED_FILE_TYPE, None
        info = dict(file_type=ftype, channels=channels, block_length=block, max_lpc=max_lpc,
                    mean_count=means, bytes_to_skip=skip, bits_per_sample=bps,
                    signed_samples=int(signed), sample_rate=44100, channel_mask=0,
                    total_pcm_frames=0, first_command_bit=r.pos)
        if r.unsigned(2) == FN_VERBATIM:
            v = bytes(bytearray(r.unsigned(8) & 0xFF for _ in range(r.unsigned(5))))
            got = wave_fmt(v) or aiff_comm(v)
            if got:
                info["sample_rate"], info["channel_mask"] = got
            info["total_pcm_frames"] = total_frames(v, channels, bps)
        return OK, info
    except EndOfStream:
        return IOERROR, None
    except Unsupported:
        return UNSUPPORTED, None


# ------------------------------------------------------------------- decoder
def shnmean(values):
    return cdiv(i32(len(values) // 2 + sum(values)), len(values))


def decode(data):
    """-> (status, pcm int32 interleaved, info, header bytes, footer bytes).
    status is END_OF_STREAM for a stream that ended with QUIT; the PCM of any
    other ends before the first incomplete set of channels."""
    status, info = read_info(data)
    empty = np.zeros(0, dtype=np.int32)
    if status != OK:
        return status, empty, info, b"", b""
    C, K = info["channels"], max(3, info["max_lpc"])
    mc = info["mean_count"]
    if C < 1 or C > MAX_CHANNELS or mc > MAX_MEAN_COUNT:
        return UNSUPPORTED, empty, info, b"", b""
    adjust = 0 if info["signed_samples"] else 1 << (info["bits_per_sample"] - 1)
    r = BitReader(data)
    r.pos = info["first_command_bit"]
    L = info["block_length"]
    shift = 0
    means = [[0] * mc for _ in range(C)]
    prev = [[] for _ in range(C)]
    out, cur = [], []
    frames = 0
    head, foot, seen_audio = bytearray(), bytearray(), False
    c = 0
    try:
        while True:
            cmd = r.unsigned(2)
            if cmd <= FN_DIFF3 or cmd in (FN_QLPC, FN_ZERO):
                if L == 0 or (cmd in (FN_DIFF0, FN_QLPC) and mc == 0):
                    raise Unsupported()
                if c and L != len(cur[0]):
                    raise Unsupported()
                if (frames + L) * C > MAX_TRACK_SAMPLES:
                    raise Unsupported()
                seen_audio = True
                if cmd == FN_ZERO:
                    s = [0] * L
                else:
                    energy = r.unsigned(3)
                    if energy > 31:
                        raise Unsupported()
                    if cmd == FN_DIFF0:
                        off = shnmean(means[c])
                        s = [i32(r.signed(energy) + off) for _ in range(L)]
                    elif cmd == FN_QLPC:
                        off = shnmean(means[c])
                        n = r.unsigned(2)
                        if n > MAX_LPC_COUNT:
                            raise Unsupported()
                        coeff = [r.signed(5) for _ in range(n)]
                        p = prev[c]
                        h = [0] * (n - len(p)) + p if len(p) < n else p[len(p) - n:]
                        u = [i32(v - off) for v in h]
                        for i in range(L):
                            res = r.signed(energy)
                            acc = 32
                            for j in range(n):
                                acc = i32(acc + i32(coeff[j] * u[n + i - j - 1]))
                            u.append(i32((acc >> 5) + res))
                        s = [i32(v + off) for v in u[n:]]
                    else:
                        h = [0] * (cmd - len(prev[c])) + prev[c] if len(prev[c]) < cmd \
                            else prev[c][-cmd:]
                        s = list(h)
                        for i in range(L):
                            res = r.signed(energy)
                            if cmd == 1:
                                v = s[-1] + res
                            elif cmd == 2:
                                v = 2 * s[-1] - s[-2] + res
                            else:
                                v = 3 * (s[-1] - s[-2]) + s[-3] + res
                            s.append(i32(v))
                        s = s[cmd:]
                if mc:
                    means[c] = (means[c] + [shnmean(s)])[-mc:]
                prev[c] = s[-K:]
                cur.append([i32(i32(v << shift) - adjust) for v in s])
                c += 1
                if c == C:
                    out.append(np.array(cur, dtype=np.int64).T.reshape(-1))
                    frames += L
                    cur, c = [], 0
            elif cmd == FN_QUIT:
                status = END_OF_STREAM
                break
            elif cmd == FN_BLOCKSIZE:
                L = r.long()
            elif cmd == FN_BITSHIFT:
                shift = r.unsigned(2)
                if shift > 31:
                    raise Unsupported()
            elif cmd == FN_VERBATIM:
                dst = foot if seen_audio else head
                for _ in range(r.unsigned(5)):
                    dst.append(r.unsigned(8) & 0xFF)
            else:
                status = UNKNOWN_COMMAND
                break
    except EndOfStream:
        status = IOERROR
    except Unsupported:
        status = UNSUPPORTED
    pcm = np.concatenate(out).astype(np.int32) if out else empty
    return status, pcm, info, bytes(head), bytes(foot)


def pcm_split(data):
    """SHNDecoder.pcm_split(): (bytes in front of the audio, bytes after it);
    IOError unless the walk reaches QUIT"""
    status, _, _, head, foot = decode(data)
    if status != END_OF_STREAM:
        raise IOError("I/O error reading Shorten file")
    return head, foot
