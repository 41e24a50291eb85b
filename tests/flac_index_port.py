"""Python restatement of the FLAC frame index's listing rule
(include/atgpu_flac_index.h, csrc/flac_index.hip), written from the rule and
not from the kernels.

A position p of a range is listed when
  - a frame header parses at p inside the range, passes CRC-8 and agrees with
    the range's STREAMINFO (rate, channels, bits per sample, block size <=
    max_block_size), read as the decoder reads it: the reserved bit after the
    sample size and the form of the number's continuation bytes unchecked;
  - for some later such header q of the range, or q = the range's end, with
    9 <= q - p <= frame_bound(), the bytes [p, q) leave a zero CRC-16 residue;
  - where q is a header, it has p's blocking strategy and its number follows
    p's: frame number + 1, or sample number + p's block size.
An entry is (byte_offset from the range's start, first_sample, block_size);
first_sample is the sample number, or the frame number times the STREAMINFO
block size (min_block_size, max_block_size where that is 0) for fixed
blocking."""
import bisect
import collections

import numpy as np

MIN_FRAME = 9
MAX_FRAME = 1 << 22

Info = collections.namedtuple("Info", "sample_rate channels bits_per_sample max_block_size "
                              "min_block_size")


def info_of(si):
    """Info from anything with STREAMINFO's field names"""
    return Info(*(int(getattr(si, f)) for f in Info._fields))


def _table(width, poly):
    top, mask = 1 << (width - 1), (1 << width) - 1
    out = []
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly if c & top else c << 1) & mask
        out.append(c)
    return out


CRC8 = _table(8, 0x07)
CRC16 = _table(16, 0x8005)
RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000,
         9: 44100, 10: 48000, 11: 96000}
SIZES = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24}


def crc16(data, crc=0):
    for b in data:
        crc = ((crc << 8) & 0xFFFF) ^ CRC16[(crc >> 8) ^ b]
    return crc


def frame_bound(info):
    sub = (info.max_block_size * (info.bits_per_sample + 1) + 7) // 8 + 8
    return min(MAX_FRAME, 64 + 2 * info.channels * sub)


def parse_header(data, p, end, info):
    """-> (variable, number, block_size) of a sound header at p whose bytes end
    at or before `end`, else None"""
    def byte(i):
        if p + i >= end:
            raise IndexError
        return data[p + i]

    try:
        if byte(0) != 0xFF or byte(1) & 0xFE != 0xF8:
            return None
        variable = byte(1) & 1
        bs_bits, sr_bits = byte(2) >> 4, byte(2) & 15
        assign = byte(3) >> 4
        channels = 2 if 8 <= assign <= 10 else assign + 1
        size_bits = (byte(3) >> 1) & 7
        if size_bits in (3, 7):
            return None
        bps = SIZES.get(size_bits, info.bits_per_sample)
        first = byte(4)
        ones = 0
        while ones < 8 and first & (0x80 >> ones):
            ones += 1
        if ones > 7:
            return None
        number = first & (0x7F >> ones)
        n = 5
        for _ in range(1, ones):
            number = (number << 6) | (byte(n) & 0x3F)
            n += 1
        if bs_bits == 0:
            bs = info.max_block_size
        elif bs_bits == 1:
            bs = 192
        elif bs_bits <= 5:
            bs = 576 << (bs_bits - 2)
        elif bs_bits == 6:
            bs = byte(n) + 1
            n += 1
        elif bs_bits == 7:
            bs = ((byte(n) << 8) | byte(n + 1)) + 1
            n += 2
        else:
            bs = 256 << (bs_bits - 8)
        if sr_bits == 0:
            rate = info.sample_rate
        elif sr_bits in RATES:
            rate = RATES[sr_bits]
        elif sr_bits == 12:
            rate = byte(n) * 1000
            n += 1
        elif sr_bits == 13:
            rate = (byte(n) << 8) | byte(n + 1)
            n += 2
        elif sr_bits == 14:
            rate = ((byte(n) << 8) | byte(n + 1)) * 10
            n += 2
        else:
            return None
        byte(n)
        n += 1
    except IndexError:
        return None
    crc = 0
    for b in data[p:p + n]:
        crc = CRC8[crc ^ b]
    if crc or (rate, channels, bps) != (info.sample_rate, info.channels, info.bits_per_sample):
        return None
    if bs > info.max_block_size:
        return None
    return variable, number, bs


def candidates(data, start, end, info):
    """{position: header} of every sound header of data[start:end]"""
    a = np.frombuffer(data, dtype=np.uint8)[start:end]
    if len(a) < 2:
        return {}
    hits = np.nonzero((a[:-1] == 0xFF) & ((a[1:] & 0xFE) == 0xF8))[0]
    out = {}
    for h in hits.tolist():
        hdr = parse_header(data, start + h, end, info)
        if hdr:
            out[start + h] = hdr
    return out


def index_range(data, start, nbytes, info):
    """the entries of one range: [(byte_offset, first_sample, block_size)]"""
    info = info_of(info)
    end = start + nbytes
    cand = candidates(data, start, end, info)
    pos = sorted(cand)
    bound = frame_bound(info)
    fixed_bs = info.min_block_size or info.max_block_size
    out = []
    for k, p in enumerate(pos):
        variable, number, bs = cand[p]
        crc, prev, listed = 0, p, False
        for q in pos[k + 1:] + [end]:
            if q - p > bound:
                break
            crc = crc16(data[prev:q], crc)
            prev = q
            if crc or q - p < MIN_FRAME:
                continue
            if q == end:
                listed = True
            else:
                qv, qn, _ = cand[q]
                listed = qv == variable and qn == number + (bs if variable else 1)
            if listed:
                break
        if listed:
            out.append((p - start, number if variable else number * fixed_bs, bs))
    return out


def index_ranges(data, ranges):
    """ranges: [(start, nbytes, info)] -> [(range, byte_offset, first_sample,
    block_size)] sorted by (range, byte_offset), as the library returns them"""
    out = []
    for r, (start, nbytes, info) in enumerate(ranges):
        out += [(r,) + e for e in index_range(data, start, nbytes, info)]
    return out


def first_at_or_before(entries, sample):
    """the last entry with first_sample <= sample, or None (entries ascend)"""
    k = bisect.bisect_right([e[1] for e in entries], sample)
    return entries[k - 1] if k else None
