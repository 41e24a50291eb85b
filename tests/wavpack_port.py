"""Plain-Python restatement of the WavPack decoder (reference
src/decoders/wavpack.c), used by the tests as a checker only.

It follows the order of checks of WavPackDecoder_init, the read loop of the
standalone main and decode_block, so that a damaged stream ends with the same
status after the same number of PCM frames.  Arithmetic is done in Python
integers and wrapped to 32 bits where C's int would be; shift counts that C
leaves undefined (beyond 31) are masked to five bits, and a 1 << 32 is 0.

  read_info(data)  -> (status, info dict, sets, end status): the block table
                      with the host layout checks of the GPU decoder
                      (INCONSISTENT_BLOCK)
  decode(data)     -> (status, info, interleaved PCM list, frames per set)
  seek_position(data, offset) -> (PCM offset, byte offset) WavPackDecoder_seek
                      lands on
"""
import hashlib
import struct

(OK, IO_ERROR, SUB_BLOCK_NOT_FOUND, INVALID_BLOCK_ID, INVALID_RESERVED_BIT,
 EXCESSIVE_DECORRELATION_PASSES, INVALID_DECORRELATION_TERM, DECORRELATION_TERMS_MISSING,
 DECORRELATION_WEIGHTS_MISSING, DECORRELATION_SAMPLES_MISSING, ENTROPY_VARIABLES_MISSING,
 RESIDUALS_MISSING, EXTENDED_INTEGERS_MISSING, EXCESSIVE_DECORRELATION_WEIGHTS,
 INVALID_ENTROPY_VARIABLE_COUNT, BLOCK_DATA_CRC_MISMATCH, BLOCK_DATA_IO, INCONSISTENT_BLOCK,
 MD5_MISMATCH, SAMPLE_RATE_UNDEFINED, CHANNELS_UNDEFINED) = range(21)

# what wvdec prints for a status that ends a stream
MESSAGES = {
    IO_ERROR: "I/O error", INVALID_BLOCK_ID: "invalid block header ID",
    INVALID_RESERVED_BIT: "invalid reserved bit",
    EXCESSIVE_DECORRELATION_PASSES: "excessive decorrelation passes",
    INVALID_DECORRELATION_TERM: "invalid decorrelation term",
    DECORRELATION_TERMS_MISSING: "missing decorrelation terms sub block",
    DECORRELATION_WEIGHTS_MISSING: "missing decorrelation weights sub block",
    DECORRELATION_SAMPLES_MISSING: "missing decorrelation samples sub block",
    ENTROPY_VARIABLES_MISSING: "missing entropy variables sub block",
    RESIDUALS_MISSING: "missing bitstream sub block",
    EXTENDED_INTEGERS_MISSING: "missing extended integers sub block",
    EXCESSIVE_DECORRELATION_WEIGHTS: "excessive decorrelation weight values",
    INVALID_ENTROPY_VARIABLE_COUNT: "invalid entropy variable count",
    BLOCK_DATA_CRC_MISMATCH: "block data CRC mismatch",
    BLOCK_DATA_IO: "I/O error reading block data",
    MD5_MISMATCH: "MD5 mismatch at end of stream",
}

RATES = (6000, 8000, 9600, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 64000,
         88200, 96000, 192000)
EXP2 = [int(256 * 2.0 ** (i / 256.0) + 0.5) for i in range(256)]
M32 = 0xFFFFFFFF


def s32(v):
    v &= M32
    return v - (1 << 32) if v & 0x80000000 else v


def s8(v):
    return v - 256 if v & 0x80 else v


def wv_exp2(value):
    """read_wv_exp2 on a signed 16-bit value"""
    if value < 0:
        return s32(-wv_exp2_pos(-value))
    return wv_exp2_pos(value)


def wv_exp2_pos(v):
    e = EXP2[v & 0xFF]
    if v <= 2304:
        return e >> (9 - (v >> 8))
    return s32(e << (((v >> 8) - 9) & 31))


def parse_header(data, pos):
    """read_block_header -> (status, dict)"""
    if len(data) - pos < 32:
        return IO_ERROR, None
    (bid, size, version, track, index, total, bindex, bsamples, flags, crc) = struct.unpack(
        "<4sIHBBIIIII", data[pos:pos + 32])
    h = {"block_size": size, "version": version, "total_samples": total,
         "block_index": bindex, "block_samples": bsamples, "flags": flags, "crc": crc,
         "bits_code": flags & 3, "mono": (flags >> 2) & 1, "joint": (flags >> 4) & 1,
         "extended": (flags >> 8) & 1, "initial": (flags >> 11) & 1,
         "final": (flags >> 12) & 1, "rate_code": (flags >> 23) & 15,
         "false_stereo": (flags >> 30) & 1, "offset": pos}
    h["coded"] = 1 if (h["mono"] or h["false_stereo"]) else 2
    h["out"] = 1 if (h["mono"] and not h["false_stereo"]) else 2
    if bid != b"wvpk":
        return INVALID_BLOCK_ID, h
    if flags >> 31:
        return INVALID_RESERVED_BIT, h
    return OK, h


def sub_blocks(data):
    """read_sub_block over a block's data: yields (function, nondecoder,
    payload bytes, one_less) and finally None on an I/O error"""
    pos, left = 0, len(data)
    while left > 0:
        if len(data) - pos < 2:
            yield None
            return
        b = data[pos]
        large = b >> 7
        hdr = 4 if large else 2
        if len(data) - pos < hdr:
            yield None
            return
        size = data[pos + 1] if not large else \
            data[pos + 1] | (data[pos + 2] << 8) | (data[pos + 3] << 16)
        one_less = (b >> 6) & 1
        if one_less and size == 0:
            yield None
            return
        if len(data) - pos - hdr < size * 2:
            yield None
            return
        payload = data[pos + hdr:pos + hdr + size * 2 - one_less]
        yield (b & 31, (b >> 5) & 1, payload, one_less, size)
        pos += hdr + size * 2
        left -= hdr + size * 2


def find_sub_block(data, pos, h, function, nondecoder):
    n = (h["block_size"] - 24) & M32
    if len(data) - (pos + 32) < n:
        return IO_ERROR, None
    for sb in sub_blocks(data[pos + 32:pos + 32 + n]):
        if sb is None:
            return IO_ERROR, None
        if sb[0] == function and sb[1] == nondecoder:
            return OK, sb[2]
    return SUB_BLOCK_NOT_FOUND, None


def read_info(data, start=0):
    """-> (init status, info, sets, end status).  sets: list of lists of block
    headers, complete and consistent; end status is what stops the stream after
    them (OK at the declared total), end_blocks the readable blocks of the
    set it stopped in (decoded for their status only)"""
    data = bytes(data)
    st, h = parse_header(data, 0)
    if st:
        return st, None, [], st
    info = {"md5": None}
    rate = RATES[h["rate_code"]] if h["rate_code"] < 15 else 0
    if rate == 0:
        st, p = find_sub_block(data, 0, h, 7, 1)
        if st == SUB_BLOCK_NOT_FOUND:
            return SAMPLE_RATE_UNDEFINED, None, [], st
        if st:
            return st, None, [], st
        rate = int.from_bytes(p[:4], "little")
    info["sample_rate"] = rate
    info["bits_per_sample"] = (8, 16, 24, 32)[h["bits_code"]]
    if h["final"]:
        info["channels"], info["channel_mask"] = (2, 3) if h["out"] == 2 else (1, 4)
    else:
        st, p = find_sub_block(data, 0, h, 13, 0)
        if st == SUB_BLOCK_NOT_FOUND:
            return CHANNELS_UNDEFINED, None, [], st
        if st:
            return st, None, [], st
        if len(p) < 2:
            return IO_ERROR, None, [], IO_ERROR
        info["channels"] = p[0]
        if p[0] == 0:
            return CHANNELS_UNDEFINED, None, [], CHANNELS_UNDEFINED
        info["channel_mask"] = int.from_bytes(p[1:5], "little")
    info["total_pcm_frames"] = h["total_samples"]
    sets, end, pos, tail = walk_sets(data, info, start, None)
    info["end_blocks"] = tail
    info["end_offset"] = pos
    if end == OK:
        st, h = parse_header(data, pos)
        if st == OK:
            st, p = find_sub_block(data, pos, h, 6, 1)
            if st == OK and len(p) == 16:
                info["md5"] = bytes(p)
    return OK, info, sets, end


def walk_sets(data, info, pos, expected):
    remaining = info["total_pcm_frames"]
    if expected is not None:
        remaining -= min(remaining, expected)
    sets = []
    while remaining > 0:
        blocks, chans, p = [], 0, pos
        while True:
            st, h = parse_header(data, p)
            if st:
                return sets, st, pos, blocks
            if not blocks:
                if expected is None:      # the stream's first block: any index
                    expected = h["block_index"]
                if h["block_index"] != expected or h["block_samples"] > remaining or \
                        h["block_samples"] > 0x7FFFFFFF:
                    return sets, INCONSISTENT_BLOCK, pos, []
            elif h["block_samples"] != blocks[0]["block_samples"]:
                return sets, INCONSISTENT_BLOCK, pos, []
            chans += h["out"]
            if chans > info["channels"]:
                return sets, INCONSISTENT_BLOCK, pos, []
            n = (h["block_size"] - 24) & M32
            if len(data) - (p + 32) < n:
                return sets, BLOCK_DATA_IO, pos, blocks
            h["data"] = (p + 32, n)
            h["first_channel"] = chans - h["out"]
            blocks.append(h)
            p += 32 + n
            if h["final"]:
                break
        if chans != info["channels"]:
            return sets, INCONSISTENT_BLOCK, pos, []
        sets.append(blocks)
        pos = p
        expected = (expected + blocks[0]["block_samples"]) & M32
        remaining -= min(remaining, blocks[0]["block_samples"])
    return sets, OK, pos, []


class Bits(object):
    def __init__(self, data):
        self.v = int.from_bytes(data, "little")
        self.n = len(data) * 8

    def read(self, k):
        if k > self.n:
            raise EOFError
        r = self.v & ((1 << k) - 1)
        self.v >>= k
        self.n -= k
        return r

    def unary(self):
        c = 0
        while True:
            if self.n == 0:
                raise EOFError
            b = self.v & 1
            self.v >>= 1
            self.n -= 1
            if not b:
                return c
            c += 1


def read_egc(bs):
    t = bs.unary()
    if t > 1:
        if t > 32:
            raise EOFError
        return ((1 << (t - 1)) + bs.read(t - 1)) & M32
    return t


def read_residual(bs, state, e):
    last = state[0]
    if last < 0 or last % 2:
        u = bs.unary()
        if u == 16:
            u = (u + read_egc(bs)) & M32
        m = u // 2 + (0 if last < 0 else 1)
        state[0] = u & 0x7FFFFFFF
    else:
        state[0] = -1
        m = 0
    if m == 0:
        base = 0
        add = e[0] >> 4
        e[0] = s32(e[0] - (s32(e[0] + 126) >> 7) * 2)
    elif m == 1:
        base = (e[0] >> 4) + 1
        add = e[1] >> 4
        e[0] = s32(e[0] + (s32(e[0] + 128) >> 7) * 5)
        e[1] = s32(e[1] - (s32(e[1] + 62) >> 6) * 2)
    elif m == 2:
        base = (e[0] >> 4) + 1 + (e[1] >> 4) + 1
        add = e[2] >> 4
        e[0] = s32(e[0] + (s32(e[0] + 128) >> 7) * 5)
        e[1] = s32(e[1] + (s32(e[1] + 64) >> 6) * 5)
        e[2] = s32(e[2] - (s32(e[2] + 30) >> 5) * 2)
    else:
        base = (e[0] >> 4) + 1 + (e[1] >> 4) + 1 + ((e[2] >> 4) + 1) * (m - 2)
        add = e[2] >> 4
        e[0] = s32(e[0] + (s32(e[0] + 128) >> 7) * 5)
        e[1] = s32(e[1] + (s32(e[1] + 64) >> 6) * 5)
        e[2] = s32(e[2] + (s32(e[2] + 32) >> 5) * 5)
    base &= M32
    if add == 0:
        u = base
    else:
        p = (add & M32).bit_length() - 1
        ee = ((1 << (p + 1)) - add - 1) & M32
        r = bs.read(p)
        if r >= ee:
            u = (base + r * 2 - ee + bs.read(1)) & M32
        else:
            u = (base + r) & M32
    if bs.read(1):
        return s32(~u)
    return s32(u)


def read_bitstream(payload, n, coded, ent):
    res = [[0] * n for _ in range(coded)]
    bs = Bits(payload)
    state = [-1]
    total = coded * n
    i = 0
    try:
        while i < total:
            if state[0] < 0 and ent[0][0] < 2 and ent[1][0] < 2:
                zeroes = read_egc(bs)
                if zeroes > 0:
                    zeroes = min(zeroes, total - i)
                    i += zeroes          # already 0
                    ent[0][:] = [0, 0, 0]
                    ent[1][:] = [0, 0, 0]
                if i < total:
                    res[i % coded][i // coded] = read_residual(bs, state, ent[i % coded])
                    i += 1
            else:
                res[i % coded][i // coded] = read_residual(bs, state, ent[i % coded])
                i += 1
    except EOFError:
        return IO_ERROR, None
    return OK, res


def apply_weight(w, s):
    return s32((w * s + 512) >> 10)


def update_weight(src, res, delta):
    if src == 0 or res == 0:
        return 0
    return delta if (src ^ res) >= 0 else -delta


def clamp(w):
    return max(min(w, 1024), -1024)


def pass_1ch(term, delta, w, hist, x):
    """hist: the samples before the block, oldest first (1..8) or as stored
    (17, 18: [newest, older])"""
    out = []
    if term in (17, 18):
        a, b = hist[0], hist[1]      # out[i-1], out[i-2]
        for v in x:
            t = 2 * a - b if term == 17 else (3 * a - b) >> 1
            o = s32(apply_weight(w, t) + v)
            w = s32(w + update_weight(t, v, delta))
            a, b = o, a
            out.append(o)
    else:
        h = list(hist)
        for i, v in enumerate(x):
            t = h[i]
            o = s32(apply_weight(w, t) + v)
            w = s32(w + update_weight(t, v, delta))
            h.append(o)
            out.append(o)
    return out


def pass_2ch(term, delta, w0, w1, h0, h1, x0, x1):
    if term > 0:
        return pass_1ch(term, delta, w0, h0, x0), pass_1ch(term, delta, w1, h1, x1)
    p0, p1 = h1[0], h0[0]       # out0[i-1], out1[i-1]
    o0, o1 = [], []
    for a, b in zip(x0, x1):
        if term == -1:
            n0 = s32(apply_weight(w0, p1) + a)
            n1 = s32(apply_weight(w1, n0) + b)
            w0 = clamp(w0 + update_weight(p1, a, delta))
            w1 = clamp(w1 + update_weight(n0, b, delta))
        elif term == -2:
            n1 = s32(apply_weight(w1, p0) + b)
            n0 = s32(apply_weight(w0, n1) + a)
            w1 = clamp(w1 + update_weight(p0, b, delta))
            w0 = clamp(w0 + update_weight(n1, a, delta))
        else:
            n0 = s32(apply_weight(w0, p1) + a)
            n1 = s32(apply_weight(w1, p0) + b)
            w0 = clamp(w0 + update_weight(p1, a, delta))
            w1 = clamp(w1 + update_weight(p0, b, delta))
        p0, p1 = n0, n1
        o0.append(n0)
        o1.append(n1)
    return o0, o1


def restore_weight(v):
    v = s8(v)
    if v > 0:
        return (v << 3) + (((v << 3) + 64) >> 7)
    return v << 3


def decode_block(data, h):
    """decode_block -> (status, list of output channels)"""
    off, size = h["data"]
    coded, n = h["coded"], h["block_samples"]
    terms = None            # file order: (term, delta)
    weights = samples = ent = ext = res = None
    for sb in sub_blocks(data[off:off + size]):
        if sb is None:
            return IO_ERROR, None
        fn, nondec, p, one_less, size_words = sb
        if nondec:
            continue
        if fn == 2:
            if len(p) > 16:
                return EXCESSIVE_DECORRELATION_PASSES, None
            terms = []
            for b in p:
                t = (b & 31) - 5
                terms.append((t, b >> 5))
                if not (-3 <= t <= -1 or 1 <= t <= 8 or 17 <= t <= 18):
                    return INVALID_DECORRELATION_TERM, None
            weights = samples = None
        elif fn == 3:
            if terms is None:
                return DECORRELATION_TERMS_MISSING, None
            cnt = len(p) // coded
            if cnt > len(terms):
                return EXCESSIVE_DECORRELATION_WEIGHTS, None
            weights = [[0, 0] for _ in terms]
            for i in range(cnt):
                for c in range(coded):
                    weights[i][c] = restore_weight(p[i * coded + c])
        elif fn == 4:
            if terms is None:
                return DECORRELATION_TERMS_MISSING, None
            left, q = len(p), 0
            samples = []
            for t, _ in terms:
                if t < 0 and coded == 1:
                    return INVALID_DECORRELATION_TERM, None
                cnt = 2 if t > 8 else (t if t > 0 else 1)
                hs = [[0] * cnt for _ in range(2)]
                if left >= cnt * 2 * coded:
                    vals = [wv_exp2(struct.unpack_from("<h", p, q + 2 * k)[0])
                            for k in range(cnt * coded)]
                    q += cnt * 2 * coded
                    left -= cnt * 2 * coded
                    if t > 8:       # channel 0's two, then channel 1's
                        for c in range(coded):
                            hs[c] = vals[2 * c:2 * c + 2]
                    else:
                        for k in range(cnt):
                            for c in range(coded):
                                hs[c][k] = vals[k * coded + c]
                else:
                    left = 0
                samples.append(hs)
        elif fn == 5:
            if one_less or size_words != 3 * coded:
                return INVALID_ENTROPY_VARIABLE_COUNT, None
            v = [wv_exp2(x) for x in struct.unpack("<%dh" % (3 * coded), p)]
            ent = [v[0:3], v[3:6] if coded == 2 else [0, 0, 0]]
        elif fn == 9:
            if len(p) != 4:
                return IO_ERROR, None
            ext = tuple(p)
        elif fn == 10:
            if ent is None:
                return ENTROPY_VARIABLES_MISSING, None
            st, res = read_bitstream(p, n, coded, ent)
            if st:
                return st, None
    if terms is not None:
        if weights is None:
            return DECORRELATION_WEIGHTS_MISSING, None
        if samples is None:
            return DECORRELATION_SAMPLES_MISSING, None
    if res is None:
        return RESIDUALS_MISSING, None
    ch = res
    if terms:
        for k in range(len(terms) - 1, -1, -1):
            t, d = terms[k]
            if coded == 1:
                ch = [pass_1ch(t, d, weights[k][0], samples[k][0], ch[0])]
            else:
                ch = list(pass_2ch(t, d, weights[k][0], weights[k][1], samples[k][0],
                                   samples[k][1], ch[0], ch[1]))
    if coded == 2 and h["joint"]:
        right = [s32(s - (m >> 1)) for m, s in zip(ch[0], ch[1])]
        left = [s32(m + r) for m, r in zip(ch[0], right)]
        ch = [left, right]
    crc = M32
    if coded == 2:
        for a, b in zip(ch[0], ch[1]):
            crc = (3 * crc + a) & M32
            crc = (3 * crc + b) & M32
    else:
        for a in ch[0]:
            crc = (3 * crc + a) & M32
    if crc != h["crc"]:
        return BLOCK_DATA_CRC_MISMATCH, None
    if h["extended"]:
        if ext is None:
            return EXTENDED_INTEGERS_MISSING, None
        _, zb, ob, db = ext
        if zb:
            ch = [[s32(v << (zb & 31)) for v in c] for c in ch]
        elif ob:
            ch = [[s32((v << (ob & 31)) | ((1 << (ob & 31)) - 1)) for v in c] for c in ch]
        elif db:
            k = db & 31
            ch = [[s32((v << k) | (((1 << k) - 1) if v & 1 else 0)) for v in c] for c in ch]
    if h["false_stereo"]:
        ch = [ch[0], ch[0]]
    return OK, ch


def pcm_bytes(samples, bits_per_sample):
    """the file byte form wvdec writes and hashes: clamped to the width,
    little endian, signed at every width"""
    bb = bits_per_sample // 8
    hi = (1 << (bits_per_sample - 1)) - 1
    return b"".join((max(min(s, hi), -hi - 1) & ((1 << (8 * bb)) - 1)).to_bytes(bb, "little")
                    for s in samples)


def decode(data):
    """-> (status, info, interleaved PCM, frames per decoded set)"""
    data = bytes(data)
    st, info, sets, end = read_info(data)
    if st:
        return st, None, [], []
    pcm, counts = [], []
    C = info["channels"]
    for blocks in sets:
        chans = []
        for h in blocks:
            st, ch = decode_block(data, h)
            if st:
                return st, info, pcm, counts
            chans.extend(ch)
        n = blocks[0]["block_samples"]
        for i in range(n):
            for c in range(C):
                pcm.append(chans[c][i])
        counts.append(n)
    for h in info["end_blocks"]:      # the readable blocks of the set that failed
        st, _ = decode_block(data, h)
        if st:
            return st, info, pcm, counts
    if end == OK and info["md5"] is not None:
        if hashlib.md5(pcm_bytes(pcm, info["bits_per_sample"])).digest() != info["md5"]:
            return MD5_MISMATCH, info, pcm, counts
    return end, info, pcm, counts


def seek_position(data, offset):
    """WavPackDecoder_seek: the latest initial block with samples whose index
    is <= offset -> (its block_index, its byte offset)"""
    pos, best, best_pos = 0, 0, 0
    while True:
        st, h = parse_header(data, pos)
        if st:
            break
        if h["initial"] and h["block_samples"]:
            if h["block_index"] > offset:
                break
            best, best_pos = h["block_index"], pos
        pos += 8 + h["block_size"]
    return best, best_pos
