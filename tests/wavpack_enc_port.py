"""Plain-Python restatement of the WavPack encoder (reference
src/encoders/wavpack.c), used by the tests as a checker only.

The serial unit is the stream: one track's sequence of blocks for one channel
group (init_context).  Weights, history samples and medians are carried from
block to block and round-tripped through their stored forms at every
boundary; where the effective channel count changes (false stereo toggling)
they are reset.  Sums wrap at 32 bits where C's int would overflow and
apply_weight multiplies in 64 bits, as csrc/wavpack_common.h defines them.

  encode(samples, channels, mask, bps, rate, block_size, passes, joint, false,
         wasted, total_pcm_frames=0) -> bytes   the complete .wv image
  parse_options(wvenc option list) -> dict of encode()'s keyword arguments
"""
import hashlib
import math
import struct

from wavpack_port import M32, RATES, apply_weight, s32, update_weight, wv_exp2

WLOG = [int(256 * math.log2(1 + i / 256.0) + 0.5) for i in range(256)]

TERMS_1CH = {0: (), 1: (18,), 2: (17, 18), 5: (3, 17, 2, 18, 18)}
TERMS_1CH[10] = TERMS_1CH[16] = TERMS_1CH[5]
TERMS_2CH = {0: (), 1: (18,), 2: (17, 18), 5: (3, 17, 2, 18, 18),
             10: (4, 17, -1, 5, 3, 2, -2, 18, 18, 18),
             16: (2, 18, -1, 8, 6, 3, 5, 7, 4, 2, 18, -2, 3, 2, 18, 18)}
SPLITS = {0x7: (2, 1), 0x33: (2, 2), 0x107: (2, 1, 1), 0x37: (2, 1, 2), 0x3F: (2, 1, 1, 2)}
DELTA = 2


def stream_channels(channels, mask):
    if channels <= 2:
        return (channels,)
    return SPLITS.get(mask, (1,) * channels)


def min_block_size(channels, mask, passes):
    """the deepest history of any stream's table (terms 17 and 18 keep two
    samples).  The reference aborts on a non-final block shorter than its
    deepest term 1..8; block sizes below this depth are refused outright"""
    depth = 0
    for c in stream_channels(channels, mask):
        table = (TERMS_1CH if c == 1 else TERMS_2CH)[passes]
        depth = max([depth] + [min(t, 2) if t > 8 else t for t in table if t > 0])
    return depth


def wv_log2(value):
    a = (abs(value) + (abs(value) >> 9)) & M32
    c = a.bit_length()
    if a < 256:
        r = (c << 8) + WLOG[(a << (9 - c)) % 256]
    else:
        r = (c << 8) + WLOG[(a >> (c - 9)) % 256]
    return r if value >= 0 else -r


def store_weight(w):
    w = min(max(w, -1024), 1024)
    if w > 0:
        return (w - ((w + 64) >> 7) + 4) >> 3
    return (w + 4) >> 3 if w else 0


def restore_weight(v):
    if v > 0:
        return (v << 3) + (((v << 3) + 64) >> 7)
    return v << 3


def roundtrip(v):
    return wv_exp2(wv_log2(v))


class BitWriter(object):
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.fill = 0

    def write(self, nbits, value):
        self.acc |= (value & ((1 << nbits) - 1)) << self.fill
        self.fill += nbits
        if self.fill >= 256:
            k = self.fill // 8
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.fill -= 8 * k

    def unary(self, v):
        """v one-bits and a zero"""
        self.write(v + 1, (1 << v) - 1)

    def bytes(self):
        k = (self.fill + 7) // 8
        return bytes(self.out) + self.acc.to_bytes(k, "little")


def write_egc(bw, v):
    if v <= 1:
        bw.unary(v)
    else:
        t = v.bit_length()
        bw.unary(t)
        bw.write(t - 1, v % (1 << (t - 1)))


class Stream(object):
    """encoding_parameters of one channel group"""

    def __init__(self, channels, passes):
        self.channels = channels
        self.passes = passes
        self.reset(channels)

    def reset(self, effective):
        self.effective = effective
        self.terms = list((TERMS_1CH if effective == 1 else TERMS_2CH)[self.passes])
        self.weights = [[0] * effective for _ in self.terms]
        self.samples = [[[0] * (2 if t > 8 else (t if t > 0 else 1)) for _ in range(effective)]
                        for t in self.terms]
        self.entropies = [[0, 0, 0], [0, 0, 0]]

    def roundtrip(self):
        for w in self.weights:
            w[:] = [restore_weight(store_weight(v)) for v in w]
        for sp in self.samples:
            for sc in sp:
                sc[:] = [roundtrip(v) for v in sc]
        for c in range(self.effective):
            self.entropies[c] = [roundtrip(v) for v in self.entropies[c]]


def correlate_1ch(x, term, delta, weight, samples):
    """-> (correlated, weight); samples is updated for the next block"""
    out = []
    if term in (17, 18):
        a, b = samples[0], samples[1]          # x[i-1], x[i-2]
        for v in x:
            t = s32(2 * a - b) if term == 17 else s32(3 * a - b) >> 1
            r = s32(v - apply_weight(weight, t))
            weight = s32(weight + update_weight(t, r, delta))
            out.append(r)
            a, b = v, a
        samples[0], samples[1] = a, b
    else:
        u = list(samples) + list(x)
        for i in range(term, len(u)):
            r = s32(u[i] - apply_weight(weight, u[i - term]))
            weight = s32(weight + update_weight(u[i - term], r, delta))
            out.append(r)
        samples[:] = u[-term:]     # a block shorter than the term only comes last
    return out, weight


def clamp(w):
    return max(min(w, 1024), -1024)


def correlate_2ch(x0, x1, term, delta, weights, samples):
    if term > 0:
        o0, weights[0] = correlate_1ch(x0, term, delta, weights[0], samples[0])
        o1, weights[1] = correlate_1ch(x1, term, delta, weights[1], samples[1])
        return o0, o1
    p0, p1 = samples[1][0], samples[0][0]      # x0[i-1], x1[i-1]
    w0, w1 = weights
    o0, o1 = [], []
    for a, b in zip(x0, x1):
        s0 = b if term == -2 else p1
        s1 = a if term == -1 else p0
        r0 = s32(a - apply_weight(w0, s0))
        r1 = s32(b - apply_weight(w1, s1))
        w0 = clamp(w0 + update_weight(s0, r0, delta))
        w1 = clamp(w1 + update_weight(s1, r1, delta))
        o0.append(r0)
        o1.append(r1)
        p0, p1 = a, b
    weights[0], weights[1] = w0, w1
    samples[1][0], samples[0][0] = p0, p1
    return o0, o1


def encode_residual(r, e):
    """-> (m, offset, add, sign); e, the channel's three medians, is updated"""
    if r >= 0:
        u, sign = r, 0
    else:
        u, sign = -r - 1, 1
    m0, m1, m2 = (e[0] >> 4) + 1, (e[1] >> 4) + 1, (e[2] >> 4) + 1
    if u < m0:
        m, offset, add = 0, u, m0 - 1
        e[0] = s32(e[0] - (s32(e[0] + 126) >> 7) * 2)
    elif u - m0 < m1:
        m, offset, add = 1, u - m0, m1 - 1
        e[0] = s32(e[0] + (s32(e[0] + 128) >> 7) * 5)
        e[1] = s32(e[1] - (s32(e[1] + 62) >> 6) * 2)
    elif u - (m0 + m1) < m2:
        m, offset, add = 2, u - (m0 + m1), m2 - 1
        e[0] = s32(e[0] + (s32(e[0] + 128) >> 7) * 5)
        e[1] = s32(e[1] + (s32(e[1] + 64) >> 6) * 5)
        e[2] = s32(e[2] - (s32(e[2] + 30) >> 5) * 2)
    else:
        m = (u - (m0 + m1)) // m2 + 2
        offset, add = u - (m0 + m1 + (m - 2) * m2), m2 - 1
        e[0] = s32(e[0] + (s32(e[0] + 128) >> 7) * 5)
        e[1] = s32(e[1] + (s32(e[1] + 64) >> 6) * 5)
        e[2] = s32(e[2] + (s32(e[2] + 32) >> 5) * 5)
    return m, offset, add, sign


UNDEF = -1


def flush_residual(bw, u_i_2, res, m_i):
    """res: (zeroes, m, offset, add, sign) of residual i-1 -> unary i-1"""
    zeroes, m1, offset, add, sign = res
    if zeroes != UNDEF:
        write_egc(bw, zeroes)
    if m1 == UNDEF:
        return UNDEF
    even = u_i_2 == UNDEF or u_i_2 % 2 == 0
    odd = u_i_2 == UNDEF or u_i_2 % 2 == 1
    if m1 > 0 and m_i > 0:
        u = m1 * 2 + 1 if even else m1 * 2 - 1
    elif m1 == 0 and m_i > 0:
        u = 1 if odd else UNDEF
    elif m1 > 0 and m_i == 0:
        u = m1 * 2 if even else (m1 - 1) * 2
    else:
        u = 0 if odd else UNDEF
    if u != UNDEF:
        if u < 16:
            bw.unary(u)
        else:
            bw.unary(16)
            write_egc(bw, u - 16)
    if add > 0:
        p = add.bit_length() - 1
        e = (1 << (p + 1)) - add - 1
        if offset < e:
            bw.write(p, offset)
        else:
            bw.write(p, (offset + e) // 2)
            bw.write(1, (offset + e) % 2)
    bw.write(1, sign)
    return u


def write_bitstream(bw, ent, residuals):
    """the zero-run and deferred-unary state is local to the block; the
    medians (ent) are the stream's"""
    nch = len(residuals)
    total = nch * len(residuals[0])
    prev = (UNDEF, UNDEF, 0, 0, 0)
    u_i_2 = UNDEF
    for i in range(total):
        r = residuals[i % nch][i // nch]
        e = ent[i % nch]
        m1 = prev[1]
        undefined = m1 == UNDEF or (m1 == 0 and u_i_2 != UNDEF and u_i_2 % 2 == 0)
        if ent[0][0] < 2 and ent[1][0] < 2 and undefined:
            if prev[0] != UNDEF and m1 == UNDEF:       # in a run of zeroes
                if r == 0:
                    prev = (prev[0] + 1,) + prev[1:]
                else:
                    prev = (prev[0],) + encode_residual(r, e)
            elif r == 0:                               # a run starts
                u_i_2 = flush_residual(bw, u_i_2, prev, 0)
                prev = (1, UNDEF, 0, 0, 0)
                ent[0][:] = [0, 0, 0]
                ent[1][:] = [0, 0, 0]
            else:                                      # false alarm
                cur = (0,) + encode_residual(r, e)
                u_i_2 = flush_residual(bw, u_i_2, prev, cur[1])
                prev = cur
        else:
            cur = (UNDEF,) + encode_residual(r, e)
            u_i_2 = flush_residual(bw, u_i_2, prev, cur[1])
            prev = cur
    flush_residual(bw, u_i_2, prev, 0)


def sub_block(function, nondecoder, payload):
    odd = len(payload) % 2
    head = function | (nondecoder << 5) | (odd << 6)
    words = len(payload) // 2 + odd
    if len(payload) > 510:
        out = bytes([head | 0x80]) + words.to_bytes(3, "little")
    else:
        out = bytes([head, words])
    return out + payload + (b"\0" if odd else b"")


def rate_code(rate):
    return RATES.index(rate) if rate in RATES else 15


def block_header(sub_size, total, index, n, bps, channel_count, joint, n_terms, wasted, first,
                 last, magnitude, rate, false_stereo, crc):
    flags = (bps // 8 - 1) | ((2 - channel_count) << 2) | (joint << 4) | \
        ((n_terms > 5) << 5) | ((wasted > 0) << 8) | (first << 11) | (last << 12) | \
        (magnitude << 18) | (rate_code(rate) << 23) | (false_stereo << 30)
    return struct.pack("<4sIHBBIIIII", b"wvpk", sub_size + 24, 0x407, 0, 0, total & M32,
                       index & M32, n, flags, crc & M32)


def wave_header(channels, mask, bps, rate, frames):
    bb = bps // 8
    data = (frames * channels * bb) & M32
    if channels <= 2 and bps <= 16:
        fmt = struct.pack("<HHIIHH", 1, channels, rate, (rate * channels * bb) & M32,
                          channels * bb, bps)
    else:
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, channels, rate, (rate * channels * bb) & M32,
                          channels * bb, bps, 22, bps, mask) + \
            b"\x01\x00\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
    total = 12 + 8 + len(fmt) + 8 + data
    return b"RIFF" + struct.pack("<I", (total - 8) & M32) + b"WAVEfmt " + \
        struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", data)


def md5_bytes(samples, bps):
    """the PCM as the reference hashes it: little endian at the sample width,
    8-bit samples unsigned"""
    bb = bps // 8
    if bps == 8:
        return bytes((int(s) + 128) & 0xFF for s in samples)
    mask = (1 << bps) - 1
    return b"".join((int(s) & mask).to_bytes(bb, "little") for s in samples)


def encode_block(st, chans, opts, bps, rate, total, index, first, last, channels, mask,
                 first_of_file):
    n = len(chans[0])
    if len(chans) == 1 or (opts["false"] and chans[0] == chans[1]):
        false_stereo = int(len(chans) == 2)
        eff = 1
        work = [chans[0]]
    else:
        false_stereo, eff = 0, 2
        work = chans
    magnitude = max(abs(v).bit_length() for c in work for v in c)
    wasted = 0
    if opts["wasted"]:
        per = []
        for c in work:
            w = [(v & -v).bit_length() - 1 for v in c if v]
            per.append(min(w) if w else 0)
        wasted = min(per)
    shifted = [[v >> wasted for v in c] for c in work]
    crc = M32
    for i in range(n):
        for c in shifted:
            crc = (3 * crc + c[i]) & M32
    if eff == 2 and opts["joint"]:
        shifted = [[s32(a - b) for a, b in zip(*shifted)],
                   [s32(a + b) >> 1 for a, b in zip(*shifted)]]
    if eff == st.effective:
        st.roundtrip()
    else:
        st.reset(eff)
    subs = b""
    if first_of_file:
        size = 20 + (16 if channels <= 2 and bps <= 16 else 40) + 8
        subs += sub_block(0, 0, bytes(size))
    order = range(len(st.terms) - 1, -1, -1)
    if st.terms:
        subs += sub_block(2, 0, bytes(((st.terms[p] + 5) | (DELTA << 5)) for p in order))
        subs += sub_block(3, 0, bytes(store_weight(st.weights[p][c]) & 0xFF
                                      for p in order for c in range(eff)))
        vals = []
        for p in order:
            t, sp = st.terms[p], st.samples[p]
            if t > 8:
                vals += [v for c in range(eff) for v in sp[c][:2]]
            elif t > 0:
                vals += [sp[c][s] for s in range(t) for c in range(eff)]
            else:
                vals += [sp[0][0], sp[1][0]]
        subs += sub_block(4, 0, struct.pack("<%dh" % len(vals), *[wv_log2(v) for v in vals]))
    if wasted > 0:
        subs += sub_block(9, 0, bytes([0, wasted, 0, 0]))
    if channels > 2:
        subs += sub_block(13, 0, bytes([channels]) + struct.pack("<I", mask))
    if rate_code(rate) == 15:
        subs += sub_block(7, 1, struct.pack("<I", rate))
    cur = shifted
    for p in order:
        if eff == 1:
            o, st.weights[p][0] = correlate_1ch(cur[0], st.terms[p], DELTA, st.weights[p][0],
                                                st.samples[p][0])
            cur = [o]
        else:
            cur = list(correlate_2ch(cur[0], cur[1], st.terms[p], DELTA, st.weights[p],
                                     st.samples[p]))
    subs += sub_block(5, 0, struct.pack("<%dH" % (3 * eff), *[
        wv_log2(v) & 0xFFFF for c in range(eff) for v in st.entropies[c]]))
    bw = BitWriter()
    write_bitstream(bw, st.entropies, cur)
    subs += sub_block(10, 0, bw.bytes())
    return block_header(len(subs), total, index, n, bps, len(chans), int(len(chans) == 2 and
                        opts["joint"]), len(st.terms), wasted, first, last, magnitude, rate,
                        false_stereo, crc) + subs


def encode(samples, channels, mask, bps, rate, block_size, passes, joint, false, wasted,
           total_pcm_frames=0):
    """interleaved samples -> the file encoders.encode_wavpack writes.  With
    total_pcm_frames 0 every header's total is fixed up at the end to the
    frames read; otherwise the declared total is written (a path the
    reference's stand-alone encoder cannot reach: read from its source)"""
    samples = [int(v) for v in samples]
    frames = len(samples) // channels
    if passes not in TERMS_2CH or block_size < 1 or channels < 1 or bps not in (8, 16, 24):
        raise ValueError("invalid WavPack encoding parameters")
    if passes and block_size < min_block_size(channels, mask, passes):
        raise ValueError("block size below the history depth of the pass table")
    opts = {"joint": joint, "false": false, "wasted": wasted}
    split = stream_channels(channels, mask)
    streams = [Stream(c, passes) for c in split]
    total_field = total_pcm_frames if total_pcm_frames else frames
    out = bytearray()
    for start in range(0, frames, block_size):
        n = min(block_size, frames - start)
        first_ch = 0
        for k, st in enumerate(streams):
            chans = [samples[(start * channels + first_ch + c):(start + n) * channels:channels]
                     for c in range(st.channels)]
            first_ch += st.channels
            out += encode_block(st, chans, opts, bps, rate, total_field, start, int(k == 0),
                                int(k == len(streams) - 1), channels, mask, not out)
    md5 = hashlib.md5(md5_bytes(samples, bps)).digest()
    footer = sub_block(6, 1, md5)
    out += block_header(len(footer), total_field, M32, 0, bps, 1, 0, 0, 0, 1, 1, 0, rate, 0,
                        M32) + footer
    if frames * channels * (bps // 8) < (1 << 32):
        hdr = sub_block(1, 1, wave_header(channels, mask, bps, rate, frames))
        out[32:32 + len(hdr)] = hdr
    return bytes(out)


def parse_options(opts):
    """a wvenc option list -> encode()'s arguments after the samples"""
    kw = {"channels": 2, "mask": 3, "bps": 16, "rate": 44100, "block_size": 22050, "passes": 5,
          "joint": False, "false": False, "wasted": False}
    names = {"-c": ("channels", 10), "-m": ("mask", 16), "-r": ("rate", 10), "-b": ("bps", 10),
             "-B": ("block_size", 10), "-p": ("passes", 10)}
    flags = {"-j": "joint", "-f": "false", "-w": "wasted"}
    i = 0
    while i < len(opts):
        if opts[i] in names:
            key, base = names[opts[i]]
            kw[key] = int(opts[i + 1], base)
            i += 2
        else:
            kw[flags[opts[i]]] = True
            i += 1
    return kw
