"""A plain Python restatement of the MLP title decode: the access-unit walk,
check data, parser, filters and rematrixing of the reference's
src/decoders/mlp.c, driven as its src/decoders/aob.c drives them (one read
per sector, every whole access unit in the buffer decoded after it).  It
returns the fields of the C ABI's atg_mlp_result and atg_mlp_unit
(include/atgpu_mlp.h) and answers in the terms of the reference's stand-alone
decoder for the golden vectors.  Sequential and written from the rules, not
from the kernels: the GPU is compared with it.

Where the reference reads filter state it never wrote (an order above the
state's length: it indexes before its array and dies), the missing state is
zero here, which is what the format means.  The limits (status UNSUPPORTED)
are those of include/atgpu_mlp.h.
"""
import numpy as np

import aob_port

SECTOR = 2048
(OK, NOT_MLP, NO_MAJOR_SYNC, BAD_SECTOR, EOF, IO_ERROR, INVALID_MAJOR_SYNC, INVALID_EXTRAWORD,
 INVALID_RESTART_HEADER, INVALID_DECODING_PARAMETERS, INVALID_MATRIX_PARAMETERS,
 INVALID_CHANNEL_PARAMETERS, INVALID_BLOCK_DATA, INVALID_FILTER_PARAMETERS, PARITY_MISMATCH,
 CRC8_MISMATCH, UNSUPPORTED) = range(17)
MAX_UNIT_FRAMES = 4096
MAX_MATRIX_CHANNEL = 5

MESSAGES = {
    IO_ERROR: "I/O error reading MLP stream",
    INVALID_MAJOR_SYNC: "invalid MLP major sync",
    INVALID_EXTRAWORD: "invalid extraword present value in substream info",
    INVALID_RESTART_HEADER: "invalid MLP restart header",
    INVALID_DECODING_PARAMETERS: "invalid MLP decoding parameters",
    INVALID_MATRIX_PARAMETERS: "invalid MLP matrix parameters",
    INVALID_CHANNEL_PARAMETERS: "invalid MLP channel parameters",
    INVALID_BLOCK_DATA: "invalid MLP block data",
    INVALID_FILTER_PARAMETERS: "invalid MLP filter parameters",
    PARITY_MISMATCH: "parity mismatch decoding MLP substream",
    CRC8_MISMATCH: "CRC8 mismatch decoding MLP substream",
}

# MLP channel c of assignment a is RIFF WAVE channel WAVE_CHANNEL[a][c]
WAVE_CHANNEL = [[0, 1, 2, 3, 4, 5]] * 18 + [[0, 1, 3, 4, 2, 5]] * 2 + [[0, 1, 4, 5, 2, 3]]


def crc8_table():
    """CRC-8, polynomial 0x63, most significant bit first"""
    t = []
    for i in range(256):
        v = i
        for _ in range(8):
            v = ((v << 1) ^ 0x63) & 0xFF if v & 0x80 else v << 1
        t.append(v)
    return t


CRC8 = crc8_table()


def codebook(k):
    """the prefix code of codebook k (1..3) -> [(bit string, value)]; value -1
    is the invalid codeword"""
    extra = 3 - k
    codes = [("1" + "{:0{}b}".format(b, extra) if extra else "1", 7 + b) for b in range(1 << extra)]
    for z in range(7):
        codes.append(("01" + "0" * z + "1", 7 + (1 << extra) + z))
        codes.append(("00" + "0" * z + "1", 6 - z))
    codes += [("01" + "0" * 7, -1), ("00" + "0" * 7, -1)]
    return codes


def wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def mask(x, q):
    return (x >> q) << q


class Error(Exception):
    def __init__(self, status):
        Exception.__init__(self, status)
        self.status = status


class Bits(object):
    """big-endian bit reader over bytes; a read past the end is an I/O error"""

    def __init__(self, data):
        self.v = int.from_bytes(data, "big") if data else 0
        self.n = 8 * len(data)
        self.pos = 0

    def read(self, k):
        if k > self.n - self.pos:
            raise Error(IO_ERROR)
        self.pos += k
        return (self.v >> (self.n - self.pos)) & ((1 << k) - 1)

    def signed(self, k):
        s = self.read(1)
        v = self.read((k - 1) & 0xFFFFFFFF)
        return v - (s << (k - 1))

    def huffman(self, k):
        if self.read(1):
            return 7 + self.read(3 - k)
        s = self.read(1)
        for z in range(7):
            if self.read(1):
                return 7 + (1 << (3 - k)) + z if s else 6 - z
        return -1


class Channel(object):
    def __init__(self):
        self.fir_shift = self.iir_shift = 0
        self.fir, self.iir = [], []
        self.fir_state, self.iir_state = [0] * 8, [0] * 8   # [0] is the newest
        self.offset = self.codebook = 0
        self.lsbs = 24


class Substream(object):
    """one substream's parser state between restart headers"""

    def __init__(self):
        self.started = False
        self.min = self.max = self.mmc = self.noise_shift = self.seed = 0
        self.flags = [1] * 8
        self.block_size = 8
        self.matrices = []
        self.out_shift, self.quant = [0] * 8, [0] * 8
        self.ch = [Channel() for _ in range(8)]
        self.range0 = None


def read_filter(b, ch, iir):
    order = b.read(4)
    if order > 8:
        raise Error(INVALID_CHANNEL_PARAMETERS)
    coeff, shift, state = [], 0, [0] * 8
    if order:
        shift = b.read(4)
        bits = b.read(5)
        if not 1 <= bits <= 16:
            raise Error(INVALID_CHANNEL_PARAMETERS)
        cshift = b.read(3)
        if bits + cshift > 16:
            raise Error(INVALID_CHANNEL_PARAMETERS)
        coeff = [b.signed(bits) << cshift for _ in range(order)]
        if b.read(1):
            if not iir:
                raise Error(INVALID_CHANNEL_PARAMETERS)
            sbits, sshift = b.read(4), b.read(4)
            for i in range(order):
                state[i] = wrap32(b.signed(sbits) << sshift)
    if iir:
        ch.iir_shift, ch.iir, ch.iir_state = shift, coeff, state
    else:
        ch.fir_shift, ch.fir = shift, coeff


def read_restart(b, ss, title):
    sync, noise_type = b.read(13), b.read(1)
    b.read(16)
    lo, hi, mmc, ss.noise_shift = b.read(4), b.read(4), b.read(4), b.read(4)
    ss.seed = b.read(23)
    b.read(19)
    b.read(1)
    b.read(8)
    b.read(16)
    if sync != 0x18F5 or noise_type or hi < lo or mmc < hi:
        raise Error(INVALID_RESTART_HEADER)
    if mmc > MAX_MATRIX_CHANNEL:
        raise Error(UNSUPPORTED)
    for _ in range(mmc + 1):
        if b.read(6) > mmc:
            raise Error(INVALID_RESTART_HEADER)
    b.read(8)
    ss.min, ss.max, ss.mmc = lo, hi, mmc
    # limits: the channel ranges must tile 0..max_matrix_channel, cover the
    # title's channels and stay what the title's first restart header said
    last = title["index"] == title["substreams"] - 1
    if (title["index"] == 0 and lo != 0) or (last and (hi != mmc or mmc + 1 < title["channels"])):
        raise Error(UNSUPPORTED)
    if ss.range0 is None:
        ss.range0 = (lo, hi, mmc)
    elif ss.range0 != (lo, hi, mmc):
        raise Error(UNSUPPORTED)


def read_parameters(b, ss, header):
    if header:
        ss.flags = [b.read(1) for _ in range(8)] if b.read(1) else [1] * 8
    elif ss.flags[0] and b.read(1):
        ss.flags = [b.read(1) for _ in range(8)]
    f = ss.flags
    if f[7] and b.read(1):
        ss.block_size = b.read(9)
        if ss.block_size < 8:
            raise Error(INVALID_DECODING_PARAMETERS)
    elif header:
        ss.block_size = 8
    if f[6] and b.read(1):
        n = b.read(4)
        if n > 6:
            raise Error(UNSUPPORTED)    # the reference has six matrices
        ms = []
        ss.matrices = ms
        for _ in range(n):
            out, frac = b.read(4), None
            if out > ss.mmc:
                raise Error(INVALID_MATRIX_PARAMETERS)
            frac = b.read(4)
            if frac > 14:
                raise Error(INVALID_MATRIX_PARAMETERS)
            bypass = b.read(1)
            coeff = [(b.signed(frac + 2) << (14 - frac)) if b.read(1) else 0
                     for _ in range(ss.mmc + 3)]
            ms.append((out, bypass, coeff))
    elif header:
        ss.matrices = []
    if f[5] and b.read(1):
        for c in range(ss.mmc + 1):
            ss.out_shift[c] = b.signed(4)
            if ss.out_shift[c] < 0:
                raise Error(UNSUPPORTED)
    elif header:
        ss.out_shift = [0] * 8
    if f[4] and b.read(1):
        for c in range(ss.max + 1):
            ss.quant[c] = b.read(4)
    elif header:
        ss.quant = [0] * 8
    for c in range(ss.min, ss.max + 1):
        ch = ss.ch[c]
        if b.read(1):
            if f[3] and b.read(1):
                read_filter(b, ch, False)
            elif header:
                ch.fir_shift, ch.fir = 0, []
            if f[2] and b.read(1):
                read_filter(b, ch, True)
            elif header:
                ch.iir_shift, ch.iir, ch.iir_state = 0, [], [0] * 8
            if f[1] and b.read(1):
                ch.offset = b.signed(15)
            elif header:
                ch.offset = 0
            ch.codebook = b.read(2)
            ch.lsbs = b.read(5)
            if ch.lsbs > 24:
                raise Error(INVALID_CHANNEL_PARAMETERS)
        elif header:
            ch.fir_shift, ch.fir, ch.iir_shift, ch.iir, ch.iir_state = 0, [], 0, [], [0] * 8
            ch.offset, ch.codebook, ch.lsbs = 0, 0, 24


def read_block(b, ss, title, out, bypass, first):
    """one block: its filtered samples are appended to out[c], its bypassed
    LSBs (a bit per matrix) to bypass"""
    if b.read(1):
        header = b.read(1)
        if header:
            read_restart(b, ss, title)
            ss.started = True
        elif not ss.started:
            raise Error(UNSUPPORTED)    # the reference decodes from unset state
        read_parameters(b, ss, header)
    elif not ss.started:
        raise Error(UNSUPPORTED)
    n = ss.block_size
    if len(bypass) + n > MAX_UNIT_FRAMES:
        raise Error(UNSUPPORTED)
    lsb_bits, offs = {}, {}
    for c in range(ss.min, ss.max + 1):
        ch = ss.ch[c]
        lb = (ch.lsbs - ss.quant[c]) & 0xFFFFFFFF
        lsb_bits[c] = lb
        s = lb & 31
        shift = (lb + 2 - ch.codebook if ch.codebook else lb - 1) & 0xFFFFFFFF
        off = ch.offset - (7 * (1 << s) if ch.codebook else 0)
        if shift < 0x80000000:
            off -= 1 << (shift & 31)
        offs[c] = off
    res = dict((c, []) for c in lsb_bits)
    for _ in range(n):
        bits = 0
        for m, (_, flag, _) in enumerate(ss.matrices):
            if flag:
                bits |= b.read(1) << m
        bypass.append(bits)
        for c in range(ss.min, ss.max + 1):
            ch = ss.ch[c]
            msb = b.huffman(ch.codebook) if ch.codebook else 0
            if msb < 0:
                raise Error(INVALID_BLOCK_DATA)
            lsb = b.read(lsb_bits[c])
            res[c].append(wrap32(wrap32((msb << lsb_bits[c]) + lsb + offs[c]) << ss.quant[c]))
    if first[0] is None:
        first[0] = len(ss.matrices)
    first[0] = min(first[0], len(ss.matrices))
    for c in range(ss.min, ss.max + 1):
        ch = ss.ch[c]
        if len(ch.fir) + len(ch.iir) > 8:
            raise Error(INVALID_FILTER_PARAMETERS)
        if ch.fir_shift and ch.iir_shift:
            if ch.fir_shift != ch.iir_shift:
                raise Error(INVALID_FILTER_PARAMETERS)
            shift = ch.fir_shift
        else:
            shift = ch.fir_shift if ch.fir else ch.iir_shift
        q = ss.quant[c]
        for r in res[c]:
            acc = sum(k * s for k, s in zip(ch.fir, ch.fir_state))
            acc += sum(k * s for k, s in zip(ch.iir, ch.iir_state))
            ssum = wrap32(acc >> shift)
            v = mask(wrap32(ssum + r), q)
            out[c].append(v)
            ch.fir_state = [v] + ch.fir_state[:7]
            ch.iir_state = [wrap32(v - ssum)] + ch.iir_state[:7]


def read_substream(data, ss, title, out):
    """-> the unit's bypassed LSBs of this substream"""
    b = Bits(data)
    bypass, first = [], [None]
    while True:
        read_block(b, ss, title, out, bypass, first)
        if b.read(1):
            break
    if len(ss.matrices) > first[0]:
        raise Error(UNSUPPORTED)    # a matrix added inside the unit
    return bypass


def rematrix(ss, ch, bypass):
    n = len(bypass)
    noise = [[], []]
    seed = ss.seed
    for _ in range(n):
        shifted = (seed >> 7) & 0xFFFF
        a, c = (seed >> 15) & 0xFF, shifted & 0xFF
        noise[0].append(wrap32((a - ((a & 0x80) << 1)) << ss.noise_shift))
        noise[1].append(wrap32((c - ((c & 0x80) << 1)) << ss.noise_shift))
        seed = ((seed << 16) & 0xFFFFFFFF) ^ shifted ^ (shifted << 5)
    ss.seed = seed
    for m, (out, _, coeff) in enumerate(ss.matrices):
        for i in range(n):
            acc = sum(ch[c][i] * coeff[c] for c in range(ss.mmc + 1))
            acc += noise[0][i] * coeff[ss.mmc + 1] + noise[1][i] * coeff[ss.mmc + 2]
            ch[out][i] = wrap32(mask(wrap32(acc >> 14), ss.quant[out]) + ((bypass[i] >> m) & 1))
    for c in range(ss.mmc + 1):
        ch[c] = [wrap32(v << ss.out_shift[c]) for v in ch[c]]


def check_data(data):
    """-> a substream's status from its parity and CRC bytes"""
    parity, crc, final = 0, 0x3C, 0
    for byte in data[:-2]:
        parity ^= byte
        final = crc ^ byte
        crc = CRC8[final]
    if (data[-2] ^ parity) != 0xA9:
        return PARITY_MISMATCH
    return OK if final == data[-1] else CRC8_MISMATCH


def walk_units(stream, ends):
    """the access-unit table of a title's payload stream.  ends[i]: stream
    bytes up to and including sector i.  -> (units, status, unit): status
    UNSUPPORTED for a length field below 2 words at unit `unit`"""
    units, pos, sec = [], 0, 0
    first = None        # the first unit's major sync: the title's
    while len(stream) - pos >= 4:
        words = ((stream[pos] & 15) << 8) | stream[pos + 1]
        if words < 2:
            while ends[sec] < pos + 4:
                sec += 1
            return units, UNSUPPORTED, sec
        size = 2 * words
        if len(stream) - pos < size:
            break
        while ends[sec] < pos + size:
            sec += 1
        u = {"offset": pos, "size": size, "end_sector": sec, "flags": 0, "status": OK,
             "data_start": 0, "substream_end": [0, 0], "substream_flags": [0, 0]}
        body = stream[pos:pos + size]
        p = 4
        if size >= 32 and body[4:8] == b"\xf8\x72\x6f\xbb":
            key = (body[8], body[9], body[11] & 31, body[20] >> 4)
            u["flags"] |= 1
            p = 32
            if first is None and not units:
                first = key
            if key[3] not in (1, 2):
                u["status"] = INVALID_MAJOR_SYNC
            elif key == first:
                u["flags"] |= 2
            elif first is not None:
                u["status"] = INVALID_MAJOR_SYNC
        if first is None:
            # no major sync in the first unit: the reference has no substream count
            u["status"] = UNSUPPORTED
        nss = first[3] if first and first[3] in (1, 2) else 0
        if u["status"] == OK:
            for s in range(nss):
                if p + 2 > size:
                    u["status"] = IO_ERROR
                    break
                info = (body[p] << 8) | body[p + 1]
                p += 2
                u["substream_flags"][s] = (info >> 15) | ((info >> 12) & 2)
                u["substream_end"][s] = 2 * (info & 0xFFF)
                if info >> 15:
                    u["status"] = INVALID_EXTRAWORD
                    break
        u["data_start"] = p
        if u["status"] == OK:
            a = 0
            for s in range(nss):
                e = u["substream_end"][s]
                if a < e <= size - p and (body[p + a] >> 6) == 3:
                    u["substream_flags"][s] |= 4
                a = e
        units.append(u)
        pos += size
    return units, OK, 0


def substream_bytes(u, body, s):
    """the bytes of substream s of a unit -> (data, status)"""
    a = u["substream_end"][s - 1] if s else 0
    e = u["substream_end"][s]
    check = u["substream_flags"][0] & 2
    if e < a + (2 if check else 0) or u["data_start"] + e > u["size"]:
        return b"", IO_ERROR
    data = body[u["data_start"] + a:u["data_start"] + e]
    if check:
        return data[:-2], check_data(data)
    return data, OK


def decode(image, first=0, count=None):
    """a title (sectors [first, first + count) of image) -> (result dict,
    int32 interleaved samples, access-unit table)"""
    recs = aob_port.walk(image, first, count)
    res = {"status": EOF, "stop_sector": 0, "stop_unit": 0, "sample_rate": 0,
           "bits_per_sample": 0, "channels": 0, "channel_mask": 0, "channel_assignment": 0,
           "substreams": 0, "access_units": 0, "good_frames": 0}
    none = np.zeros(0, np.int32)
    if not recs:
        return res, none, []
    bad = next((i for i, r in enumerate(recs) if r["status"]), len(recs))
    if bad == 0:
        res["status"] = BAD_SECTOR
        return res, none, []
    if recs[0]["codec_id"] != 0xA1:
        res["status"] = NOT_MLP
        res["codec_id"] = recs[0]["codec_id"]
        return res, none, []
    parts = [image[(first + i) * SECTOR + r["payload_offset"]:
                   (first + i) * SECTOR + r["payload_offset"] + r["payload_length"]]
             for i, r in enumerate(recs[:bad])]
    if len(parts[0]) < 18 or parts[0][4:8] != b"\xf8\x72\x6f\xbb":
        res["status"] = NO_MAJOR_SYNC
        return res, none, []
    stream = b"".join(parts)
    ends = list(np.cumsum([len(p) for p in parts]))
    ca = stream[11] & 31
    res["channel_assignment"] = ca
    res["bits_per_sample"] = aob_port.BITS.get(stream[8] >> 4, 0)
    res["sample_rate"] = aob_port.RATES.get(stream[9] >> 4, 0)
    res["channels"] = aob_port.CHANNELS[ca] if ca <= 20 else 0
    res["channel_mask"] = aob_port.CHANNEL_MASK[ca] if ca <= 20 else 0
    if res["bits_per_sample"] not in (16, 24) or not res["sample_rate"] or not res["channels"]:
        res["status"] = UNSUPPORTED
        return res, none, []
    units, wstatus, wsector = walk_units(stream, ends)
    res["access_units"] = len(units)
    nss = 0
    if units and units[0]["flags"] & 1 and (stream[units[0]["offset"] + 20] >> 4) in (1, 2):
        nss = stream[units[0]["offset"] + 20] >> 4
    res["substreams"] = nss
    channels = res["channels"]
    sub = [Substream(), Substream()]
    frames, per_unit = [[] for _ in range(channels)], []
    fail = None
    for n, u in enumerate(units):
        body = stream[u["offset"]:u["offset"] + u["size"]]
        status = u["status"]
        out = [[] for _ in range(8)]
        bypass = None
        try:
            if status != OK:
                raise Error(status)
            for s in range(nss):
                data, status = substream_bytes(u, body, s)
                if status != OK:
                    raise Error(status)
                title = {"index": s, "substreams": nss, "channels": channels}
                got = read_substream(data, sub[s], title, out)
                if bypass is not None and len(bypass) != len(got):
                    raise Error(UNSUPPORTED)
                bypass = got
            if nss == 2 and sub[1].min != sub[0].max + 1:
                raise Error(UNSUPPORTED)
            rematrix(sub[nss - 1], out, bypass)
        except Error as e:
            fail = (n, e.status, u["end_sector"])
            break
        per_unit.append((u["end_sector"], len(bypass)))
        for c in range(channels):
            frames[WAVE_CHANNEL[ca][c]] += out[c]
    if fail is None and wstatus != OK:
        fail = (len(units), wstatus, wsector)
    if fail is not None:
        good = sum(k for sec, k in per_unit if sec < fail[2])
        res.update(status=fail[1], stop_unit=fail[0], stop_sector=fail[2])
    else:
        good = sum(k for _, k in per_unit)
        res.update(status=BAD_SECTOR if bad < len(recs) else OK, stop_unit=len(units),
                   stop_sector=bad)
    res["good_frames"] = good
    x = np.array([ch[:good] for ch in frames], dtype=np.int64).reshape(channels, good).T.reshape(-1)
    bits = res["bits_per_sample"]
    # the ABI's value is sign-wrapped to the title's bits; the reference's
    # stand-alone decoder clips instead, so its answer needs the full value
    res["full"] = x
    x = ((x + (1 << (bits - 1))) & ((1 << bits) - 1)) - (1 << (bits - 1))
    return res, x.astype(np.int32), units


def answer_from(res, x, pts_ticks):
    """aobdec's answer (PCM bytes, stderr without the frame count line) for a
    request of pts_ticks, from a title's result and samples, whoever decoded
    it; None where the reference has no defined answer (a limit, a request
    past the end of the sectors, a title it does not type as MLP)"""
    if res["status"] == BAD_SECTOR and res["stop_sector"] == 0:
        return b"", "I/O error reading initialization packet\n*** Error getting next track\n"
    if res["status"] == NOT_MLP and res.get("codec_id") != 0xA0:
        return b"", "*** Error getting next track\n"
    if res["status"] in (NOT_MLP, NO_MAJOR_SYNC, UNSUPPORTED, EOF):
        return None
    want = aob_port.track_frames(pts_ticks, res["sample_rate"])
    have = min(want, res["good_frames"])
    bits = res["bits_per_sample"]
    full = np.clip(res.get("full", x), -(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    raw = aob_port.pcm_bytes(full[:have * res["channels"]], bits)
    if want <= res["good_frames"]:
        return raw, ""
    if res["status"] == BAD_SECTOR:
        return raw, "I/O Error reading MLP packet\n"
    if res["status"] == OK:
        return None
    return raw, "*** MLP Error: %s\n" % MESSAGES[res["status"]]
