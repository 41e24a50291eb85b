"""A writer of MLP streams for the tests (there is no MLP encoder anywhere):
access units, major syncs, substream infos, check data, restart headers,
every decoding-parameter field, FIR and IIR parameters with residuals
computed so that a chosen signal comes out of the filters, matrices with LSB
bypass and noise coefficients, the three codebooks, two substreams.  The
stream is cut into the payloads of dvda_build.sector(..., codec=0xA1) sectors.

Everything is made from a dict (`title`) and a seed; tests/mlp_cases.py
expands its compact specs into such dicts.

title: bits, rate (code), assignment, substreams (1 / 2), check (bool),
  units: [unit].
unit: sync (bool), blocks: [[block ...] per substream]; optional: words (the
  length field when it should lie), extraword / nonrestart (per substream),
  sync_fields (a changed major sync), tail (bytes appended to the unit),
  bad_parity / bad_crc (substream index).  build_stream leaves
  title["signal"][substream][channel]: the values that come out of the filters.
block: n (frames, written as block size where it differs), and optional
  restart {min, max, mmc, noise_shift, seed, sync, noise_type, assign},
  flags [8], matrices [{out, frac, bypass, coef [raw or None]}], out_shift,
  quant, chan {c: {fir, iir, offset, codebook, lsbs}}, absent (no decoding
  parameters at all), symbols (codeword values to cycle through, -1 the
  invalid one) or amp (the signal's bits).
fir / iir: {order, shift, bits, cshift, coef [raw], state {bits, shift, vals}}
"""
import numpy as np

import dvda_build
from mlp_port import CRC8, codebook

SYNC = b"\xf8\x72\x6f\xbb"
MAX_SYMBOL = {1: 17, 2: 15, 3: 14}


def wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


class Writer(object):
    def __init__(self):
        self.s = []

    def u(self, v, n):
        if n:
            self.s.append("{:0{}b}".format(v & ((1 << n) - 1), n))

    def code(self, bits):
        self.s.append(bits)

    def data(self):
        """padded with zero bits to a whole number of 16-bit words"""
        s = "".join(self.s)
        s += "0" * (-len(s) % 16)
        return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""


class Chan(object):
    def __init__(self):
        self.fir, self.iir, self.fir_shift, self.iir_shift = [], [], 0, 0
        self.fir_state, self.iir_state = [0] * 8, [0] * 8
        self.offset, self.codebook, self.lsbs = 0, 0, 24


class State(object):
    """what a decoder holds after the blocks written so far"""

    def __init__(self):
        self.flags = [1] * 8
        self.block_size = 8
        self.min = self.max = self.mmc = 0
        self.matrices = []
        self.quant = [0] * 8
        self.ch = [Chan() for _ in range(8)]
        self.signal = [[] for _ in range(8)]    # what comes out of the filters


def write_filter(w, ch, f, iir):
    order = f["order"]
    w.u(order, 4)
    coef, shift, state = [], 0, [0] * 8
    if 0 < order <= 8:
        shift = f.get("shift", 0)
        w.u(shift, 4)
        w.u(f["bits"], 5)
        w.u(f.get("cshift", 0), 3)
        for v in f["coef"]:
            w.u(v, f["bits"])
        coef = [v << f.get("cshift", 0) for v in f["coef"]]
        st = f.get("state")
        w.u(1 if st else 0, 1)
        if st:
            w.u(st["bits"], 4)
            w.u(st["shift"], 4)
            for i, v in enumerate(st["vals"]):
                w.u(v, st["bits"])
                state[i] = v << st["shift"]
    if iir:
        ch.iir, ch.iir_shift, ch.iir_state = coef, shift, state
    else:
        ch.fir, ch.fir_shift = coef, shift


def write_block(w, st, blk, rng):
    """-> the block's frames"""
    if blk.get("absent"):
        w.u(0, 1)
    else:
        w.u(1, 1)
        r = blk.get("restart")
        w.u(1 if r else 0, 1)
        if r:
            w.u(r.get("sync", 0x18F5), 13)
            w.u(r.get("noise_type", 0), 1)
            w.u(0, 16)
            for k in ("min", "max", "mmc", "noise_shift"):
                w.u(r.get(k, 0), 4)
            w.u(r.get("seed", 0), 23)
            w.u(0, 19)
            w.u(0, 1)
            w.u(0, 8)
            w.u(0, 16)
            for c in range(r.get("mmc", 0) + 1):
                w.u(r.get("assign", list(range(16)))[c], 6)
            w.u(0, 8)
            st.min, st.max, st.mmc = r.get("min", 0), r.get("max", 0), r.get("mmc", 0)
        if "flags" in blk:
            w.u(1, 1)
            for f in blk["flags"]:
                w.u(f, 1)
            st.flags = list(blk["flags"])
        elif r:
            w.u(0, 1)
            st.flags = [1] * 8
        elif st.flags[0]:
            w.u(0, 1)
        f = st.flags
        if f[7]:
            size = blk.get("block_size", blk.get("n", 8 if r else st.block_size))
            change = size != (8 if r else st.block_size)
            w.u(1 if change else 0, 1)
            if change:
                w.u(size, 9)
                st.block_size = size
            elif r:
                st.block_size = 8
        elif r:
            st.block_size = 8
        if f[6]:
            ms = blk.get("matrices")
            w.u(0 if ms is None else 1, 1)
            if ms is not None:
                w.u(blk.get("matrix_count", len(ms)), 4)
                st.matrices = []
                for m in ms:
                    w.u(m["out"], 4)
                    w.u(m["frac"], 4)
                    w.u(m.get("bypass", 0), 1)
                    for v in m["coef"]:
                        w.u(0 if v is None else 1, 1)
                        if v is not None:
                            w.u(v, m["frac"] + 2)
                    st.matrices.append(m.get("bypass", 0))
            elif r:
                st.matrices = []
        elif r:
            st.matrices = []
        if f[5]:
            sh = blk.get("out_shift")
            w.u(0 if sh is None else 1, 1)
            for v in sh or ():
                w.u(v, 4)
        if f[4]:
            q = blk.get("quant")
            w.u(0 if q is None else 1, 1)
            if q is not None:
                for c, v in enumerate(q):
                    w.u(v, 4)
                    st.quant[c] = v
            elif r:
                st.quant = [0] * 8
        elif r:
            st.quant = [0] * 8
        for c in range(st.min, st.max + 1):
            ch = st.ch[c]
            p = blk.get("chan", {}).get(str(c))
            w.u(0 if p is None else 1, 1)
            if p is None:
                if r:
                    ch.fir, ch.iir, ch.fir_shift, ch.iir_shift = [], [], 0, 0
                    ch.iir_state = [0] * 8
                    ch.offset, ch.codebook, ch.lsbs = 0, 0, 24
                continue
            for key, iir, flag in (("fir", False, f[3]), ("iir", True, f[2])):
                if flag:
                    w.u(1 if key in p else 0, 1)
                if flag and key in p:
                    write_filter(w, ch, p[key], iir)
                elif r and iir:
                    ch.iir, ch.iir_shift, ch.iir_state = [], 0, [0] * 8
                elif r:
                    ch.fir, ch.fir_shift = [], 0
            if f[1]:
                w.u(1 if "offset" in p else 0, 1)
            if f[1] and "offset" in p:
                w.u(p["offset"], 15)
                ch.offset = p["offset"]
            elif r:
                ch.offset = 0
            ch.codebook, ch.lsbs = p.get("codebook", 0), p.get("lsbs", 24)
            w.u(ch.codebook, 2)
            w.u(ch.lsbs, 5)
    n = st.block_size
    symbols = blk.get("symbols")
    amp = blk.get("amp", 10)
    codes = dict((k, dict((v, b) for b, v in codebook(k) if v >= 0)) for k in (1, 2, 3))
    bad = dict((k, [b for b, v in codebook(k) if v < 0]) for k in (1, 2, 3))
    count = 0
    for i in range(n):
        for flag in st.matrices:
            if flag:
                w.u(int(rng.integers(0, 2)), 1)
        for c in range(st.min, st.max + 1):
            ch = st.ch[c]
            q = st.quant[c]
            lb = ch.lsbs - q
            k = ch.codebook
            if lb < 0:
                return n     # a case that lies: the reader fails on the first sample
            off = ch.offset - ((7 << lb) if k else 0)
            sign = lb + 2 - k if k else lb - 1
            if sign >= 0:
                off -= 1 << sign
            shift = ch.fir_shift if (ch.fir_shift and ch.iir_shift) or ch.fir else ch.iir_shift
            acc = sum(a * b for a, b in zip(ch.fir, ch.fir_state))
            acc += sum(a * b for a, b in zip(ch.iir, ch.iir_state))
            ssum = wrap32(acc >> shift)
            top = ((MAX_SYMBOL[k] + 1) if k else 1) << lb
            if symbols is not None and k:
                sym = symbols[count % len(symbols)]
                count += 1
                if sym < 0:
                    w.code(bad[k][(-sym - 1) % 2])
                    return n
                t = (sym % (MAX_SYMBOL[k] + 1) << lb) | int(rng.integers(0, 1 << lb))
            else:
                want = (int(rng.integers(-(1 << amp), 1 << amp)) >> q) << q
                t = min(max(((want - ssum) >> q) - off, 0), top - 1)
            if k:
                w.code(codes[k][t >> lb])
            w.u(t & ((1 << lb) - 1), lb)
            v = wrap32(ssum + wrap32((t + off) << q))
            v = (v >> q) << q
            ch.fir_state = [v] + ch.fir_state[:7]
            ch.iir_state = [wrap32(v - ssum)] + ch.iir_state[:7]
            st.signal[c].append(v)
    return n


def check_bytes(data):
    parity, crc, final = 0, 0x3C, 0
    for b in data:
        parity ^= b
        final = crc ^ b
        crc = CRC8[final]
    return bytes([parity ^ 0xA9, final])


def major_sync(title, fields=None):
    f = dict(bps=dvda_build.BPS_CODE[title["bits"]], rate=title.get("rate", 0),
             assignment=title["assignment"], count=title["substreams"])
    f.update(fields or {})
    b = bytearray(28)
    b[0:4] = SYNC
    b[4] = (f["bps"] << 4) | f.get("bps1", 0)
    b[5] = (f["rate"] << 4) | f.get("rate1", 0)
    b[7] = f["assignment"] & 31
    b[16] = (f["count"] << 4)
    return bytes(b)


def build_stream(title, seed=0):
    rng = np.random.default_rng(seed)
    states = [State(), State()]
    out = []
    for u in title["units"]:
        subs, ends = [], []
        for s in range(title["substreams"]):
            w = Writer()
            blocks = u["blocks"][s]
            for i, blk in enumerate(blocks):
                write_block(w, states[s], blk, rng)
                w.u(1 if i == len(blocks) - 1 else 0, 1)
            data = w.data()
            if title.get("check"):
                cb = bytearray(check_bytes(data))
                if u.get("bad_parity") == s:
                    cb[0] ^= 1
                if u.get("bad_crc") == s:
                    cb[1] ^= 1
                data += bytes(cb)
            subs.append(data)
            ends.append(sum(len(d) for d in subs))
        body = major_sync(title, u.get("sync_fields")) if u.get("sync") else b""
        for s in range(title["substreams"]):
            end = u.get("ends", ends)[s]
            info = (0x8000 if s in u.get("extraword", ()) else 0) | \
                (0x4000 if s in u.get("nonrestart", ()) else 0) | \
                (0x2000 if title.get("check") else 0) | (end // 2)
            body += info.to_bytes(2, "big")
        body += b"".join(subs) + bytes(u.get("tail", 0))
        words = u.get("words", (len(body) + 4) // 2)
        out.append(bytes([0xF0 & int(rng.integers(0, 256)) | (words >> 8), words & 0xFF,
                          int(rng.integers(0, 256)), int(rng.integers(0, 256))]) + body)
    title["signal"] = [st.signal for st in states]
    return b"".join(out)


def image(stream, payloads, codec=0xA1, pad2=6, **kw):
    """cut a stream into sector payloads (the list is cycled; the stream's
    rest goes to a last sector) -> AOB image"""
    out, pos, i = [], 0, 0
    while pos < len(stream) or not out:
        n = payloads[i % len(payloads)]
        if i >= len(payloads):
            n = max(n, 1)
        out.append(dvda_build.sector(stream[pos:pos + n], codec=codec, pad2=pad2, **kw))
        pos += n
        i += 1
    return b"".join(out)
