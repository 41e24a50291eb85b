"""True Audio (TTA1) in numpy: the checker the TTA tests compare the GPU
codec with.  Written from the format description; never imported by the
package.

A TTA frame is a serial recurrence per channel, which plain Python walks at
about a second per frame.  Instead every chain of a call (all frames, all
channels, all tracks handed in together) advances in lockstep, one numpy
operation per step over the vector of chains, so a whole set of test vectors
costs about as much as one frame.

Layout of a file:  22-byte header, seektable (one u32 per frame + CRC-32),
frames (Rice payload, byte aligned, + CRC-32), all little-endian, bits LSB
first.  CRC-32 is zlib's.
"""
import struct
import zlib

import numpy as np

OK, IO_ERROR, CRC_MISMATCH, INVALID_SIGNATURE, UNSUPPORTED_FORMAT, FRAME_READ = range(6)

I32 = np.int32
U32 = np.uint32
I64 = np.int64


def block_size(rate):
    return (rate * 256) // 245


def _wrap32(a):
    """int64 values reduced to int32 with two's complement wraparound"""
    return a.astype(np.int64).astype(np.uint32).astype(np.int32)


def _pad(rows, dtype=I64):
    n = max([len(r) for r in rows] + [0])
    out = np.zeros((len(rows), n), dtype)
    for k, r in enumerate(rows):
        out[k, :len(r)] = r
    return out, np.array([len(r) for r in rows], I64)


# ------------------------------------------------------------ signal path
def correlate(x):
    """x[n, C] -> the channel differences; the last channel is itself less
    half the difference below it, halved toward zero"""
    x = x.astype(I64)
    C = x.shape[1]
    if C == 1:
        return x.copy()
    out = np.empty_like(x)
    out[:, :C - 1] = x[:, 1:] - x[:, :C - 1]
    d = out[:, C - 2]
    half = np.where(d >= 0, d // 2, -((-d) // 2))
    out[:, C - 1] = x[:, C - 1] - half
    return out


def decorrelate(p):
    p = p.astype(I64)
    C = p.shape[1]
    if C == 1:
        return p.copy()
    out = np.empty_like(p)
    d = p[:, C - 2]
    half = np.where(d >= 0, d // 2, -((-d) // 2))
    out[:, C - 1] = p[:, C - 1] + half
    for c in range(C - 2, -1, -1):
        out[:, c] = out[:, c + 1] - p[:, c]
    return out


def _fixed_term(prev, s):
    return ((prev.astype(I64) << s) - prev) >> s


class _Hybrid(object):
    """eight-tap sign-LMS filter state for a vector of chains; products and
    their sum wrap at 32 bits"""

    def __init__(self, n, shift):
        self.qm = np.zeros((8, n), I64)
        self.dx = np.zeros((8, n), I64)
        self.dl = np.zeros((8, n), I64)
        self.shift = shift  # per chain

    def adapt(self, prev_residual):
        self.qm = _wrap32(self.qm + np.sign(prev_residual) * self.dx).astype(I64)

    def predict(self):
        total = (1 << (self.shift - 1)).astype(I64)
        for j in range(8):
            total = total + _wrap32(self.dl[j] * self.qm[j]).astype(I64)
        return _wrap32(total).astype(I64) >> self.shift

    def push(self, v):
        dl, dx = self.dl, self.dx
        ndx = np.empty_like(dx)
        ndx[0:3] = dx[1:4]
        ndx[3] = dx[4]
        for j, step in ((4, 1), (5, 2), (6, 2), (7, 4)):
            ndx[j] = np.where(dl[j] >= 0, step, -step)
        ndl = np.empty_like(dl)
        ndl[0:3] = dl[1:4]
        ndl[3] = dl[4]
        a = v - dl[7]
        b = a - dl[6]
        ndl[4] = b - dl[5]
        ndl[5] = b
        ndl[6] = a
        ndl[7] = v
        self.dx = ndx
        self.dl = _wrap32(ndl).astype(I64)


def _shifts(bps):
    return (9 if bps == 16 else 10), (4 if bps == 8 else 5)


def residuals(chains, bps_list):
    """encoder: correlated channel signals (list of 1-D arrays) -> residuals"""
    x, lens = _pad(chains)
    n = len(chains)
    hs = np.array([_shifts(b)[0] for b in bps_list], I64)
    ps = np.array([_shifts(b)[1] for b in bps_list], I64)
    h = _Hybrid(n, hs)
    out = np.zeros_like(x)
    for i in range(x.shape[1]):
        if i == 0:
            p = x[:, 0].copy()
            r = p.copy()
        else:
            p = _wrap32(x[:, i] - _fixed_term(x[:, i - 1], ps)).astype(I64)
            h.adapt(out[:, i - 1])
            r = _wrap32(p - h.predict()).astype(I64)
        h.push(p)
        out[:, i] = r
    return [out[k, :lens[k]] for k in range(n)]


def reconstruct(chains, bps_list):
    """decoder: residuals -> correlated channel signals"""
    x, lens = _pad(chains)
    n = len(chains)
    hs = np.array([_shifts(b)[0] for b in bps_list], I64)
    ps = np.array([_shifts(b)[1] for b in bps_list], I64)
    h = _Hybrid(n, hs)
    out = np.zeros_like(x)
    for i in range(x.shape[1]):
        r = x[:, i]
        if i == 0:
            f = r.copy()
            o = f.copy()
        else:
            h.adapt(x[:, i - 1])
            f = _wrap32(r + h.predict()).astype(I64)
            o = _wrap32(f + _fixed_term(out[:, i - 1], ps)).astype(I64)
        h.push(f)
        out[:, i] = o
    return [out[k, :lens[k]] for k in range(n)]


# ------------------------------------------------------------------ Rice
class _Rice(object):
    def __init__(self, n):
        self.k0 = np.full(n, 10, I64)
        self.k1 = np.full(n, 10, I64)
        self.s0 = np.full(n, 1 << 14, I64)
        self.s1 = np.full(n, 1 << 14, I64)

    @staticmethod
    def _adapt(k, s, v, on):
        s2 = _wrap32(s + v - (s >> 4)).astype(I64)
        down = (k > 0) & (s2 < (1 << (k + 4)))
        up = ~down & (s2 > (1 << (k + 5)))
        k2 = k - down + up
        return np.where(on, k2, k), np.where(on, s2, s)


def rice_codes(resid):
    """residual chains -> per chain (run, k, val) arrays: `run` ones, a zero,
    then `val` in k bits"""
    r, lens = _pad(resid)
    n = len(resid)
    st = _Rice(n)
    run = np.zeros_like(r)
    kk = np.zeros_like(r)
    val = np.zeros_like(r)
    every = np.ones(n, bool)
    for i in range(r.shape[1]):
        v = r[:, i]
        u = np.where(v > 0, 2 * v - 1, -2 * v)
        small = u < (1 << st.k0)
        shifted = u - (1 << st.k0)
        run[:, i] = np.where(small, 0, 1 + (shifted >> st.k1))
        kk[:, i] = np.where(small, st.k0, st.k1)
        val[:, i] = np.where(small, u, shifted & ((1 << st.k1) - 1))
        st.k1, st.s1 = _Rice._adapt(st.k1, st.s1, shifted, ~small)
        st.k0, st.s0 = _Rice._adapt(st.k0, st.s0, u, every)
    return [(run[k, :lens[k]], kk[k, :lens[k]], val[k, :lens[k]]) for k in range(n)]


def pack_frame(codes):
    """codes of one frame's channels -> payload + CRC-32"""
    C = len(codes)
    run = np.stack([c[0] for c in codes], 1).reshape(-1)
    k = np.stack([c[1] for c in codes], 1).reshape(-1)
    val = np.stack([c[2] for c in codes], 1).reshape(-1)
    length = run + 1 + k
    end = np.cumsum(length)
    start = end - length
    total = int(end[-1]) if len(end) else 0
    mark = np.zeros(total + 1, np.int8)
    np.add.at(mark, start, 1)
    np.add.at(mark, start + run, -1)
    bits = np.cumsum(mark[:total]).astype(np.uint8)
    for b in range(int(k.max()) if len(k) else 0):
        m = k > b
        bits[(start + run + 1 + b)[m]] = ((val[m] >> b) & 1).astype(np.uint8)
    payload = np.packbits(bits, bitorder="little").tobytes()
    assert C >= 1
    return payload + struct.pack("<I", zlib.crc32(payload) & 0xFFFFFFFF)


# --------------------------------------------------------------- encoding
def split(n_frames, rate, sizes=None):
    if sizes is not None:
        assert sum(sizes) == n_frames
        return list(sizes)
    b = block_size(rate)
    out = [b] * (n_frames // b)
    if n_frames % b:
        out.append(n_frames % b)
    return out


def encode_frames_many(jobs):
    """jobs: [(interleaved samples, channels, bps, rate, sizes or None)]
    -> per job the list of frame byte strings"""
    chains, bpsl, index = [], [], []
    for j, (pcm, C, bps, rate, sizes) in enumerate(jobs):
        x = np.asarray(pcm, I64).reshape(-1, C)
        pos = 0
        for f, n in enumerate(split(len(x), rate, sizes)):
            cor = correlate(x[pos:pos + n])
            pos += n
            for c in range(C):
                chains.append(cor[:, c])
                bpsl.append(bps)
                index.append((j, f))
    codes = rice_codes(residuals(chains, bpsl)) if chains else []
    out = [[] for _ in jobs]
    k = 0
    while k < len(index):
        j, f = index[k]
        C = jobs[j][1]
        out[j].append(pack_frame(codes[k:k + C]))
        k += C
    return out


def encode_frames(pcm, channels, bps, rate, sizes=None):
    return encode_frames_many([(pcm, channels, bps, rate, sizes)])[0]


def header(channels, bps, rate, total):
    h = b"TTA1" + struct.pack("<HHHII", 1, channels, bps, rate, total)
    return h + struct.pack("<I", zlib.crc32(h) & 0xFFFFFFFF)


def seektable(sizes):
    t = b"".join(struct.pack("<I", s) for s in sizes)
    return t + struct.pack("<I", zlib.crc32(t) & 0xFFFFFFFF)


def build_file(frames, channels, bps, rate, total):
    return header(channels, bps, rate, total) + seektable([len(f) for f in frames]) + \
        b"".join(frames)


def encode_many(jobs):
    """jobs: [(samples, channels, bps, rate)] -> [(file image, frame sizes)]"""
    res = encode_frames_many([j + (None,) for j in jobs])
    out = []
    for (pcm, C, bps, rate), frames in zip(jobs, res):
        out.append((build_file(frames, C, bps, rate, len(pcm) // C), [len(f) for f in frames]))
    return out


def encode(pcm, channels, bps, rate):
    return encode_many([(pcm, channels, bps, rate)])[0]


# --------------------------------------------------------------- decoding
def skip_id3v2(data):
    pos = 0
    while (len(data) - pos >= 10 and data[pos:pos + 3] == b"ID3" and data[pos + 3] in (2, 3, 4)
           and not any(b & 0x80 for b in data[pos + 6:pos + 10])):
        size = 0
        for b in data[pos + 6:pos + 10]:
            size = (size << 7) | b
        if 10 + size > len(data) - pos:
            return len(data)
        pos += 10 + size
    return pos


def read_info(data):
    """-> (status, stage, info dict, frame sizes); stage 0 = header failed,
    1 = seektable failed, 2 = parsed"""
    data = bytes(data)
    pos = skip_id3v2(data)
    h = data[pos:]
    info = {"id3_bytes": pos}
    if len(h) < 18:
        return IO_ERROR, 0, info, []
    fmt, C, bps, rate, total = struct.unpack("<HHHII", h[4:18])
    info.update(channels=C, bits_per_sample=bps, sample_rate=rate, total_pcm_frames=total)
    if h[:4] != b"TTA1":
        return INVALID_SIGNATURE, 0, info, []
    if fmt != 1:
        return UNSUPPORTED_FORMAT, 0, info, []
    if len(h) < 22:
        return IO_ERROR, 0, info, []
    if struct.unpack("<I", h[18:22])[0] != zlib.crc32(h[:18]) & 0xFFFFFFFF:
        return CRC_MISMATCH, 0, info, []
    b = block_size(rate)
    info["block_size"] = b
    if total and not b:
        return UNSUPPORTED_FORMAT, 1, info, []
    nf = (total + b - 1) // b if total else 0
    info["total_tta_frames"] = nf
    if len(h) - 22 < 4 * nf + 4:
        return IO_ERROR, 1, info, []
    tb = h[22:22 + 4 * nf]
    if struct.unpack("<I", h[22 + 4 * nf:26 + 4 * nf])[0] != zlib.crc32(tb) & 0xFFFFFFFF:
        return CRC_MISMATCH, 1, info, []
    info["frames_offset"] = pos + 22 + 4 * nf + 4
    return OK, 2, info, list(struct.unpack("<%dI" % nf, tb))


def parse_payloads(frames):
    """frames: [(payload bytes, pcm frames n, channels)] -> per frame
    (status, [residual chain per channel]); all frames walk in lockstep"""
    F = len(frames)
    if not F:
        return []
    parts, base, end = [], np.zeros(F, I64), np.zeros(F, I64)
    pos = 0
    for k, (payload, n, C) in enumerate(frames):
        b = np.unpackbits(np.frombuffer(payload, np.uint8), bitorder="little")
        parts.append(b)
        base[k] = pos
        pos += len(b)
        end[k] = pos
    pad = 64
    raw = np.concatenate([np.frombuffer(f[0], np.uint8) for f in frames] +
                         [np.zeros(16, np.uint8)]).astype(I64)
    zeros = np.flatnonzero(np.concatenate(parts) == 0)
    del parts
    zeros = np.concatenate([zeros, [pos + pad]])
    Cs = np.array([f[2] for f in frames], I64)
    ns = np.array([f[1] for f in frames], I64)
    Cmax, nmax = int(Cs.max()), int(ns.max())
    st = [_Rice(F) for _ in range(Cmax)]
    cur = base.copy()
    alive = np.ones(F, bool)
    out = np.zeros((F, Cmax, nmax), I64)

    def take(k, on):
        nonlocal cur, alive
        ok = cur + k <= end
        p = np.minimum(cur, pos)
        at = p >> 3
        word = raw[at] | raw[at + 1] << 8 | raw[at + 2] << 16 | raw[at + 3] << 24 | \
            raw[at + 4] << 32
        v = np.where(on & ok, (word >> (p & 7)) & ((1 << k) - 1), 0)
        alive = np.where(on, alive & ok, alive)
        cur = np.where(on & ok, cur + k, cur)
        return v

    for i in range(nmax):
        for c in range(Cmax):
            on = alive & (i < ns) & (c < Cs)
            if not on.any():
                continue
            z = zeros[np.searchsorted(zeros, np.minimum(cur, pos))]
            found = z < end
            alive = np.where(on, alive & found, alive)
            on = on & found
            msb = z - cur
            cur = np.where(on, z + 1, cur)
            s = st[c]
            esc = on & (msb > 0)
            low = take(np.where(esc, s.k1, s.k0), on)
            on = on & alive
            esc = esc & on
            unshifted = (((msb - 1) << s.k1) + low) & 0xFFFFFFFF
            u = np.where(esc, (unshifted + (1 << s.k0)) & 0xFFFFFFFF, low)
            s.k1, s.s1 = _Rice._adapt(s.k1, s.s1, unshifted, esc)
            s.k0, s.s0 = _Rice._adapt(s.k0, s.s0, u, on)
            r = np.where(u & 1, ((u + 1) & 0xFFFFFFFF) >> 1, -(u >> 1))
            out[:, c, i] = np.where(on, r, out[:, c, i])
    res = []
    for k, (payload, n, C) in enumerate(frames):
        res.append((OK if alive[k] else FRAME_READ, [out[k, c, :n] for c in range(C)]))
    return res


def decode_many(images):
    """[image] -> [(status, stage, first bad frame or None, int32 interleaved
    PCM of the frames before it, info)] in the decoder's order: header,
    seektable, then per frame: bytes present, CRC, Rice walk"""
    heads = [read_info(img) for img in images]
    todo, where = [], []
    plans = []
    for t, (img, (st, stage, info, sizes)) in enumerate(zip(images, heads)):
        plan = []
        if st == OK:
            img = bytes(img)
            pos, left = info["frames_offset"], info["total_pcm_frames"]
            for k, size in enumerate(sizes):
                n = min(left, info["block_size"])
                if size < 4 or pos + size > len(img):
                    plan.append((IO_ERROR, None))
                    break
                payload = img[pos:pos + size - 4]
                if struct.unpack("<I", img[pos + size - 4:pos + size])[0] != \
                        zlib.crc32(payload) & 0xFFFFFFFF:
                    plan.append((CRC_MISMATCH, None))
                    break
                plan.append((OK, len(todo)))
                todo.append((payload, n, info["channels"]))
                where.append(t)
                pos += size
                left -= n
        plans.append(plan)
    parsed = parse_payloads(todo)
    # frames up to each track's first bad one go through the filters
    chains, bpsl, slots = [], [], []
    for t, plan in enumerate(plans):
        for st, idx in plan:
            if st != OK or parsed[idx][0] != OK:
                break
            for ch in parsed[idx][1]:
                chains.append(ch)
                bpsl.append(heads[t][2]["bits_per_sample"])
            slots.append((t, idx))
    rec = reconstruct(chains, bpsl) if chains else []
    out, k = [], 0
    per_track = [[] for _ in images]
    for t, idx in slots:
        C = heads[t][2]["channels"]
        p = np.stack(rec[k:k + C], 1)
        k += C
        per_track[t].append(decorrelate(p).reshape(-1))
    for t, (st, stage, info, sizes) in enumerate(heads):
        if st != OK:
            out.append((st, stage, None, np.zeros(0, I32), info))
            continue
        status, bad = OK, None
        for f, (fst, idx) in enumerate(plans[t]):
            s = fst if fst != OK else parsed[idx][0]
            if s != OK:
                status, bad = s, f
                break
        pcm = (np.concatenate(per_track[t]) if per_track[t] else np.zeros(0, I64))
        out.append((status, 2, bad, _wrap32(pcm), info))
    return out


def decode(image):
    return decode_many([image])[0]
