"""Ogg FLAC in Python: a deterministic muxer and the decode contract.

The muxer builds .oga images from FLAC packets with a chosen page layout.
`decode` restates what the reference's Ogg FLAC decoder does with an image
(src/ogg.c:24-254 and src/decoders/oggflac.c:324-559): the page checks in
file order, packets from the lacing tables, the first packet's checks, the
skipped header packets, one FLAC frame per audio packet (oracle_port's frame
decoder, bounded by the packet), the MD5 at the end.  The one case in which
the reference cannot be followed -- a frame whose subframes end within the
last two bytes of its packet, where it aborts -- is FD_EOF here.
"""
import ctypes
import hashlib
import random
import zlib

import numpy as np

import oracle_port

# ogg_status of include/atgpu.h (ATG_OGG_*)
OGG_OK, OGG_MAGIC, OGG_VERSION, OGG_CHECKSUM, OGG_EOF, OGG_FINISHED = 0, 1, 2, 3, 4, 5
OGG_PACKET_BYTE, OGG_SIGNATURE, OGG_MAJOR, OGG_MINOR, OGG_FLAC_SIGNATURE = 6, 7, 8, 9, 10
OGG_BLOCK_TYPE, OGG_STREAMINFO_EOF = 11, 12
OGG_MESSAGES = {
    OGG_MAGIC: "invalid magic number", OGG_VERSION: "invalid stream version",
    OGG_CHECKSUM: "checksum mismatch", OGG_EOF: "premature EOF reading Ogg stream",
    OGG_FINISHED: "stream finished", OGG_PACKET_BYTE: "invalid packet byte",
    OGG_SIGNATURE: "invalid Ogg signature", OGG_MAJOR: "invalid major version",
    OGG_MINOR: "invalid minor version", OGG_FLAC_SIGNATURE: "invalid fLaC signature",
    OGG_BLOCK_TYPE: "invalid block type", OGG_STREAMINFO_EOF: "EOF while reading STREAMINFO block",
}
OGG_IOERRORS = (OGG_EOF, OGG_FINISHED, OGG_STREAMINFO_EOF)
FD_OK, FD_FRAME_CRC, FD_EOF, FD_MD5 = 0, 14, 15, 16
NO_PAGE = 0xFFFFFFFF


def _crc_table():
    t = []
    for b in range(256):
        c = b << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
        t.append(c)
    return t


_CRC = _crc_table()


def ogg_crc_bytewise(data, crc=0):
    """CRC-32, polynomial 0x04C11DB7, initial value 0, MSB first, no final xor"""
    for b in data:
        crc = ((crc << 8) & 0xFFFFFFFF) ^ _CRC[(crc >> 24) ^ b]
    return crc


_REV8 = bytes(int("{:08b}".format(b)[::-1], 2) for b in range(256))


def _rev32(x):
    return int("{:032b}".format(x)[::-1], 2)


def ogg_crc(data, crc=0):
    """the same checksum at C speed: it is zlib's CRC-32 with the bits of
    every byte and of the state mirrored, without zlib's initial value and
    final xor (tests/test_oggflac_port.py holds the two to each other)"""
    return _rev32(zlib.crc32(bytes(data).translate(_REV8), _rev32(crc) ^ 0xFFFFFFFF) ^ 0xFFFFFFFF)


# ------------------------------------------------------------------ muxer
def page(lacing, body, flags=0, granule=0, serial=1, sequence=0, checksum=None, version=0,
         magic=b"OggS"):
    head = (magic + bytes([version, flags]) + int(granule).to_bytes(8, "little", signed=True) +
            (serial & 0xFFFFFFFF).to_bytes(4, "little") +
            (sequence & 0xFFFFFFFF).to_bytes(4, "little"))
    tail = bytes([len(lacing)]) + bytes(lacing) + body
    if checksum is None:
        checksum = ogg_crc(head + b"\0\0\0\0" + tail)
    return head + checksum.to_bytes(4, "little") + tail


def lacing_of(n):
    """the lacing values of an n-byte packet (a 255 k one ends with a 0)"""
    return [255] * (n // 255) + [n % 255]


def mux(packets, segs_per_page=255, seed=None, eos=True, scramble=False, empty_page_after=None,
        trailing=b"", unfinished=b""):
    """packets -> image.  segs_per_page: segments per page, or with `seed` the
    upper end of a seeded random 1..segs_per_page per page.  scramble: another
    serial on every page, sequence numbers running backwards, no continuation
    flags.  empty_page_after: a zero-segment page after that page index.
    unfinished: bytes of a last packet without its terminator."""
    segs = []  # (lacing value, bytes, first of a packet)
    for p in packets:
        lv = lacing_of(len(p))
        for k, v in enumerate(lv):
            segs.append((v, p[255 * k:255 * k + v], k == 0))
    if unfinished:
        assert len(unfinished) % 255 == 0
        for k in range(len(unfinished) // 255):
            segs.append((255, unfinished[255 * k:255 * k + 255], k == 0))
    rng = random.Random(seed) if seed is not None else None
    groups, i = [], 0
    while i < len(segs):
        n = rng.randint(1, segs_per_page) if rng else segs_per_page
        groups.append(segs[i:i + n])
        i += n
    if empty_page_after is not None:
        groups.insert(empty_page_after + 1, [])
    if not groups:
        groups = [[]]
    out = []
    for k, g in enumerate(groups):
        flags = 0
        if g and not g[0][2] and not scramble:
            flags |= 1
        if k == 0 and not scramble:
            flags |= 2
        if eos and k == len(groups) - 1:
            flags |= 4
        out.append(page([s[0] for s in g], b"".join(s[1] for s in g), flags, granule=k,
                        serial=(0x1234567 * (k + 3)) if scramble else 1,
                        sequence=(len(groups) - k) if scramble else k))
    return b"".join(out) + trailing


def flac_packets(flac, header_packets=None, streaminfo_patch=None):
    """a .flac image -> (Ogg FLAC packets, number of header packets after the
    first): the mapping's first packet, one packet per further metadata block,
    one per frame"""
    blocks, body = oracle_port.split_flac(flac)
    assert blocks[0][0] == 0
    si = bytearray(blocks[0][1])
    if streaminfo_patch:
        streaminfo_patch(si)
    rest = blocks[1:]
    n = len(rest) if header_packets is None else header_packets
    first = (b"\x7fFLAC\x01\x00" + n.to_bytes(2, "big") + b"fLaC" +
             bytes([0x80 if not rest else 0]) + len(si).to_bytes(3, "big") + bytes(si))
    packets = [first]
    for k, (btype, payload) in enumerate(rest):
        last = 0x80 if k == len(rest) - 1 else 0
        packets.append(bytes([last | btype]) + len(payload).to_bytes(3, "big") + payload)
    start = len(flac) - len(body)
    d = oracle_port.decode_frames(flac)
    assert d["code"] == 0, d["code"]
    offs = [o for o, _ in d["offsets"]] + [None]
    for k in range(len(offs) - 1):
        packets.append(flac[start + offs[k]:(start + offs[k + 1]) if offs[k + 1] is not None
                            else len(flac)])
    return packets, len(rest)


# ---------------------------------------------------------------- decoder
def read_pages(image):
    """the page walk: -> (pages [(offset, lacing, body offset, flags)],
    ogg status, failing page index, its offset).  Stops after the
    end-of-stream page or at the first failure (status OGG_OK when the stream
    ended with its flag)."""
    pages, pos, n = [], 0, len(image)
    while True:
        idx = len(pages)
        if n - pos < 4:
            return pages, OGG_EOF, idx, pos
        if image[pos:pos + 4] != b"OggS":
            return pages, OGG_MAGIC, idx, pos
        if n - pos < 5:
            return pages, OGG_EOF, idx, pos
        if image[pos + 4] != 0:
            return pages, OGG_VERSION, idx, pos
        if n - pos < 27:
            return pages, OGG_EOF, idx, pos
        nseg = image[pos + 26]
        if n - pos < 27 + nseg:
            return pages, OGG_EOF, idx, pos
        lacing = list(image[pos + 27:pos + 27 + nseg])
        size = 27 + nseg + sum(lacing)
        if n - pos < size:
            return pages, OGG_EOF, idx, pos
        raw = image[pos:pos + size]
        if ogg_crc(raw[:22] + b"\0\0\0\0" + raw[26:]) != int.from_bytes(raw[22:26], "little"):
            return pages, OGG_CHECKSUM, idx, pos
        pages.append((pos, lacing, pos + 27 + nseg, image[pos + 5]))
        pos += size
        if image[pages[-1][0] + 5] & 4:
            return pages, OGG_OK, NO_PAGE, 0


def read_packets(image):
    """-> (complete packets, page count, status, failing page, its offset)"""
    pages, status, fail, fail_off = read_pages(image)
    packets, cur = [], []
    for _, lacing, body, _ in pages:
        for v in lacing:
            cur.append(image[body:body + v])
            body += v
            if v < 255:
                packets.append(b"".join(cur))
                cur = []
    return packets, len(pages), status, fail, fail_off


def parse_first_packet(p):
    """oggflac_read_streaminfo -> (ogg status, header packets, streaminfo dict)"""
    def short(n):
        return len(p) < n
    if short(1):
        return OGG_STREAMINFO_EOF, 0, None
    if p[0] != 0x7F:
        return OGG_PACKET_BYTE, 0, None
    if short(5):
        return OGG_STREAMINFO_EOF, 0, None
    if p[1:5] != b"FLAC":
        return OGG_SIGNATURE, 0, None
    if short(6):
        return OGG_STREAMINFO_EOF, 0, None
    if p[5] != 1:
        return OGG_MAJOR, 0, None
    if short(7):
        return OGG_STREAMINFO_EOF, 0, None
    if p[6] != 0:
        return OGG_MINOR, 0, None
    if short(9):
        return OGG_STREAMINFO_EOF, 0, None
    count = int.from_bytes(p[7:9], "big")
    if short(13):
        return OGG_STREAMINFO_EOF, count, None
    if p[9:13] != b"fLaC":
        return OGG_FLAC_SIGNATURE, count, None
    if short(14):
        return OGG_STREAMINFO_EOF, count, None
    if p[13] & 0x7F:
        return OGG_BLOCK_TYPE, count, None
    if short(51):
        return OGG_STREAMINFO_EOF, count, None
    s = p[17:51]
    x = int.from_bytes(s[10:18], "big")
    si = dict(min_block_size=int.from_bytes(s[0:2], "big"),
              max_block_size=int.from_bytes(s[2:4], "big"),
              min_frame_size=int.from_bytes(s[4:7], "big"),
              max_frame_size=int.from_bytes(s[7:10], "big"),
              sample_rate=x >> 44, channels=((x >> 41) & 7) + 1,
              bits_per_sample=((x >> 36) & 31) + 1, total_samples=x & ((1 << 36) - 1),
              md5=bytes(s[18:34]))
    return OGG_OK, count, si


_FRAME_CACHE = {}


def _decode_one_frame(packet, psi):
    """one FLAC frame from the packet's first byte, reads bounded by the
    packet -> (FD status, pcm int32 interleaved or None); remembered per
    packet, since the damage sweeps decode the same packets thousands of times"""
    key = (packet, psi.max_block_size, psi.sample_rate, psi.channels, psi.bits_per_sample)
    if key not in _FRAME_CACHE:
        if len(_FRAME_CACHE) > 20000:
            _FRAME_CACHE.clear()
        _FRAME_CACHE[key] = _decode_one_frame_now(packet, psi)
    return _FRAME_CACHE[key]


def _decode_one_frame_now(packet, psi):
    lib = oracle_port._dec_lib()
    ch = max(1, psi.channels)
    cap = max(1, psi.max_block_size) * ch
    pcm = np.zeros(cap, dtype=np.int32)
    offs = np.zeros(1, dtype=np.uint64)
    bss = np.zeros(1, dtype=np.uint32)
    nf, got = ctypes.c_size_t(), ctypes.c_uint64()
    # room for one frame only: the loop stops at the second (bytes after the
    # frame are never looked at by the reference)
    code = lib.flacport_decode_frames(packet, len(packet), ctypes.byref(psi), 1 << 40, 1,
                                      pcm.ctypes.data_as(ctypes.c_void_p), cap,
                                      offs.ctypes.data_as(ctypes.c_void_p),
                                      bss.ctypes.data_as(ctypes.c_void_p), 1,
                                      ctypes.byref(nf), ctypes.byref(got))
    if nf.value >= 1:
        return FD_OK, pcm[:int(bss[0]) * ch].copy()
    if code == oracle_port.FD_ERROR:
        code = loose_frame_status(packet, psi)
    return code, None


class _Bits(object):
    """MSB-first reads that raise EOFError past the end, as the reference's
    reader aborts to its br_try"""

    def __init__(self, data):
        self.v = int.from_bytes(data, "big")
        self.n = 8 * len(data)
        self.pos = 0

    def get(self, k):
        if self.pos + k > self.n:
            raise EOFError
        self.pos += k
        return (self.v >> (self.n - self.pos)) & ((1 << k) - 1)

    def get_signed(self, k):
        if k == 0 or k > 33:  # (sign + 2^32 - 1 magnitude bits / more than the reader has)
            raise EOFError
        return self.get(k)

    def unary(self, stop):
        q = 0
        while self.get(1) != stop:
            q += 1
        return q


def _crc16(data):
    crc = 0
    for b in data:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x8005) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def loose_frame_status(packet, psi):
    """A residual whose partition order does not divide the block: the frame
    decoder of this project rejects it (FD_ERROR, a documented limit: the
    reference predicts from a stale buffer there).  The reference reads on
    with partitions of block / 2^order values, rounded down, and fails further
    on: an error in a later subframe, the packet's end, or the CRC-16.  This
    walks the frame that way (its header passed already) -> what stops the
    reference; FD_ERROR stays for a frame that passes even its CRC-16."""
    r = _Bits(packet)
    try:
        r.get(16)
        bs_bits, sr_bits, assign, bps_bits = r.get(4), r.get(4), r.get(4), r.get(3)
        r.get(1)
        ones = r.unary(0)
        r.get(7 - ones)
        for _ in range(max(0, ones - 1)):
            r.get(8)
        if bs_bits == 0:
            bs = psi.max_block_size
        elif bs_bits == 1:
            bs = 192
        elif bs_bits <= 5:
            bs = 576 << (bs_bits - 2)
        elif bs_bits == 6:
            bs = r.get(8) + 1
        elif bs_bits == 7:
            bs = r.get(16) + 1
        else:
            bs = 256 << (bs_bits - 8)
        if sr_bits == 12:
            r.get(8)
        elif sr_bits in (13, 14):
            r.get(16)
        r.get(8)
        bps = {0: psi.bits_per_sample, 1: 8, 2: 12, 4: 16, 5: 20, 6: 24}[bps_bits]
        channels = 2 if 8 <= assign <= 10 else assign + 1
        for c in range(channels):
            sb = bps + 1 if (assign, c) in ((8, 1), (9, 0), (10, 1)) else bps
            r.get(1)
            t = r.get(6)
            if t == 0:
                kind, order = 0, 0
            elif t == 1:
                kind, order = 1, 0
            elif (t & 0x38) == 0x08:
                kind, order = 2, t & 7
            elif t & 0x20:
                kind, order = 3, (t & 0x1F) + 1
            else:
                return 13
            if r.get(1):
                sb = (sb - (r.unary(1) + 1)) & 0xFFFFFFFF
            if kind == 0:
                r.get_signed(sb)
            elif kind == 1:
                for _ in range(bs):
                    r.get_signed(sb)
            else:
                for _ in range(order):
                    r.get_signed(sb)
                if kind == 3:
                    prec = r.get(4) + 1
                    r.get_signed(5)
                    for _ in range(order):
                        r.get_signed(prec)
                method, porder = r.get(2), r.get(4)
                if method > 1:
                    return 11
                plen = bs >> porder
                for part in range(1 << porder):
                    cnt = plen if part else max(plen - order, 0)
                    rice = r.get(5 if method else 4)
                    esc = r.get(5) if rice == (31 if method else 15) else 0
                    for _ in range(cnt):
                        if esc:
                            r.get_signed(esc)
                        else:
                            r.unary(1)
                            r.get(rice)
                if kind == 2 and order > 4:
                    return 12
        if r.pos & 7:
            r.get(8 - (r.pos & 7))
        r.get(16)
    except EOFError:
        return FD_EOF
    return FD_FRAME_CRC if _crc16(packet[:r.pos // 8]) else oracle_port.FD_ERROR


def decode(image):
    """-> dict(ogg_status, status, pcm (bytes, as the reference writes them),
    samples (int32 interleaved), n_frames, pages, packets, fail_page,
    fail_offset, header_packets, streaminfo, md5)"""
    packets, npages, ostat, fail, fail_off = read_packets(image)
    out = dict(ogg_status=OGG_OK, status=FD_OK, pcm=b"", samples=np.zeros(0, np.int32), n_frames=0,
               pages=npages, packets=len(packets), fail_page=fail, fail_offset=fail_off,
               header_packets=0, streaminfo=None, md5=hashlib.md5(b"").digest())
    ran_out = ostat if ostat != OGG_OK else OGG_FINISHED
    if not packets:
        out["ogg_status"] = ran_out
        return out
    hstat, count, si = parse_first_packet(packets[0])
    out["header_packets"] = count
    if hstat != OGG_OK:
        out["ogg_status"] = hstat
        return out
    out["streaminfo"] = si
    if len(packets) < 1 + count:
        out["ogg_status"] = ran_out
        return out
    psi = oracle_port.PortStreamInfo()
    for k in ("min_block_size", "max_block_size", "min_frame_size", "max_frame_size",
              "sample_rate", "channels", "bits_per_sample", "total_samples"):
        setattr(psi, k, si[k])
    parts, raw = [], []
    for p in packets[1 + count:]:
        st, pcm = _decode_one_frame(p, psi)
        if st != FD_OK:
            out["status"] = st
            break
        parts.append(pcm)
        raw.append(oracle_port.pcm_bytes(pcm, si["bits_per_sample"]))
    out["n_frames"] = len(parts)
    out["samples"] = np.concatenate(parts) if parts else np.zeros(0, np.int32)
    out["pcm"] = b"".join(raw)
    out["md5"] = hashlib.md5(out["pcm"]).digest()
    if out["status"] == FD_OK:
        if ostat != OGG_OK:
            out["ogg_status"] = ostat
        elif si["md5"] != bytes(16) and si["md5"] != out["md5"]:
            out["status"] = FD_MD5
    return out


def message_class(d):
    """the outcome as the reference words it: "" for success, else "ogg:<n>",
    "flac:<n>" (FD status; 15 is its "I/O Error reading FLAC frame")"""
    if d["status"] not in (FD_OK, FD_MD5):
        return "flac:%d" % d["status"]
    if d["ogg_status"] != OGG_OK:
        return "ogg:%d" % d["ogg_status"]
    return "flac:16" if d["status"] == FD_MD5 else ""


def golden_class(d):
    """message_class as tests/golden/oggflac_vectors.json records it: the
    reference's standalone decoder prints nothing for a first-packet error"""
    c = message_class(d)
    if c.startswith("ogg:") and int(c[4:]) >= OGG_PACKET_BYTE:
        return "header"
    return c


def returncode(d):
    return 0 if message_class(d) == "" else 1
