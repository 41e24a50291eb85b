"""Synthetic DVD-Audio material for the tests: AOB sector images with the
packed-PCM codec (or an MLP-typed / unknown first packet), and whole
AUDIO_TS directories (AOB files, AUDIO_TS.IFO, ATS_01_0.IFO) that
audiotools.dvda parses back.

Everything is made from a small dict of parameters (`spec`) and a seed, so
the golden file keeps specs and no AOB file is committed.

Sector layout, as the reference's src/decoders/aob.c reads it:
  pack header (14 bytes, sync 0x000001BA, six marker fields), `stuffing`
  bytes, then packets `00 00 01 <id> <len16>` tiling the sector exactly.
  The audio packet (id 0xBD): 2 bytes, pad1 size, pad1, codec id, CRC, 1
  byte, pad2 size, pad2 (for codec 0xA0 its first 9 bytes are the PCM
  header), payload.  The rest of the sector is one 0xBE padding packet.
"""
import os
import struct

import numpy as np

SECTOR = 2048
PCM, MLP = 0xA0, 0xA1

# byte i of a 24-bit chunk in the file is byte ORDER24[ch][i] of the chunk's
# little-endian samples (the data of the format; csrc/aob_common.h has the
# same table)
ORDER24 = {
    1: [2, 1, 5, 4, 0, 3],
    2: [2, 1, 5, 4, 8, 7, 11, 10, 0, 3, 6, 9],
    3: [8, 7, 17, 16, 6, 15, 2, 1, 5, 4, 11, 10, 14, 13, 0, 3, 9, 12],
    4: [8, 7, 11, 10, 20, 19, 23, 22, 6, 9, 18, 21, 2, 1, 5, 4, 14, 13, 17, 16, 0, 3, 12, 15],
    5: [8, 7, 11, 10, 14, 13, 23, 22, 26, 25, 29, 28, 6, 9, 12, 21, 24, 27, 2, 1, 5, 4, 17, 16,
        20, 19, 0, 3, 15, 18],
    6: [8, 7, 11, 10, 26, 25, 29, 28, 6, 9, 24, 27, 2, 1, 5, 4, 14, 13, 17, 16, 20, 19, 23, 22,
        32, 31, 35, 34, 0, 3, 12, 15, 18, 21, 30, 33],
}
CHANNELS = [1, 2, 3, 4, 3, 4, 5, 3, 4, 5, 4, 5, 6, 4, 5, 4, 5, 6, 5, 5, 6]
CHANNEL_MASK = [0x4, 0x3, 0x103, 0x33, 0xB, 0x10B, 0x3B, 0x7, 0x107, 0x37, 0xF, 0x10F, 0x3F,
                0x107, 0x37, 0xF, 0x10F, 0x3F, 0x3B, 0x37, 0x3F]
SAMPLE_RATE = {0: 48000, 1: 96000, 2: 192000, 8: 44100, 9: 88200, 10: 176400}
BPS_CODE = {16: 0, 20: 1, 24: 2}
# the lowest channel assignment of every channel count
ASSIGNMENT = {1: 0, 2: 1, 3: 2, 4: 3, 5: 6, 6: 12}


def file_order(bits, channels):
    """byte i of a chunk in the file is byte file_order[i] of its samples"""
    if bits == 16:
        return [i ^ 1 for i in range(4 * channels)]
    return ORDER24[channels]


def swizzle(samples, bits, channels):
    """interleaved samples (an even number of frames) -> the codec's bytes"""
    x = np.asarray(samples, dtype=np.int64)
    B = bits // 8
    chunk = B * channels * 2
    assert len(x) % (2 * channels) == 0
    le = np.zeros((len(x), B), dtype=np.uint8)
    for k in range(B):
        le[:, k] = (x >> (8 * k)) & 0xFF
    le = le.reshape(-1, chunk)
    return le[:, file_order(bits, channels)].tobytes()


def pack_header(stuffing=0, pts=0):
    """14 bytes: 32u sync, 2u 01, 3u, 1u 1, 15u, 1u 1, 15u, 1u 1, 9u, 1u 1,
    22u, 2u 11, 5 bits, 3u stuffing count"""
    bits = "{:032b}".format(0x000001BA) + "01" + "{:03b}".format((pts >> 30) & 7) + "1" + \
        "{:015b}".format((pts >> 15) & 0x7FFF) + "1" + "{:015b}".format(pts & 0x7FFF) + "1" + \
        "{:09b}".format(0) + "1" + "{:022b}".format(0x1890) + "11" + "11111" + \
        "{:03b}".format(stuffing)
    assert len(bits) == 112
    return int(bits, 2).to_bytes(14, "big") + b"\xff" * stuffing


def packet(stream_id, body):
    return b"\x00\x00\x01" + bytes([stream_id]) + struct.pack(">H", len(body)) + body


def audio_packet(payload, codec=PCM, bps_code=0, rate_code=8, assignment=1, pad1=0, pad2=9):
    """a private-stream-1 packet; pad2 >= 9 for the PCM codec"""
    body = b"\x81\x80" + bytes([pad1]) + b"\xff" * pad1 + bytes([codec, 0x00, 0x00, pad2])
    if codec == PCM:
        assert pad2 >= 9
        body += struct.pack(">HBBBBBBB", 0x0004, 0x00, (bps_code << 4) | 0x0F,
                            (rate_code << 4) | 0x0F, 0x00, assignment, 0x00, 0x00)
        body += b"\x00" * (pad2 - 9)
    else:
        body += b"\x00" * pad2
    return packet(0xBD, body + payload)


def sector(payload, stuffing=0, before=(), after=(), decoy=None, **audio):
    """one 2048-byte sector.  before / after: [(stream id, body length)] of
    packets round the audio packet; decoy: the payload of a first 0xBD packet
    the reader must drop (the sector's payload is its last audio packet's)"""
    s = pack_header(stuffing)
    for sid, n in before:
        s += packet(sid, b"\x55" * n)
    if decoy is not None:
        s += audio_packet(decoy, **audio)
    s += audio_packet(payload, **audio)
    for sid, n in after:
        s += packet(sid, b"\xaa" * n)
    rest = SECTOR - len(s)
    assert rest == 0 or rest >= 6, "no room for the padding packet (%d left)" % rest
    if rest:
        s += packet(0xBE, b"\xff" * (rest - 6))
    return s


def spec_samples(spec):
    """the source samples of a spec: full-scale noise from its seed, as many
    whole chunks as its payload bytes hold -> (int32 array, stream bytes)"""
    rng = np.random.default_rng(spec["seed"])
    bits, ch = spec["bits"], CHANNELS[spec["assignment"]]
    total = sum(spec["payloads"])
    chunk = bits // 8 * ch * 2
    n = total // chunk * 2 * ch
    x = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=n, dtype=np.int64).astype(np.int32)
    tail = rng.integers(0, 256, size=total - total // chunk * chunk, dtype=np.uint8).tobytes()
    return x, swizzle(x, bits, ch) + tail


def _per_sector(spec, key, default, i):
    v = spec.get(key, default)
    return v[i % len(v)] if isinstance(v, (list, tuple)) else v


def aob_image(spec):
    """spec -> (image bytes, source samples).  Keys: seed, bits (16 / 24),
    assignment, rate (code, default 8), payloads (bytes per sector), and per
    sector (a value or a list that is cycled) pad1, pad2, stuffing; before /
    after: {sector: [(id, length)]}; decoy: {sector: bytes length}; codec:
    the first sector's codec id when not PCM (its payload is then noise)."""
    x, stream = spec_samples(spec)
    out, pos = [], 0
    for i, n in enumerate(spec["payloads"]):
        codec = spec.get("codec", PCM) if i == 0 else PCM
        decoy = spec.get("decoy", {}).get(str(i))
        out.append(sector(
            stream[pos:pos + n], stuffing=_per_sector(spec, "stuffing", 0, i),
            before=spec.get("before", {}).get(str(i), ()),
            after=spec.get("after", {}).get(str(i), ()),
            decoy=None if decoy is None else b"\x33" * decoy, codec=codec,
            bps_code=BPS_CODE[spec["bits"]], rate_code=spec.get("rate", 8),
            assignment=spec["assignment"], pad1=_per_sector(spec, "pad1", 0, i),
            pad2=_per_sector(spec, "pad2", 9, i)))
        pos += n
    return b"".join(out), x


def flip(image, bit):
    b = bytearray(image)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


def header_bits(spec):
    """the bit numbers of a spec's image that a reader looks at outside the
    audio: every byte but the payloads of the audio packets and the bodies of
    the other packets (which are skipped unread)"""
    image, _ = aob_image(spec)
    bits = []
    for s in range(len(image) // SECTOR):
        sec = image[s * SECTOR:(s + 1) * SECTOR]
        keep = list(range(14 + (sec[13] & 7)))
        pos = len(keep)
        while pos < SECTOR:
            length = (sec[pos + 4] << 8) | sec[pos + 5]
            head = 6
            if sec[pos + 3] == 0xBD:
                pad1 = sec[pos + 8]
                head = 6 + 3 + pad1 + 4 + sec[pos + 9 + pad1 + 3]
            keep += range(pos, pos + head)
            pos += 6 + length
        bits += [8 * (s * SECTOR + byte) + k for byte in keep for k in range(8)]
    return bits


# ------------------------------------------------------------------ discs
def _ifo_audio_ts(titlesets):
    b = b"DVDAUDIO-AMG" + struct.pack(">I", 0) + b"\0" * 12 + struct.pack(">IH", 1, 0x12)
    b += b"\0" * 4 + struct.pack(">HHB", 1, 1, 0) + b"\0" * 4 + struct.pack(">BI", 0, 0)
    b += b"\0" * 10 + struct.pack(">BB", 0, titlesets) + b"test".ljust(40, b"\0")
    return b.ljust(SECTOR, b"\0")


def _ifo_ats(titles):
    """titles: [{"pts_length", "tracks": [(first_pts, pts_length, first_sector,
    last_sector)]}]; one index per track"""
    head = struct.pack(">HHI", len(titles), 0, 0)
    tables, offset = [], 8 + 8 * len(titles)
    offsets = []
    for t in titles:
        tr = t["tracks"]
        tab = b"\0\0" + struct.pack(">BBI", len(tr), len(tr), t["pts_length"]) + b"\0" * 4
        tab += struct.pack(">H", 16 + 20 * len(tr)) + b"\0\0"
        for i, (first_pts, pts_length, _, _) in enumerate(tr):
            tab += b"\0" * 4 + struct.pack(">BBII", i + 1, 0, first_pts, pts_length) + b"\0" * 6
        for _, _, first, last in tr:
            tab += struct.pack(">III", 0x01000000, first, last)
        offsets.append(offset)
        tables.append(tab)
        offset += len(tab)
    for i, o in enumerate(offsets):
        head += struct.pack(">BBHI", 0x80 | (i + 1), 0, 0, o)
    body = head + b"".join(tables)
    return b"DVDAUDIO-ATS".ljust(SECTOR, b"\0") + body.ljust(SECTOR, b"\0")


def write_disc(path, titles, split_at=None, lower=False):
    """Write an AUDIO_TS directory of one titleset.  titles: [(spec, [track
    frames])]; the titles' sectors follow each other in ATS_01_1.AOB, or with
    split_at = N the first N sectors go there and the rest to ATS_01_2.AOB.
    Returns [{"spec", "samples", "first_sector", "tracks": [(first frame,
    frames, pts length)]}]."""
    os.makedirs(path, exist_ok=True)
    image, info, ifo = b"", [], []
    for spec, track_frames in titles:
        img, x = aob_image(spec)
        first = len(image) // SECTOR
        last = first + len(img) // SECTOR - 1
        rate = SAMPLE_RATE[spec.get("rate", 8)]
        tracks, rows, pos, pts = [], [], 0, 0
        for n in track_frames:
            ticks = n * 90000 // rate
            assert ticks * rate == n * 90000, "track lengths must be whole PTS ticks"
            tracks.append((pos, n, ticks))
            rows.append((pts, ticks, first, last))
            pos += n
            pts += ticks
        ifo.append({"pts_length": pts, "tracks": rows})
        info.append({"spec": spec, "samples": x, "first_sector": first, "tracks": tracks})
        image += img
    name = (lambda s: s.lower()) if lower else (lambda s: s)
    cut = len(image) if split_at is None else split_at * SECTOR
    for i, part in enumerate([image[:cut], image[cut:]]):
        if part:
            with open(os.path.join(path, name("ATS_01_%d.AOB" % (i + 1))), "wb") as f:
                f.write(part)
    with open(os.path.join(path, name("AUDIO_TS.IFO")), "wb") as f:
        f.write(_ifo_audio_ts(1))
    with open(os.path.join(path, name("ATS_01_0.IFO")), "wb") as f:
        f.write(_ifo_ats(ifo))
    return info
