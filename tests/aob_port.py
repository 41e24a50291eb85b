"""A plain Python / numpy port of the DVD-Audio title decode: the sector walk
of the reference's src/decoders/aob.c (read_audio_packet), the title layout
and the packed-PCM un-swizzle of aobpcm.c.  It returns the fields of the C
ABI's atg_aob_sector and atg_aob_result (include/atgpu_dvda.h), and answers
in the terms of the reference's stand-alone decoder for the golden vectors.
Written from the rules, not from the kernels: the GPU is compared with it.
"""
import numpy as np

SECTOR = 2048
(OK, BAD_SECTOR, EOF, UNKNOWN_CODEC, MLP, UNSUPPORTED) = range(6)
(S_OK, S_SYNC, S_MARKER, S_SHORT, S_START_CODE, S_PACKET_END, S_AUDIO_HEADER, S_NEGATIVE,
 S_NO_AUDIO) = range(9)

BITS = {0: 16, 1: 20, 2: 24}
RATES = {0: 48000, 1: 96000, 2: 192000, 8: 44100, 9: 88200, 10: 176400}
CHANNELS = [1, 2, 3, 4, 3, 4, 5, 3, 4, 5, 4, 5, 6, 4, 5, 4, 5, 6, 5, 5, 6]
CHANNEL_MASK = [0x4, 0x3, 0x103, 0x33, 0xB, 0x10B, 0x3B, 0x7, 0x107, 0x37, 0xF, 0x10F, 0x3F,
                0x107, 0x37, 0xF, 0x10F, 0x3F, 0x3B, 0x37, 0x3F]
# 24 bit: byte i of a chunk in the file is byte ORDER24[channels][i] of the
# chunk's little-endian samples
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


def _bad(why):
    return {"status": why, "payload_offset": 0, "payload_length": 0, "codec_id": 0,
            "group_1_bps": 0, "group_1_rate": 0, "channel_assignment": 0}


class _Reader(object):
    """reads that fail past the sector's end, as the reference's substream"""

    def __init__(self, data):
        self.d, self.pos = data, 0

    def left(self):
        return len(self.d) - self.pos

    def take(self, n):
        if n > self.left():
            raise EOFError
        v = self.d[self.pos:self.pos + n]
        self.pos += n
        return v


def walk_sector(data):
    """one 2048-byte sector -> its record (a dict of atg_aob_sector's fields)"""
    assert len(data) == SECTOR
    r = _Reader(data)
    head = r.take(14)
    if head[:4] != b"\x00\x00\x01\xba":
        return _bad(S_SYNC)
    bits = "{:0112b}".format(int.from_bytes(head, "big"))
    markers = (bits[32:34], bits[37], bits[53], bits[69], bits[79], bits[102:104])
    if markers != ("01", "1", "1", "1", "1", "11"):
        return _bad(S_MARKER)
    r.take(int(bits[109:112], 2))
    rec = _bad(S_NO_AUDIO)
    pcm_fields = (0, 0, 0)
    while r.left():
        if r.left() < 6:
            return _bad(S_SHORT)
        h = r.take(6)
        if h[:3] != b"\x00\x00\x01":
            return _bad(S_START_CODE)
        length = (h[4] << 8) | h[5]
        if h[3] != 0xBD:
            if length > r.left():
                return _bad(S_PACKET_END)
            r.take(length)
            continue
        try:
            pad1 = r.take(3)[2]
            r.take(pad1)
            codec, _, _, pad2 = r.take(4)
            if codec == 0xA0:
                p = r.take(9)
                pcm_fields = (p[3] >> 4, p[4] >> 4, p[6])
                if pad2 < 9:
                    raise EOFError
                r.take(pad2 - 9)
            else:
                r.take(pad2)
        except EOFError:
            return _bad(S_AUDIO_HEADER)
        payload = length - (3 + pad1 + 4 + pad2)
        if payload < 0:
            return _bad(S_NEGATIVE)
        if payload > r.left():
            return _bad(S_PACKET_END)
        rec = {"status": S_OK, "payload_offset": r.pos, "payload_length": payload,
               "codec_id": codec, "group_1_bps": pcm_fields[0], "group_1_rate": pcm_fields[1],
               "channel_assignment": pcm_fields[2]}
        r.take(payload)
    return rec


def walk(image, first=0, count=None):
    n = len(image) // SECTOR - first if count is None else count
    return [walk_sector(image[(first + i) * SECTOR:(first + i + 1) * SECTOR]) for i in range(n)]


def title_result(records):
    """the sector records of a title -> (result dict, payload bytes per good
    sector)"""
    res = {"status": EOF, "stop_sector": 0, "sample_rate": 0, "bits_per_sample": 0,
           "channels": 0, "channel_mask": 0, "channel_assignment": 0, "good_frames": 0}
    if not records:
        return res
    bad = next((i for i, r in enumerate(records) if r["status"]), len(records))
    if bad == 0:
        res["status"] = BAD_SECTOR
        return res
    first = records[0]
    if first["codec_id"] != 0xA0:
        res["status"] = MLP if first["codec_id"] == 0xA1 else UNKNOWN_CODEC
        return res
    ca = first["channel_assignment"]
    res["channel_assignment"] = ca
    res["bits_per_sample"] = BITS.get(first["group_1_bps"], 0)
    res["sample_rate"] = RATES.get(first["group_1_rate"], 0)
    res["channels"] = CHANNELS[ca] if ca <= 20 else 0
    res["channel_mask"] = CHANNEL_MASK[ca] if ca <= 20 else 0
    if res["bits_per_sample"] not in (16, 24) or not res["sample_rate"] or not res["channels"]:
        res["status"] = UNSUPPORTED
        return res
    total = sum(r["payload_length"] for r in records[:bad])
    chunk = res["bits_per_sample"] // 8 * res["channels"] * 2
    res["good_frames"] = 2 * (total // chunk)
    res["stop_sector"] = bad
    res["status"] = BAD_SECTOR if bad < len(records) else OK
    return res


def unswizzle(stream, bits, channels):
    """the codec's bytes (whole chunks) -> interleaved int32 samples"""
    B = bits // 8
    chunk = B * channels * 2
    a = np.frombuffer(stream, dtype=np.uint8).reshape(-1, chunk)
    order = [i ^ 1 for i in range(chunk)] if bits == 16 else ORDER24[channels]
    le = np.zeros_like(a)
    le[:, order] = a          # sample byte order[i] is file byte i
    le = le.reshape(-1, B).astype(np.int64)
    v = sum(le[:, k] << (8 * k) for k in range(B))
    v -= (v >> (bits - 1)) << bits
    return v.astype(np.int32)


def decode(image, first=0, count=None):
    """a title (sectors [first, first + count) of image) -> (result, int32
    samples, sector records)"""
    recs = walk(image, first, count)
    res = title_result(recs)
    if not res["good_frames"]:
        return res, np.zeros(0, np.int32), recs
    stream = b"".join(
        image[(first + i) * SECTOR + r["payload_offset"]:
              (first + i) * SECTOR + r["payload_offset"] + r["payload_length"]]
        for i, r in enumerate(recs[:res["stop_sector"]]))
    chunk = res["bits_per_sample"] // 8 * res["channels"] * 2
    n = res["good_frames"] // 2 * chunk
    return res, unswizzle(stream[:n], res["bits_per_sample"], res["channels"]), recs


def track_frames(pts_ticks, sample_rate):
    """aob.c: (unsigned)round(pts_ticks * sample_rate / 90000), half away from 0"""
    return (2 * pts_ticks * sample_rate + 90000) // 180000


def pcm_bytes(samples, bits):
    """little-endian signed bytes, as the reference's stand-alone decoder writes"""
    x = np.asarray(samples, dtype=np.int64)
    B = bits // 8
    out = np.zeros((len(x), B), dtype=np.uint8)
    for k in range(B):
        out[:, k] = (x >> (8 * k)) & 0xFF
    return out.tobytes()


def reference_answer(image, pts_ticks, first=0):
    """What the reference's stand-alone decoder does with `pts_ticks` of the
    title that starts at sector `first` and runs to the image's end ->
    (PCM bytes, its stderr without the frame count line, status)."""
    res, x, _ = decode(image, first)
    return answer_from(res, x, pts_ticks)


def answer_from(res, x, pts_ticks):
    """the same from a title's result (a dict of atg_aob_result's fields) and
    its samples, whoever decoded it.  Deviations from the reference
    (documented in DESIGN): an MLP title and a header the reference's asserts
    abort on give no PCM here; a request past the end of the sectors gives
    the frames present (status EOF) where the reference replays its last
    packet."""
    if res["status"] == BAD_SECTOR and res["stop_sector"] == 0:
        return b"", "I/O error reading initialization packet\n*** Error getting next track\n", \
            BAD_SECTOR
    if res["status"] == UNKNOWN_CODEC:
        return b"", "*** Error getting next track\n", UNKNOWN_CODEC
    if res["status"] in (MLP, UNSUPPORTED, EOF):
        return b"", "", res["status"]
    want = track_frames(pts_ticks, res["sample_rate"])
    have = min(want, res["good_frames"])
    raw = pcm_bytes(x[:have * res["channels"]], res["bits_per_sample"])
    if want <= res["good_frames"]:
        return raw, "", OK
    if res["status"] == BAD_SECTOR:
        return raw, "I/O Error reading PCM packet\n", BAD_SECTOR
    return raw, "", EOF
