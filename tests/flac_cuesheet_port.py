"""A struct-only builder and reader of FLAC CUESHEET blocks and of the
metadata around them, written from the FLAC format description: what
tests/test_flac_cuesheet.py holds audiotools.flac's block against.  It knows
nothing of Sheets: a layout here is (catalog, [(number, ISRC or None, audio,
[(index number, CD frames)])])."""

import struct


def block_body(catalog, tracks, total_pcm_frames, sample_rate, is_cdda):
    """the block as set_cuesheet is to write it.  Offsets are CD frames
    (1/75 s) turned to PCM frames one by one, rounding down."""
    def pcm(cd_frames):
        return cd_frames * sample_rate // 75

    out = [(catalog or "").encode("ascii").ljust(128, b"\0"),
           struct.pack(">Q", 2 * sample_rate),
           bytes([0x80 if is_cdda else 0]) + b"\0" * 258,
           struct.pack(">B", len(tracks) + 1)]
    for number, isrc, audio, indexes in tracks:
        first = pcm(indexes[0][1])
        out.append(struct.pack(">QB", first, number))
        out.append((isrc or "").encode("ascii").ljust(12, b"\0"))
        out.append(bytes([0 if audio else 0x80]) + b"\0" * 13)
        out.append(struct.pack(">B", len(indexes)))
        for n, at in indexes:
            out.append(struct.pack(">QB", pcm(at) - first, n) + b"\0" * 3)
    # the lead-out
    out.append(struct.pack(">QB", total_pcm_frames, 170) + b"\0" * 12 + b"\0" * 14 + b"\0")
    return b"".join(out)


def parse_body(body):
    """-> (catalog bytes, lead-in, cd flag, [(offset, number, isrc bytes,
    track type, [(offset, number)])]) with the lead-out track included"""
    catalog = body[:128]
    lead_in, = struct.unpack_from(">Q", body, 128)
    cdda = body[136] >> 7
    assert body[136] & 0x7F == 0 and not any(body[137:395]), "reserved bits set"
    n, pos, tracks = body[395], 396, []
    for _ in range(n):
        offset, number = struct.unpack_from(">QB", body, pos)
        isrc = body[pos + 9:pos + 21]
        flags = body[pos + 21]
        assert flags & 0x3F == 0 and not any(body[pos + 22:pos + 35]), "reserved bits set"
        count = body[pos + 35]
        pos += 36
        indexes = []
        for _ in range(count):
            o, i = struct.unpack_from(">QB", body, pos)
            assert body[pos + 9:pos + 12] == b"\0\0\0"
            indexes.append((o, i))
            pos += 12
        tracks.append((offset, number, isrc, flags >> 7, indexes))
    assert pos == len(body), "bytes left behind the last track"
    return catalog, lead_in, cdda, tracks


def blocks(data):
    """a .flac file -> ([(type, body)], offset of the first frame)"""
    assert data[:4] == b"fLaC"
    pos, out = 4, []
    while True:
        last, kind = data[pos] >> 7, data[pos] & 0x7F
        size = int.from_bytes(data[pos + 1:pos + 4], "big")
        out.append((kind, data[pos + 4:pos + 4 + size]))
        pos += 4 + size
        if last:
            return out, pos


def build(block_list, frames):
    out = [b"fLaC"]
    for k, (kind, body) in enumerate(block_list):
        out.append(bytes([kind | (0x80 if k == len(block_list) - 1 else 0)]) +
                   len(body).to_bytes(3, "big") + body)
    return b"".join(out) + frames


def with_padding(data, size):
    """the file with a PADDING block of `size` bytes as its last block"""
    block_list, at = blocks(data)
    return build([b for b in block_list if b[0] != 1] + [(1, b"\0" * size)], data[at:])
