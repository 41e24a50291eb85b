"""The Ogg FLAC encoder's page layout in plain Python:
what csrc/ogg_mux.hip must write, byte for byte.

Packets come from the native .flac image (oggflac_port.flac_packets): the
mapping's first packet with STREAMINFO, one packet per further metadata block
(VORBIS_COMMENT -- with WAVEFORMATEXTENSIBLE_CHANNEL_MASK when a mask is given
-- and PADDING when it is not empty), one per FLAC frame.  Segments are taken
in order; a page closes when it holds `page_segments` of them, when the last
segment of a header packet was placed on it, and with `page_per_packet` when
the last segment of any packet was.  The pages themselves are
oggflac_port.page's, the lacing values oggflac_port.lacing_of's.
"""
import hashlib

import numpy as np

import oggflac_port as op
import oracle_port

VORBIS_COMMENT, PADDING = 4, 1
MASK_TAG = "WAVEFORMATEXTENSIBLE_CHANNEL_MASK=0x%.4X"


def container_flac(flac, channel_mask=0):
    """the native image as the container carries it: the mask's comment in
    VORBIS_COMMENT, no empty PADDING block (the last-block flag moves up)"""
    blocks, body = oracle_port.split_flac(flac)
    out = []
    for btype, payload in blocks:
        if btype == PADDING and not payload:
            continue
        if btype == VORBIS_COMMENT and channel_mask:
            vlen = int.from_bytes(payload[:4], "little")
            assert payload[4 + vlen:] == bytes(4), "the native image carries no comments"
            tag = (MASK_TAG % channel_mask).encode("ascii")
            payload = (payload[:4 + vlen] + (1).to_bytes(4, "little") +
                       len(tag).to_bytes(4, "little") + tag)
        out.append((btype, payload))
    image = [b"fLaC"]
    for k, (btype, payload) in enumerate(out):
        last = 0x80 if k == len(out) - 1 else 0
        image.append(bytes([last | btype]) + len(payload).to_bytes(3, "big") + bytes(payload))
    return b"".join(image) + bytes(body)


def mux_flac(flac_image, frame_pcm_counts, serial, page_segments=255, page_per_packet=True,
             channel_mask=0, details=None):
    """-> the .oga image.  frame_pcm_counts: PCM frames of every FLAC frame
    (the granules).  details, a dict, receives pages, header_pages and
    page_offsets (per FLAC frame: byte of the page its packet begins on)."""
    S = page_segments or 255
    assert 1 <= S <= 255
    packets, n_header = op.flac_packets(container_flac(flac_image, channel_mask))
    n_header += 1
    assert len(packets) - n_header == len(frame_pcm_counts)
    pages, cur = [], []  # a page: [(lacing value, bytes, first of its packet, packet, last)]
    for k, p in enumerate(packets):
        lv = op.lacing_of(len(p))
        for j, v in enumerate(lv):
            last = j == len(lv) - 1
            cur.append((v, p[255 * j:255 * j + v], j == 0, k, last))
            if len(cur) == S or (last and (k < n_header or page_per_packet)):
                pages.append(cur)
                cur = []
    if cur:
        pages.append(cur)
    ends = np.cumsum([0] * n_header + list(frame_pcm_counts))  # PCM frames through packet k
    out, pos, begins, header_pages = [], 0, {}, 0
    for n, g in enumerate(pages):
        flags = (0 if g[0][2] else 1) | (2 if n == 0 else 0) | (4 if n == len(pages) - 1 else 0)
        done = [s[3] for s in g if s[4]]
        if g[0][3] < n_header:
            granule = 0
            header_pages += 1
        else:
            granule = int(ends[done[-1]]) if done else -1
        for s in g:
            if s[2]:
                begins[s[3]] = pos
        out.append(op.page([s[0] for s in g], b"".join(s[1] for s in g), flags, granule,
                           serial & 0xFFFFFFFF, n))
        pos += len(out[-1])
    if details is not None:
        details.update(pages=len(pages), header_pages=header_pages,
                       page_offsets=[begins[k] for k in range(n_header, len(packets))])
    return b"".join(out)


def encode(pcm, channels, bps, rate, ogg=None, frame_sizes=None, **flac_options):
    """oracle_port.encode, then mux_flac.  ogg: serial_number, page_segments,
    page_per_packet, channel_mask.  -> dict(image, pages, header_pages,
    page_offsets, pcm_frames, md5, flac)"""
    ogg = dict(ogg or {})
    flac, frames = oracle_port.encode(pcm, channels, bps, rate, frame_sizes=frame_sizes,
                                      **flac_options)
    counts = [n for _, n in frames]
    d = {}
    image = mux_flac(flac, counts, ogg.get("serial_number", 0), ogg.get("page_segments", 255),
                     ogg.get("page_per_packet", True), ogg.get("channel_mask", 0), d)
    d.update(image=image, pcm_frames=counts, flac=flac,
             md5=hashlib.md5(oracle_port.pcm_bytes(np.asarray(pcm, dtype=np.int32),
                                                   bps)).digest())
    return d
