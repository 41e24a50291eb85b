"""The predictor order of the first subframe of every frame of a FLAC image
(test helper: which orders a signal makes the exhaustive search choose).
Only the frame header and the first subframe's type byte are read, so no
residual is parsed."""


def _frame_header_len(b, p):
    assert b[p] == 0xFF and (b[p + 1] & 0xFE) == 0xF8, "no frame sync at %d" % p
    bs_code, sr_code = b[p + 2] >> 4, b[p + 2] & 15
    q = p + 4
    lead = b[q]  # UTF-8 coded frame / sample number
    n = 0
    while lead & (0x80 >> n):
        n += 1
    q += max(n, 1)
    q += {6: 1, 7: 2}.get(bs_code, 0)
    q += {12: 1, 13: 2, 14: 2}.get(sr_code, 0)
    return q + 1 - p  # CRC-8


def first_subframe_orders(image, frame_offsets):
    """[(kind, order)] per frame; kind in 'constant', 'verbatim', 'fixed', 'lpc'.
    image: a whole FLAC stream; frame_offsets: from the first frame's start."""
    import oracle_port
    image = oracle_port.split_flac(image)[1]
    out = []
    for off in frame_offsets:
        t = (image[off + _frame_header_len(image, off)] >> 1) & 0x3F
        if t == 0:
            out.append(("constant", 0))
        elif t == 1:
            out.append(("verbatim", 0))
        elif 8 <= t <= 12:
            out.append(("fixed", t - 8))
        else:
            assert t >= 32
            out.append(("lpc", t - 31))
    return out
