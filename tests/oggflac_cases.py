"""The Ogg FLAC cases shared by tests/golden/make_oggflac_golden.py and the
tests: every image is rebuilt from the committed .flac fixtures or from
oracle_port.encode of tests/signals.py signals with oggflac_port's
deterministic muxer (the golden file pins each image's sha256)."""
import functools
import json
import os

import oggflac_port as op
import oracle_port
import signals

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "golden", "fixtures")
LAYOUTS = {"p1": dict(segs_per_page=1), "p7": dict(segs_per_page=7),
           "p255": dict(segs_per_page=255), "rnd": dict(segs_per_page=40, seed=7)}
MATRIX_SHAPES = [(ch, bps) for ch in (1, 2, 8) for bps in (8, 16, 24)]


def load_golden():
    """tests/golden/oggflac_vectors.json with every sweep's rows expanded"""
    with open(os.path.join(HERE, "golden", "oggflac_vectors.json")) as f:
        gold = json.load(f)
    for sweep in gold["sweeps"].values():
        sweep["rows"] = [sweep["unique"][k] for k in sweep["index"]]
    return gold


def fixture(name):
    with open(os.path.join(FIXTURES, name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def tone_flac(channels, bps, frames=700, block=192, padding=0, kind="tone"):
    preset = dict(oracle_port.PRESETS["8"])
    preset.update(block_size=block, padding_size=padding)
    x = signals.make(kind, frames * block, channels, bps, seed=channels * 100 + bps)
    return oracle_port.encode(x, channels, bps, 44100, **preset)[0]


@functools.lru_cache(maxsize=None)
def source(name):
    if name == "allframes":
        return fixture("flac-allframes.flac")
    if name == "tone8":
        return fixture("tone8.flac")
    ch, bps = name[1:].split("x")
    return tone_flac(int(ch), int(bps))


def source_names():
    return ["allframes", "tone8"] + ["t%dx%d" % s for s in MATRIX_SHAPES]


def matrix_cases():
    for s in source_names():
        pk, _ = op.flac_packets(source(s))
        for lname, layout in LAYOUTS.items():
            yield "matrix:%s:%s" % (s, lname), op.mux(pk, **layout)


def _small(padding=0, frames=6):
    return tone_flac(2, 16, frames=frames, padding=padding)


def _patch_total0(si):
    si[13] &= 0xF0
    si[14:18] = bytes(4)


def _patch_md5_zero(si):
    si[18:34] = bytes(16)


def _patch_md5_wrong(si):
    si[18] ^= 0x55


def edge_cases():
    """name -> image; the lacing edges, ignored fields and stream ends"""
    out = {}
    for pad in (761, 65021, 70000):
        pk, nh = op.flac_packets(_small(pad))
        assert len(pk[nh]) == pad + 4
        out["lacing:packet%d" % (pad + 4)] = op.mux(pk)
    big = tone_flac(8, 24, frames=1, block=4096, kind="noise")
    pk, _ = op.flac_packets(big)
    out["lacing:bigframe"] = op.mux(pk)
    pk, nh = op.flac_packets(_small())
    a = 1 + nh  # the first audio packet
    out["lacing:zero_segment_page"] = op.mux(pk, segs_per_page=2, empty_page_after=1)
    out["lacing:junk_tail"] = op.mux(pk[:a] + [p + bytes(range(37)) for p in pk[a:]])
    out["lacing:empty_packet"] = op.mux(pk[:a + 2] + [b""] + pk[a + 2:])
    out["lacing:two_frames"] = op.mux(pk[:a + 1] + [pk[a + 1] + pk[a + 2]] + pk[a + 3:])
    for cut in (100, 1, 2):
        q = list(pk)
        q[a + 2] = q[a + 2][:-cut]
        out["lacing:cut%d" % cut] = op.mux(q, segs_per_page=3)
    out["ignored:scrambled"] = op.mux(pk, segs_per_page=2, scramble=True)
    out["end:no_eos"] = op.mux(pk, segs_per_page=3, eos=False)
    out["end:garbage"] = op.mux(pk, segs_per_page=3, trailing=b"garbage after the last page" * 9)
    out["end:unfinished_packet"] = op.mux(pk, segs_per_page=3, unfinished=bytes(510))
    for name, patch in (("total0", _patch_total0), ("md5_zero", _patch_md5_zero),
                        ("md5_wrong", _patch_md5_wrong)):
        out["end:" + name] = op.mux(op.flac_packets(_small(), streaminfo_patch=patch)[0],
                                    segs_per_page=5)
    return out


def header_cases():
    """name -> image; the first packet and the header-packet count"""
    flac = _small(761)
    pk, nh = op.flac_packets(flac)
    out = {"header:good": op.mux(pk, segs_per_page=4)}
    for name, at in (("packet_byte", 0), ("signature", 2), ("major", 5), ("minor", 6),
                     ("flac_signature", 10), ("block_type", 13)):
        first = bytearray(pk[0])
        first[at] ^= 0x01
        out["header:" + name] = op.mux([bytes(first)] + pk[1:], segs_per_page=4)
    out["header:short20"] = op.mux([pk[0][:20]] + pk[1:], segs_per_page=4)
    out["header:count_plus2"] = op.mux(op.flac_packets(flac, header_packets=nh + 2)[0],
                                       segs_per_page=4)
    out["header:count_60000"] = op.mux(op.flac_packets(flac, header_packets=60000)[0],
                                       segs_per_page=4)
    good = out["header:good"]
    for name, at in (("page_magic", 1), ("page_version", 4), ("page_crc", 23)):
        b = bytearray(good)
        b[at] ^= 0x10
        out["header:" + name] = bytes(b)
    out["header:spanning"] = op.mux(pk, segs_per_page=1)
    first = pk[0] + bytes(300)  # the first packet itself over three pages
    out["header:first_spanning"] = op.mux([first] + pk[1:], segs_per_page=1)
    out["header:empty_file"] = b""
    out["header:no_packets"] = op.mux([], segs_per_page=1)
    return out


def with_comment(mask_text):
    """a stream whose VORBIS_COMMENT header packet carries the channel mask tag"""
    pk, nh = op.flac_packets(_small())
    vendor = b"oggflac cases"
    line = b"WAVEFORMATEXTENSIBLE_CHANNEL_MASK=" + mask_text
    body = (len(vendor).to_bytes(4, "little") + vendor + (1).to_bytes(4, "little") +
            len(line).to_bytes(4, "little") + line)
    comment = bytes([0x80 | 4]) + len(body).to_bytes(3, "big") + body
    first = bytearray(pk[0])
    first[7:9] = (nh + 1).to_bytes(2, "big")
    return op.mux([bytes(first), comment] + pk[1:], segs_per_page=4)


@functools.lru_cache(maxsize=None)
def damage_base():
    pk, _ = op.flac_packets(source("allframes"))
    return tuple(pk), op.mux(pk, segs_per_page=3)


def flip(image, bit):
    b = bytearray(image)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


def raw_flips():
    img = damage_base()[1]
    return [flip(img, k) for k in range(8 * len(img))]


def raw_truncations():
    img = damage_base()[1]
    return [img[:n] for n in range(len(img))]


def packet_flips():
    """every single-bit flip of every packet, under valid page checksums"""
    pk = list(damage_base()[0])
    out = []
    for i, p in enumerate(pk):
        for k in range(8 * len(p)):
            out.append(op.mux(pk[:i] + [flip(p, k)] + pk[i + 1:], segs_per_page=3))
    return out


TONE8_FLIPS = 4000


@functools.lru_cache(maxsize=None)
def tone8_base():
    pk, nh = op.flac_packets(source("tone8"))
    return tuple(pk), 1 + nh + 1  # the second audio packet


def tone8_flips():
    pk, at = tone8_base()
    pk = list(pk)
    assert 8 * len(pk[at]) >= TONE8_FLIPS
    return [op.mux(pk[:at] + [flip(pk[at], k)] + pk[at + 1:], segs_per_page=255)
            for k in range(TONE8_FLIPS)]


SWEEPS = {"raw_flips": raw_flips, "raw_truncations": raw_truncations,
          "packet_flips": packet_flips, "tone8_flips": tone8_flips}


def single_cases():
    out = dict(matrix_cases())
    out.update(edge_cases())
    out.update(header_cases())
    return out
