"""CPU: the Ogg FLAC encoder's layout as
tests/oggflac_mux_port.py restates it -- pinned by the golden file whose every
image the reference's oggflacdec accepted, read back by oggflac_port, and
checked page by page by a walk that does not use the muxer -- and the host
side of the C ABI: atg_oggflac_batch_bounds."""
import ctypes
import hashlib

import numpy as np
import pytest

import oggflac_enc_cases as cases
import oggflac_mux_port as mp
import oggflac_port as op
import oracle_port
import signals
from audiotools import _atgpu

GOLD = cases.load_golden()
ALL = cases.all_cases()
IDS = [c.name for c in ALL]
SINGLE = list(cases.single_cases())


def test_every_case_has_a_golden_row():
    assert sorted(GOLD["cases"]) == sorted(IDS)
    assert GOLD["mult255_seed"] is not None


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_port_image_is_the_golden(case):
    d, g = case.port(), GOLD["cases"][case.name]
    assert len(d["image"]) == g["bytes"]
    assert hashlib.sha256(d["image"]).hexdigest() == g["sha256"]
    assert d["pages"] == g["pages"]
    assert hashlib.md5(oracle_port.pcm_bytes(case.pcm(), case.bps)).hexdigest() == g["pcm_md5"]


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_packets_read_back(case):
    d = case.port()
    want, _ = op.flac_packets(mp.container_flac(d["flac"], case.ogg["channel_mask"]))
    got, npages, status, fail, _ = op.read_packets(d["image"])
    assert status == op.OGG_OK and fail == op.NO_PAGE
    assert npages == d["pages"]
    assert got == want


def walk(image):
    """[(offset, flags, granule, serial, sequence, lacing)] of every page"""
    pages, status, _, _ = op.read_pages(image)
    assert status == op.OGG_OK
    out = []
    for off, lacing, _, flags in pages:
        out.append((off, flags, int.from_bytes(image[off + 6:off + 14], "little", signed=True),
                    int.from_bytes(image[off + 14:off + 18], "little"),
                    int.from_bytes(image[off + 18:off + 22], "little"), lacing))
    return out


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_page_rules(case):
    """section 1 of the layout, from the pages alone"""
    d = case.port()
    S, ppp = case.ogg["page_segments"] or 255, case.ogg["page_per_packet"]
    pages = walk(d["image"])
    n_header = 1 + int.from_bytes(d["image"][28 + 7:28 + 9], "big")
    ends = np.cumsum(d["pcm_frames"])
    packet, open_packet, header_pages, begins = 0, False, 0, []
    for n, (off, flags, granule, serial, seq, lacing) in enumerate(pages):
        assert serial == case.ogg["serial_number"] & 0xFFFFFFFF and seq == n
        assert bool(flags & 1) == open_packet, "continuation flag of page %d" % n
        assert bool(flags & 2) == (n == 0)
        assert bool(flags & 4) == (n == len(pages) - 1)
        assert 1 <= len(lacing) <= S
        header_page = packet < n_header
        header_pages += header_page
        last_done, closed = None, False
        for j, v in enumerate(lacing):
            assert not closed, "a segment after the one that closes page %d" % n
            if not open_packet and packet >= n_header:
                begins.append(off)
            open_packet = v == 255
            if v < 255:
                last_done = packet
                closed = packet < n_header or ppp
                packet += 1
            closed = closed or j + 1 == S
        if n < len(pages) - 1:
            assert closed, "page %d ends without a reason" % n
        if header_page:
            assert granule == 0
            assert last_done is None or last_done < n_header, "audio on a header page"
        else:
            assert granule == (-1 if last_done is None else int(ends[last_done - n_header]))
    assert not open_packet and packet == n_header + len(d["pcm_frames"])
    assert header_pages == d["header_pages"] and begins == d["page_offsets"]


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_port_decoder_accepts(case):
    r = op.decode(case.port()["image"])
    assert r["ogg_status"] == op.OGG_OK and r["status"] == op.FD_OK
    assert r["pcm"] == oracle_port.pcm_bytes(case.pcm(), case.bps)
    assert r["header_packets"] == (2 if case.padding else 1)


def test_shapes_the_cases_promise():
    by = {c.name: c for c in SINGLE}
    # one frame of exactly 255 k bytes: its lacing ends with a 0
    d = by["mult255:default"].port()
    _, body = oracle_port.split_flac(d["flac"])
    assert len(body) and len(body) % 255 == 0 and len(d["pcm_frames"]) == 1
    assert walk(d["image"])[-1][5][-1] == 0
    # a page whose first lacing value is the terminating 0 continues its packet
    assert walk(by["mult255:s1"].port()["image"])[-1][1] & 1
    # PADDING of 251 bytes: a 255-byte packet
    pk, _, _, _, _ = op.read_packets(by["pad251:s255"].port()["image"])
    assert len(pk[2]) == 255
    # no PADDING packet: VORBIS_COMMENT is the last block
    pk, _, _, _, _ = op.read_packets(by["pad0"].port()["image"])
    assert pk[1][0] == 0x84 and pk[0][7:9] == b"\0\1" and pk[2][:2] == b"\xff\xf8"
    assert b"WAVEFORMATEXTENSIBLE_CHANNEL_MASK=0x060F" in \
        op.read_packets(by["mask6x24"].port()["image"])[0][1]
    # packets over a page body, a header packet over pages, granules of sizes
    assert max(len(p) for p in op.read_packets(by["big8x24:default"].port()["image"])[0]) > 65025
    assert by["pad70000"].port()["header_pages"] == 4
    assert [p[2] for p in walk(by["sizes"].port()["image"])[-3:]] == [4096, 5096, 5101]
    assert walk(by["empty"].port()["image"])[-1][1] & 4
    assert any(p[2] == -1 for p in walk(by["cuts:s1:pp"].port()["image"]))
    assert any(sum(v < 255 for v in p[5]) > 1 for p in walk(by["cuts:s255:fill"].port()["image"]))


# ------------------------------------------------------------ the C ABI
def ogg_bounds(case_or_opts, ogg, tracks, ch, bps):
    lib = _atgpu.load_library()
    arr, n, _keep = _atgpu._track_array(tracks)
    nf, nb = ctypes.c_uint64(), ctypes.c_uint64()
    st = lib.atg_oggflac_batch_bounds(ctypes.byref(case_or_opts), ctypes.byref(ogg), arr, n, ch,
                                      bps, ctypes.byref(nf), ctypes.byref(nb))
    return st, nf.value, nb.value


def ogg_options(case):
    return _atgpu.oggflac_enc_options(case.ogg["serial_number"], case.ogg["page_segments"],
                                      case.ogg["page_per_packet"], case.ogg["channel_mask"])


def track_of(case):
    if case.frame_sizes is not None:
        return (0, case.frames, np.asarray(case.frame_sizes, np.uint32))
    return (0, case.frames)


@pytest.mark.parametrize("case", SINGLE, ids=[c.name for c in SINGLE])
def test_bounds_cover_noise(case):
    """white noise, the largest frames: the port's image fits the bound, and
    the frame count is atg_flac_batch_bounds'"""
    opts = _atgpu.make_options(**case.flac_options())
    st, nf, nb = ogg_bounds(opts, ogg_options(case), [track_of(case)], case.ch, case.bps)
    assert st == _atgpu.ATG_OK
    x = signals.noise(case.frames, case.ch, case.bps, 99) if case.frames else case.pcm()
    d = mp.encode(x, case.ch, case.bps, cases.RATE, case.ogg, frame_sizes=case.frame_sizes,
                  **case.flac_options())
    assert nb >= len(d["image"]) and nf == len(d["pcm_frames"])
    lib = _atgpu.load_library()
    arr, n, _keep = _atgpu._track_array([track_of(case)])
    f2 = ctypes.c_uint64()
    assert lib.atg_flac_batch_bounds(ctypes.byref(opts), arr, n, case.ch, case.bps,
                                     ctypes.byref(f2), None) == _atgpu.ATG_OK
    assert f2.value == nf


def test_bounds_cover_the_batch():
    batch = cases.batch_cases()
    opts = _atgpu.make_options(**batch[0].flac_options())
    tracks, start, total = [], 0, 0
    for c in batch:
        tracks.append((start, c.frames))
        start += c.frames
        x = signals.noise(c.frames, 2, 16, 7) if c.frames else c.pcm()
        total += (len(mp.encode(x, 2, 16, cases.RATE, c.ogg, **c.flac_options())["image"]) +
                  15) & ~15
    st, nf, nb = ogg_bounds(opts, ogg_options(batch[0]), tracks, 2, 16)
    assert st == _atgpu.ATG_OK and nb >= total
    assert nf == sum(-(-c.frames // 256) for c in batch)


@pytest.mark.parametrize("ogg,flac,ch,bps,status", [
    (dict(page_segments=256), {}, 2, 16, _atgpu.ATG_ERR_INVALID),
    (dict(flags=2), {}, 2, 16, _atgpu.ATG_ERR_INVALID),
    (dict(flags=0x80000001), {}, 2, 16, _atgpu.ATG_ERR_INVALID),
    ({}, dict(block_size=0), 2, 16, _atgpu.ATG_ERR_INVALID),
    ({}, dict(max_lpc_order=33), 2, 16, _atgpu.ATG_ERR_INVALID),
    ({}, dict(block_size=65536), 2, 16, _atgpu.ATG_ERR_UNSUPPORTED),
    ({}, {}, 9, 16, _atgpu.ATG_ERR_INVALID),
    ({}, {}, 2, 32, _atgpu.ATG_ERR_UNSUPPORTED),
    (dict(page_segments=0), {}, 2, 16, _atgpu.ATG_OK),
    (dict(page_segments=255, flags=1), {}, 2, 16, _atgpu.ATG_OK),
])
def test_bounds_option_validation(ogg, flac, ch, bps, status):
    opts = _atgpu.make_options(**dict(oracle_port.PRESETS["8"], **flac))
    st, _, _ = ogg_bounds(opts, _atgpu.oggflac_enc_options(**ogg), [(0, 10000)], ch, bps)
    assert st == status
    if status != _atgpu.ATG_OK:
        assert _atgpu.load_library().atg_last_error()


def test_bounds_null_options():
    lib = _atgpu.load_library()
    arr, n, _keep = _atgpu._track_array([(0, 100)])
    opts = _atgpu.make_options(**oracle_port.PRESETS["8"])
    assert lib.atg_oggflac_batch_bounds(ctypes.byref(opts), None, arr, n, 2, 16, None,
                                        None) == _atgpu.ATG_ERR_INVALID
    assert lib.atg_oggflac_batch_bounds(None, ctypes.byref(_atgpu.oggflac_enc_options()), arr, n,
                                        2, 16, None, None) == _atgpu.ATG_ERR_INVALID
