"""GPU: libatgpu's Ogg FLAC encoder (the FLAC kernels + ogg_mux.hip) against
tests/oggflac_mux_port.py byte for byte, on every case of
tests/oggflac_enc_cases.py, through the host and the device entry.  The
golden file pins each image's sha256, and every golden image was accepted by
the reference's oggflacdec (tests/golden/make_oggflac_enc_golden.py)."""
import functools
import hashlib

import numpy as np
import pytest

import oggflac_enc_cases as cases
import oracle_port
from audiotools import _atgpu

pytestmark = pytest.mark.gpu
GOLD = cases.load_golden()["cases"]
SINGLE = list(cases.single_cases())
SINGLE_IDS = [c.name for c in SINGLE]


def ogg_options(case):
    return _atgpu.oggflac_enc_options(case.ogg["serial_number"], case.ogg["page_segments"],
                                      case.ogg["page_per_packet"], case.ogg["channel_mask"])


def batch_of(members, dtype=None):
    """the cases as one call's arguments: (pcm, tracks, ch, bps)"""
    ch, bps = members[0].ch, members[0].bps
    tracks, start = [], 0
    for c in members:
        if c.frame_sizes is not None:
            tracks.append((start, c.frames, np.asarray(c.frame_sizes, np.uint32)))
        else:
            tracks.append((start, c.frames))
        start += c.frames
    pcm = np.concatenate([c.pcm() for c in members] + [np.zeros(0, np.int32)])
    return pcm.astype(dtype or (np.int16 if bps <= 16 else np.int32)), tracks, ch, bps


def encode_host(eng, members, dtype=None):
    pcm, tracks, ch, bps = batch_of(members, dtype)
    opts = _atgpu.make_options(**members[0].flac_options())
    out, res, offs, fpcm = eng.encode_oggflac(opts, ogg_options(members[0]), pcm, tracks, ch, bps,
                                              cases.RATE)
    return [out[r.out_offset:r.out_offset + r.bytes].tobytes() for r in res], res, offs, fpcm


def encode_device(eng, members, dtype=None):
    pcm, tracks, ch, bps = batch_of(members, dtype)
    opts, ogg = _atgpu.make_options(**members[0].flac_options()), ogg_options(members[0])
    nf, nb = eng.oggflac_bounds(opts, ogg, tracks, ch, bps)
    d_pcm, d_out = eng.device_alloc(pcm.nbytes), eng.device_alloc(nb)
    try:
        if pcm.nbytes:
            eng.copy_to_device(d_pcm, pcm)
        fmt = _atgpu.PCM_S16 if pcm.dtype == np.int16 else _atgpu.PCM_S32
        res, offs, fpcm = eng.encode_oggflac_device(opts, ogg, d_pcm, fmt, tracks, ch, bps,
                                                    cases.RATE, d_out, nb, n_frames=nf)
        out = eng.copy_to_host(np.empty(max(nb, 1), np.uint8), d_out)
    finally:
        eng.device_free(d_pcm)
        eng.device_free(d_out)
    assert all(r.out_offset % 16 == 0 for r in res)
    return [out[r.out_offset:r.out_offset + r.bytes].tobytes() for r in res], res, offs, fpcm


def check(members, images, res, offs, fpcm):
    """images and results of one call against the port and the golden"""
    assert len(images) == len(res) == len(members)
    frame = 0
    for t, (c, img, r) in enumerate(zip(members, images, res)):
        d = c.port()
        assert r.status == 0, c.name
        assert r.bytes == len(d["image"]), c.name
        assert img == d["image"], c.name
        assert hashlib.sha256(img).hexdigest() == GOLD[c.name]["sha256"], c.name
        assert (r.pages, r.header_pages) == (d["pages"], d["header_pages"]), c.name
        assert r.serial_number == (members[0].ogg["serial_number"] + t) & 0xFFFFFFFF
        assert bytes(r.md5) == d["md5"], c.name
        assert (r.first_frame, r.n_frames) == (frame, len(d["pcm_frames"])), c.name
        assert [int(v) for v in offs[frame:frame + r.n_frames]] == d["page_offsets"], c.name
        assert [int(v) for v in fpcm[frame:frame + r.n_frames]] == d["pcm_frames"], c.name
        frame += r.n_frames
    assert frame == len(offs) == len(fpcm)


@functools.lru_cache(maxsize=None)
def host_images():
    """every single case through the host entry, once: {name: image}"""
    eng = _atgpu.engine()
    got = {}
    for c in SINGLE:
        images, res, offs, fpcm = encode_host(eng, [c])
        got[c.name] = (images, res, offs, fpcm)
    return got


@pytest.mark.parametrize("case", SINGLE, ids=SINGLE_IDS)
def test_host_entry_equals_port(case):
    check([case], *host_images()[case.name])


@pytest.mark.parametrize("case", SINGLE, ids=SINGLE_IDS)
def test_device_entry_equals_port(gpu_engine, case):
    check([case], *encode_device(gpu_engine, [case]))


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("entry", [encode_host, encode_device], ids=["host", "device"])
def test_batch_of_70(gpu_engine, entry, dtype):
    """more tracks than a wave, lengths 0 .. 3000, an empty one in the middle,
    serial numbers that wrap"""
    members = list(cases.batch_cases())
    images, res, offs, fpcm = entry(gpu_engine, members, dtype)
    check(members, images, res, offs, fpcm)
    assert res[16].serial_number == 0 and res[15].serial_number == 0xFFFFFFFF


def test_images_decode_on_the_gpu():
    from audiotools.decoders import decode_oggflac_batch
    members = SINGLE + list(cases.batch_cases())
    images = [host_images()[c.name][0][0] for c in SINGLE]
    images += encode_host(_atgpu.engine(), list(cases.batch_cases()))[0]
    for c, (r, pcm, _) in zip(members, decode_oggflac_batch(images)):
        assert (r.status, r.ogg_status) == (0, 0), c.name
        assert np.array_equal(pcm, c.pcm()), c.name
        assert r.pages == GOLD[c.name]["pages"], c.name


def test_native_encode_unchanged_around_an_ogg_batch(gpu_engine):
    """the same engine's native FLAC before and after: still the oracle's bytes"""
    by = {c.name: c for c in SINGLE}
    c = by["cuts:s7:fill"]
    pcm, tracks, ch, bps = batch_of([c])
    opts = _atgpu.make_options(**c.flac_options())
    want = oracle_port.encode(c.pcm(), ch, bps, cases.RATE, **c.flac_options())[0]

    def native():
        out, res, _, _ = gpu_engine.encode(opts, pcm, tracks, ch, bps, cases.RATE)
        return out[res[0].out_offset:res[0].out_offset + res[0].bytes].tobytes()

    assert native() == want
    assert "ogg_plan" not in gpu_engine.kernel_times()
    check([c], *encode_host(gpu_engine, [c]))
    times = gpu_engine.kernel_times()
    assert list(times)[-4:] == ["ogg_plan", "ogg_pages", "ogg_split", "ogg_crc"]
    assert native() == want
    assert "ogg_plan" not in gpu_engine.kernel_times()
    big = by["big65535"]
    check([big], *encode_device(gpu_engine, [big]))
    assert native() == want


@pytest.mark.parametrize("ogg", [dict(page_segments=256), dict(flags=2), dict(flags=3)],
                         ids=["segments", "flag2", "flag3"])
def test_invalid_options(gpu_engine, ogg):
    c = SINGLE[0]
    pcm, tracks, ch, bps = batch_of([c])
    opts = _atgpu.make_options(**c.flac_options())
    bad = _atgpu.oggflac_enc_options(**ogg)
    with pytest.raises(_atgpu.ATGError) as e:
        gpu_engine.encode_oggflac(opts, bad, pcm, tracks, ch, bps, cases.RATE)
    assert e.value.status == _atgpu.ATG_ERR_INVALID
    d_buf = gpu_engine.device_alloc(1 << 20)
    try:
        with pytest.raises(_atgpu.ATGError) as e:
            gpu_engine.encode_oggflac_device(opts, bad, d_buf, _atgpu.PCM_S16, tracks, ch, bps,
                                             cases.RATE, d_buf, 1 << 20)
        assert e.value.status == _atgpu.ATG_ERR_INVALID
    finally:
        gpu_engine.device_free(d_buf)


def test_invalid_flac_options_and_unwaited_ticket(gpu_engine):
    c = {c.name: c for c in SINGLE}["pad4096"]
    pcm, tracks, ch, bps = batch_of([c])
    ogg = ogg_options(c)
    for kw in (dict(block_size=0), dict(max_lpc_order=33), dict(padding_size=1 << 24)):
        opts = _atgpu.make_options(**dict(c.flac_options(), **kw))
        with pytest.raises(_atgpu.ATGError) as e:
            gpu_engine.encode_oggflac(opts, ogg, pcm, tracks, ch, bps, cases.RATE)
        assert e.value.status == _atgpu.ATG_ERR_INVALID
    # while an asynchronous FLAC batch is unwaited
    opts = _atgpu.make_options(**c.flac_options())
    nf, nb = gpu_engine.bounds(opts, tracks, ch, bps)
    d_pcm, d_out = gpu_engine.device_alloc(pcm.nbytes), gpu_engine.device_alloc(nb)
    try:
        gpu_engine.copy_to_device(d_pcm, pcm)
        ticket = gpu_engine.encode_device_async(opts, d_pcm, _atgpu.PCM_S16, tracks, ch, bps,
                                                cases.RATE, d_out, nb)
        try:
            with pytest.raises(_atgpu.ATGError) as e:
                gpu_engine.encode_oggflac(opts, ogg, pcm, tracks, ch, bps, cases.RATE)
            assert e.value.status == _atgpu.ATG_ERR_INVALID
        finally:
            gpu_engine.wait(ticket)
    finally:
        gpu_engine.device_free(d_pcm)
        gpu_engine.device_free(d_out)
    check([c], *encode_host(gpu_engine, [c]))
