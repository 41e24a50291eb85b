"""The eight handle classes of audiotools._atgpu over their shared base
(_atgpu._Handle, csrc/host_common.h): kernel_times() before and after the
smallest real run of each, and close() twice.  One track of 100 stereo 16-bit
frames goes through every encoder; every decoder gets the image its encoder
made."""
import math

import numpy as np
import pytest

import signals
import tta_port

pytestmark = pytest.mark.gpu

CH, BPS, RATE, N = 2, 16, 44100, 100

STAGES = {
    "Engine": ["lpc_analyze", "subframe_search", "frame_decide", "track_scan", "frame_pack",
               "track_md5", "stream_header", "total"],
    "Decoder": ["dec_scan", "dec_parse", "dec_chain", "dec_subframe", "dec_emit", "dec_md5",
                "dec_total"],
    "AlacEncoder": ["alac_lpc", "alac_chain", "alac_decide", "alac_scan", "alac_pack",
                    "alac_total"],
    "AlacDecoder": ["adec_parse", "adec_chain", "adec_channel", "adec_interleave", "adec_total"],
    "TtaEncoder": ["tta_chain", "tta_size", "tta_pack", "tta_crc", "tta_total"],
    "TtaDecoder": ["ttad_crc", "ttad_parse", "ttad_chain", "ttad_out", "ttad_total"],
    "WvDecoder": ["wvd_parse", "wvd_decorr", "wvd_out", "wvd_total"],
    "WvEncoder": ["wv_prep", "wv_chain", "wv_md5", "wv_size", "wv_pack", "wv_total"],
}
# the single-stream handles: their last entry spans the whole run
SIMPLE = ("AlacEncoder", "AlacDecoder", "TtaEncoder", "TtaDecoder", "WvDecoder", "WvEncoder")


@pytest.fixture(scope="module")
def pcm():
    return signals.make("tone", N, CH, BPS, seed=3).astype(np.int16)


def _aligned(img):
    return img + b"\0" * (-len(img) % 4)


def _check(handle, want_pcm=None, got_pcm=None):
    name = type(handle).__name__
    times = handle.kernel_times()
    assert list(times) == STAGES[name]
    print(name, times)
    for v in times.values():
        assert math.isfinite(v) and v >= 0
    if name in SIMPLE:
        total = times[STAGES[name][-1]]
        assert all(total >= v for v in times.values())
    if want_pcm is not None:
        assert np.array_equal(got_pcm, want_pcm.astype(np.int32))
    handle.close()
    handle.close()
    assert not handle.handle


def _open(cls):
    h = cls(0)
    assert h.kernel_times() == {}
    return h


def test_flac_engine_and_decoder(pcm):
    from audiotools import _atgpu
    eng = _open(_atgpu.Engine)
    opts = _atgpu.make_options(block_size=4096, max_lpc_order=12,
                               min_residual_partition_order=0, max_residual_partition_order=6,
                               mid_side=True, exhaustive_model_search=True)
    out, res, _, _ = eng.encode(opts, pcm, [(0, N)], CH, BPS, RATE)
    assert res[0].status == 0
    img = out[res[0].out_offset:res[0].out_offset + res[0].bytes].tobytes()
    _check(eng)
    dec = _open(_atgpu.Decoder)
    _, si, _ = _atgpu.read_metadata(img)
    body = _aligned(img[si.frames_offset:])
    got, dres, _, _ = dec.decode(body, [_atgpu.dec_track(0, len(img) - si.frames_offset, si)])
    assert dres[0].status == 0
    _check(dec, pcm, got)


def test_alac_encoder_and_decoder(pcm):
    from audiotools import _atgpu
    enc = _open(_atgpu.AlacEncoder)
    out, res, fsb = enc.encode(enc.options(), pcm, [(0, N)], CH, BPS)
    assert res[0].status == 0
    mdat = out[res[0].out_offset:res[0].out_offset + res[0].bytes].tobytes()
    _check(enc)
    dec = _open(_atgpu.AlacDecoder)
    info = _atgpu.AlacInfo()
    info.max_samples_per_frame, info.bits_per_sample = 4096, BPS
    info.history_multiplier, info.initial_history, info.maximum_k = 40, 10, 14
    info.channels, info.sample_rate, info.total_frames = CH, RATE, N
    # the frames follow the mdat atom's 8-byte header
    track = _atgpu.alac_dec_track(0, len(mdat), info, start=8, remaining=N, frameset_bytes=fsb)
    got, dres, _, _ = dec.decode(_aligned(mdat), [track])
    assert dres[0].status == 0
    _check(dec, pcm, got)


def test_tta_encoder_and_decoder(pcm):
    from audiotools import _atgpu
    enc = _open(_atgpu.TtaEncoder)
    out, res, fsb = enc.encode(pcm, [(0, N)], CH, BPS, RATE)
    assert res[0].status == 0
    frames = out[res[0].out_offset:res[0].out_offset + res[0].bytes].tobytes()
    _check(enc)
    dec = _open(_atgpu.TtaDecoder)
    sizes = [int(x) for x in fsb]
    img = tta_port.header(CH, BPS, RATE, N) + tta_port.seektable(sizes) + frames
    st, info, sizes = _atgpu.tta_read_info(img)
    assert st == 0
    got, dres = dec.decode(_aligned(img), [_atgpu.tta_dec_track(0, len(img), info, sizes)])
    assert dres[0].status == 0
    _check(dec, pcm, got)


def test_wavpack_encoder_and_decoder(pcm):
    from audiotools import _atgpu
    enc = _open(_atgpu.WvEncoder)
    out, res, _ = enc.encode(enc.options(22050), pcm, [(0, N)], CH, 0x3, BPS, RATE)
    assert res[0].status == 0
    img = out[res[0].out_offset:res[0].out_offset + res[0].bytes].tobytes()
    _check(enc)
    dec = _open(_atgpu.WvDecoder)
    st, info, blocks = _atgpu.wv_read_info(img)
    assert st == 0
    got, dres = dec.decode(_aligned(img), [_atgpu.wv_dec_track(0, len(img), info, blocks)])
    assert dres[0].status == 0
    _check(dec, pcm, got)
