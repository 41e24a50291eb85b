"""GPU: audiotools.encoders.encode_wavpack / encode_wavpack_batch and
WavPackAudio.from_pcm with an encoding function, against the reference
encoder's vectors (tests/golden/wavpack_enc_vectors.json, wavpack_images.bin)
and tests/wavpack_enc_port.py."""
import hashlib
import os

import numpy as np
import pytest

import wavpack_cases as cases
import wavpack_enc_cases as enc_cases
import wavpack_enc_port as port
import wavpack_port as dec

pytestmark = pytest.mark.gpu
G, IMAGES = cases.load_vectors()
VECTORS = enc_cases.load_vectors()


def drain(pcmreader):
    got = []
    while True:
        fl = pcmreader.read(4096)
        if not len(fl):
            break
        got.append(fl.samples)
    pcmreader.close()
    return np.concatenate(got) if got else np.zeros(0, np.int32)


def reader(case):
    import audiotools
    name, opts, ch, bps, rate, x = case
    return audiotools.FrameListReader(x, rate, ch, bps, port.parse_options(opts)["mask"])


def keywords(opts):
    kw = port.parse_options(opts)
    return dict(block_size=kw["block_size"], false_stereo=kw["false"], wasted_bits=kw["wasted"],
                joint_stereo=kw["joint"], correlation_passes=kw["passes"])


def read(path):
    with open(path, "rb") as f:
        return f.read()


def matches(image, name):
    return len(image) == VECTORS[name]["bytes"] and \
        hashlib.md5(image).hexdigest() == VECTORS[name]["md5"]


def test_encode_wavpack_writes_the_vectors(tmp_path):
    from audiotools import encoders
    for name in ("false_ded_p16", "chan6_3F_fjw_p16", "stereo_b8_blocks", "long_p5_mono"):
        case = enc_cases.by_name()[name]
        fn = str(tmp_path / (name + ".wv"))
        assert encoders.encode_wavpack(fn, reader(case), **keywords(case[1])) is None
        assert matches(read(fn), name), name
    src = {c[0]: c for c in cases.cases()}
    for name in ("empty_c2", "rate12345_c3", "noise_p16_j_b24"):
        fn = str(tmp_path / (name + ".wv"))
        encoders.encode_wavpack(fn, reader(src[name]), **keywords(src[name][1]))
        assert read(fn) == IMAGES[name], name


def test_encode_wavpack_batch_writes_the_vectors(tmp_path):
    from audiotools import encoders
    for names in (["long_p16_j1", "exact_multiple", "one_frame"],
                  ["false_ede_p16", "false_ded_p16"]):
        group = [enc_cases.by_name()[n] for n in names]
        assert len({tuple(c[1]) for c in group}) == 1
        files = [str(tmp_path / (n + ".wv")) for n in names]
        encoders.encode_wavpack_batch(files, [reader(c) for c in group], **keywords(group[0][1]))
        for fn, name in zip(files, names):
            assert matches(read(fn), name), name
    with pytest.raises(ValueError):
        encoders.encode_wavpack_batch(files[:2], [reader(group[0]),
                                                  reader(enc_cases.by_name()["long_p5_mono"])], 56)


def test_total_pcm_frames(tmp_path):
    from audiotools import encoders
    case = enc_cases.by_name()["chan4_107"]
    frames = len(case[5]) // 4
    fn = str(tmp_path / "t.wv")
    encoders.encode_wavpack(fn, reader(case), total_pcm_frames=frames, **keywords(case[1]))
    assert matches(read(fn), "chan4_107")
    # a different total is written as declared (from the reference's source:
    # its stand-alone encoder cannot reach this path)
    encoders.encode_wavpack(fn, reader(case), total_pcm_frames=7, **keywords(case[1]))
    kw = port.parse_options(case[1])
    assert read(fn) == port.encode(case[5], 4, 0x107, 16, 44100, kw["block_size"], kw["passes"],
                                   kw["joint"], kw["false"], kw["wasted"], total_pcm_frames=7)


def test_refused_arguments(tmp_path):
    from audiotools import encoders
    case = enc_cases.by_name()["one_block"]
    fn = str(tmp_path / "r.wv")
    with pytest.raises(ValueError):
        encoders.encode_wavpack(fn, reader(case), 56, wave_header=b"x")
    with pytest.raises(ValueError):
        encoders.encode_wavpack(fn, reader(case), 56, wave_footer=b"x")
    with pytest.raises(ValueError):
        encoders.encode_wavpack(fn, reader(case), 56, correlation_passes=3)
    with pytest.raises(ValueError):
        encoders.encode_wavpack(fn, reader(case), 4, correlation_passes=16)
    with pytest.raises(ValueError):
        encoders.encode_wavpack(fn, reader(case), 0)


def test_from_pcm_every_mode(tmp_path):
    import audiotools
    from audiotools import WavPackAudio, encoders
    assert WavPackAudio.DEFAULT_COMPRESSION == "standard"
    assert WavPackAudio.COMPRESSION_MODES == ("veryfast", "fast", "standard", "high", "veryhigh")
    assert [WavPackAudio.__options__[m]["correlation_passes"]
            for m in WavPackAudio.COMPRESSION_MODES] == [1, 2, 5, 10, 16]
    case = enc_cases.by_name()["std_44100"]
    x = case[5]
    sizes = {}
    for mode in WavPackAudio.COMPRESSION_MODES + (None, "nonsense"):
        fn = str(tmp_path / ("m_%s.wv" % mode))
        t = WavPackAudio.from_pcm(fn, audiotools.FrameListReader(x, 44100, 2, 16, 0x3), mode,
                                  len(x) // 2, encoding_function=encoders.encode_wavpack)
        assert isinstance(t, WavPackAudio) and t.total_frames() == len(x) // 2
        assert (t.channels(), t.bits_per_sample(), t.sample_rate()) == (2, 16, 44100)
        assert t.verify() is True
        assert np.array_equal(drain(t.to_pcm()), x)
        sizes[mode] = os.path.getsize(fn)
        if mode in ("standard", None, "nonsense"):
            assert matches(read(fn), "std_44100"), mode
        if mode == "veryhigh":
            assert matches(read(fn), "std_44100_p16")
    assert len({sizes[m] for m in WavPackAudio.COMPRESSION_MODES}) == 5


def test_from_pcm_total_mismatch_leaves_no_file(tmp_path):
    import audiotools
    from audiotools import EncodingError, WavPackAudio, encoders
    x = enc_cases.by_name()["one_block"][5]
    fn = str(tmp_path / "m.wv")
    with pytest.raises(EncodingError):
        WavPackAudio.from_pcm(fn, audiotools.FrameListReader(x, 44100, 2, 16, 0x3), "fast",
                              len(x) // 2 + 1, encoding_function=encoders.encode_wavpack)
    assert not os.path.exists(fn)

    def failing(filename, pcmreader, **kw):
        open(filename, "wb").close()
        raise ValueError("no")
    with pytest.raises(EncodingError, match="no"):
        WavPackAudio.from_pcm(fn, audiotools.FrameListReader(x, 44100, 2, 16, 0x3),
                              encoding_function=failing)
    assert not os.path.exists(fn)


def test_flac_to_wavpack_round_trip(tmp_path):
    import audiotools
    from audiotools import FlacAudio, WavPackAudio, encoders
    x = enc_cases.by_name()["long_p16_j1"][5]
    flac = FlacAudio.from_pcm(str(tmp_path / "s.flac"),
                              audiotools.FrameListReader(x, 44100, 2, 16, 0x3), "8")
    wv = WavPackAudio.from_pcm(str(tmp_path / "s.wv"), flac.to_pcm(), "high",
                               flac.total_frames(), encoding_function=encoders.encode_wavpack)
    assert wv.total_frames() == len(x) // 2
    assert np.array_equal(drain(wv.to_pcm()), x)
    assert dec.decode(read(str(tmp_path / "s.wv")))[0] == dec.OK
