"""GPU: audiotools.encoders.encode_oggflac / encode_oggflac_batch and
OggFlacAudio.from_pcm with that encoding function, against the source PCM and
tests/oggflac_mux_port.py."""
import hashlib

import numpy as np
import pytest

import oggflac_mux_port as mp
import oggflac_port as op
import oracle_port
import signals

pytestmark = pytest.mark.gpu
RATE = 44100


def drain(pcmreader):
    got = []
    while True:
        fl = pcmreader.read(4096)
        if not len(fl):
            break
        got.append(fl.samples)
    pcmreader.close()
    return np.concatenate(got) if got else np.zeros(0, np.int32)


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("ch,bps,mask,want_mask", [(2, 16, 0x3, 0), (6, 24, 0x060F, 0x060F)],
                         ids=["stereo16", "six24"])
def test_from_pcm_with_the_encoder(tmp_path, ch, bps, mask, want_mask):
    import audiotools
    from audiotools.encoders import encode_oggflac
    x = signals.make("tone", 4096 * 2 + 77, ch, bps, seed=ch)
    fn = str(tmp_path / "a.oga")
    a = audiotools.OggFlacAudio.from_pcm(fn, audiotools.FrameListReader(x, RATE, ch, bps, mask),
                                         compression="8", encoding_function=encode_oggflac)
    assert isinstance(a, audiotools.OggFlacAudio) and a.filename == fn
    assert (a.channels(), a.bits_per_sample(), a.sample_rate()) == (ch, bps, RATE)
    assert a.total_frames() == len(x) // ch
    assert int(a.channel_mask()) == mask
    assert np.array_equal(drain(a.to_pcm()), x)
    assert a.verify() is True
    # the image is the port's, apart from the random serial number
    image = read(fn)
    serial = int.from_bytes(image[14:18], "little")
    assert a.__serial_number__ == serial
    want = mp.encode(x, ch, bps, RATE, dict(serial_number=serial, channel_mask=want_mask),
                     **oracle_port.PRESETS["8"])
    assert image == want["image"]
    packets = op.read_packets(image)[0]
    assert (b"WAVEFORMATEXTENSIBLE_CHANNEL_MASK=0x%.4X" % mask in packets[1]) == bool(want_mask)
    assert bytes(a._si.md5) == hashlib.md5(oracle_port.pcm_bytes(x, bps)).digest()


def test_batch_equals_single_calls(tmp_path):
    import audiotools
    from audiotools import encoders
    xs = [signals.make("tone", n, 2, 16, seed=n) for n in (5000, 1, 12289)]
    opts = dict(oracle_port.PRESETS["8"], padding_size=100, serial_number=0xFFFFFFFF,
                page_segments=7, page_per_packet=False)

    def readers():
        return [audiotools.FrameListReader(x, RATE, 2, 16, 0x3) for x in xs]

    names = [str(tmp_path / ("b%d.oga" % k)) for k in range(3)]
    lists = encoders.encode_oggflac_batch(names, readers(), **opts)
    for k, (x, r) in enumerate(zip(xs, readers())):
        one = str(tmp_path / ("s%d.oga" % k))
        single = encoders.encode_oggflac(one, r, **dict(opts, serial_number=0xFFFFFFFF + k))
        assert read(one) == read(names[k])
        assert single == lists[k]
        d = mp.encode(x, 2, 16, RATE, dict(serial_number=0xFFFFFFFF + k, page_segments=7,
                                           page_per_packet=False),
                      **dict(oracle_port.PRESETS["8"], padding_size=100))
        assert read(one) == d["image"]
        assert lists[k] == list(zip(d["page_offsets"], d["pcm_frames"]))
    # a call without a serial number draws one
    a, b = str(tmp_path / "r1.oga"), str(tmp_path / "r2.oga")
    encoders.encode_oggflac(a, readers()[0], **oracle_port.PRESETS["8"])
    encoders.encode_oggflac(b, readers()[0], **oracle_port.PRESETS["8"])
    assert read(a)[:14] == read(b)[:14] and read(a)[18:22] == read(b)[18:22]
    assert read(a)[14:18] != read(b)[14:18]


def test_default_from_pcm_still_raises(tmp_path):
    import audiotools
    x = signals.make("tone", 1000, 2, 16, seed=3)
    with pytest.raises(audiotools.EncodingError) as e:
        audiotools.OggFlacAudio.from_pcm(str(tmp_path / "c.oga"),
                                         audiotools.FrameListReader(x, RATE, 2, 16, 0x3))
    assert "encode_oggflac" in str(e.value)
    with pytest.raises(NotImplementedError):
        audiotools.OggFlacAudio.update_metadata(None, None)


def test_refused_readers(tmp_path):
    import audiotools
    from audiotools import encoders
    from audiotools.encoders import encode_oggflac
    a = audiotools.FrameListReader(signals.make("tone", 100, 2, 16), RATE, 2, 16, 0x3)
    b = audiotools.FrameListReader(signals.make("tone", 100, 1, 16), RATE, 1, 16, 0x4)
    with pytest.raises(ValueError):
        encoders.encode_oggflac_batch([str(tmp_path / "x.oga"), str(tmp_path / "y.oga")], [a, b],
                                      **oracle_port.PRESETS["8"])
    x = signals.make("tone", 100, 3, 16)
    from audiotools.flac import UnsupportedChannelMask
    with pytest.raises(UnsupportedChannelMask):
        audiotools.OggFlacAudio.from_pcm(str(tmp_path / "m.oga"),
                                         audiotools.FrameListReader(x, RATE, 3, 16, 0x0700),
                                         encoding_function=encode_oggflac)
