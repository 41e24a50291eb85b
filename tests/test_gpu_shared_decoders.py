"""GPU: two threads on the process-wide True Audio and Shorten decoders, each
decoding its own image: the host decode and the fetch of its PCM stay paired
(the lock of _atgpu._DecoderHandle)."""
import io
import threading

import numpy as np
import pytest

import signals

pytestmark = pytest.mark.gpu
RATE = 44100


def reader(x):
    import audiotools
    return audiotools.BufferedPCMReader(audiotools.FrameListReader(x, RATE, 1, 16, 0x4))


def tta_image(x, tmp_path):
    from audiotools import encoders, tta
    frames = io.BytesIO()
    sizes = encoders.encode_tta(frames, reader(x))
    return tta.tta_header(1, 16, RATE, len(x)) + tta.tta_seektable(sizes) + frames.getvalue()


def shn_image(x, tmp_path):
    from audiotools import encoders
    name = str(tmp_path / ("%d.shn" % len(x)))
    encoders.encode_shn(name, reader(x), False, True, b"")
    with open(name, "rb") as f:
        return f.read()


@pytest.mark.parametrize("codec", ["tta", "shn"])
def test_two_threads_share_the_decoder(tmp_path, codec):
    """mono 16-bit noise, 3000 frames for one thread and 5000 for the other:
    six decodes each, all equal to the image's single-threaded decode (a
    crossed fetch would show in the length as well as the content)"""
    from audiotools import decoders
    make, decode = {"tta": (tta_image, decoders.decode_tta_batch),
                    "shn": (shn_image, decoders.decode_shn_batch)}[codec]
    sources = [signals.noise(n, 1, 16, seed) for n, seed in ((3000, 11), (5000, 12))]
    images = [make(x, tmp_path) for x in sources]
    alone = [decode([img])[0] for img in images]
    for x, one in zip(sources, alone):
        assert len(one[2]) == len(x) and np.array_equal(one[2], x)
    failures = []

    def work(k):
        try:
            for _ in range(6):
                got = decode([images[k]])[0]
                assert got[0] == alone[k][0]
                assert len(got[2]) == len(alone[k][2])
                assert np.array_equal(got[2], alone[k][2])
        except BaseException as e:  # noqa: B902 -- reported below
            failures.append((k, e))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures
