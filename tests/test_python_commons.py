"""CPU: the Python-side commons: the decoder base's
decode-and-fetch lock with a stub in place of libatgpu, pack_images, and the
batch encoders' reader checks and drain with stub readers.  No GPU, no kernel."""
import threading
import time

import numpy as np
import pytest

from audiotools import _atgpu


# ------------------------------------------------------------ the pair lock
class StubLib(object):
    """stands in for libatgpu: ..._decode_host records the calling thread,
    sleeps and reports that thread's sample count; every fetch call checks
    that the handle's last decode came from its own thread, with its count"""

    def __init__(self):
        self.count = {}       # thread ident -> the sample count its decodes report
        self.last = {}        # handle -> (thread ident, count) of its last decode
        self.crossed = []     # what a fetch found instead of its own decode
        self.fetches = 0

    def __getattr__(self, name):
        if name.endswith("_create"):
            return self.create
        if name.endswith("_destroy"):
            return lambda handle: None
        if name.endswith("_last_error"):
            return lambda: b""
        if name.endswith("_decode_host"):
            return self.decode_host
        if name.endswith("_decode_fetch_blocks"):
            return self.fetch_blocks
        if "_decode_fetch" in name:
            return lambda handle, dst, cap, *more: self.fetch(name, handle, cap)
        raise AttributeError(name)

    def create(self, device, out):
        out._obj.value = 1
        return _atgpu.ATG_OK

    def decode_host(self, handle, data, nbytes, tracks, n, results, *totals):
        me = threading.get_ident()
        self.last[handle.value] = (me, self.count[me])
        time.sleep(0.003)
        for t in totals:
            t._obj.value = self.count[me]
        return _atgpu.ATG_OK

    def own(self, name, handle):
        me = threading.get_ident()
        self.fetches += 1
        if self.last[handle.value] != (me, self.count[me]):
            self.crossed.append((name, self.last[handle.value], (me, self.count[me])))
        return self.count[me]

    def fetch(self, name, handle, cap):
        count = self.own(name, handle)
        if not name.endswith("_verbatim") and cap != count:
            self.crossed.append((name, "cap", cap, count))
        return _atgpu.ATG_OK

    def fetch_blocks(self, handle, track, lengths, cap, n_blocks):
        self.own("fetch_blocks", handle)
        n_blocks._obj.value = 0
        return _atgpu.ATG_OK


def _shn(dec):
    pcm, res, verbatim, blocks = dec.decode(b"", [_atgpu.ShnDecTrack()], blocks=True)
    assert len(res) == len(blocks) == 1
    return pcm


HOST_PATHS = [
    ("flac", _atgpu.Decoder, lambda d: d.decode(b"", [])[0]),
    ("oggflac", _atgpu.Decoder, lambda d: d.decode_oggflac(b"", [])[0]),
    ("alac", _atgpu.AlacDecoder, lambda d: d.decode(b"", [])[0]),
    ("tta", _atgpu.TtaDecoder, lambda d: d.decode(b"", [])[0]),
    ("wavpack", _atgpu.WvDecoder, lambda d: d.decode(b"", [])[0]),
    ("shorten", _atgpu.ShnDecoder, _shn),
]


@pytest.mark.parametrize("cls,decode", [p[1:] for p in HOST_PATHS], ids=[p[0] for p in HOST_PATHS])
def test_decode_and_fetch_hold_one_lock(monkeypatch, cls, decode):
    """two threads on one decoder, four host decodes each: every fetch sees
    its own thread's decode"""
    lib = StubLib()
    monkeypatch.setattr(_atgpu, "load_library", lambda: lib)
    assert issubclass(cls, _atgpu._DecoderHandle)
    dec = cls(0)     # the real constructor, the stub's create: no device opened
    failures = []

    def work(count):
        lib.count[threading.get_ident()] = count
        try:
            for _ in range(4):
                pcm = decode(dec)
                assert len(pcm) == count
        except BaseException as e:  # noqa: B902 -- reported below
            failures.append(e)

    threads = [threading.Thread(target=work, args=(c,)) for c in (3000, 5000)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    dec.close()
    assert not failures, failures
    assert not lib.crossed, lib.crossed
    assert lib.fetches >= 8


# -------------------------------------------------------------- pack_images
def test_pack_images():
    images = [b"", b"\x01", b"\x02\x03\x04", b"\x05\x06\x07\x08", b"\x09\x0a\x0b\x0c\x0d",
              bytearray(b"\xff\xfe")]
    data, spans = _atgpu.pack_images(images)
    assert isinstance(data, bytes)
    assert spans == [(0, 0), (0, 1), (4, 3), (8, 4), (12, 5), (20, 2)]
    assert len(data) == sum((len(i) + 3) // 4 * 4 for i in images) == 24
    covered = bytearray(len(data))
    for img, (offset, nbytes) in zip(images, spans):
        assert offset % 4 == 0 and nbytes == len(img)
        assert data[offset:offset + nbytes] == bytes(img)
        covered[offset:offset + nbytes] = b"\x01" * nbytes
    assert all(data[k] == 0 for k in range(len(data)) if not covered[k])
    ogg_data, tracks = _atgpu.oggflac_pack(images)
    assert ogg_data == data
    assert [(t.data_offset, t.data_bytes) for t in tracks] == spans
    assert _atgpu.pack_images([]) == (b"", [])


# ------------------------------------------------- the batch encoders' drain
class StubReader(object):
    """a PCMReader that hands out `reads` frames per call, whatever is asked"""

    def __init__(self, reads, channels=2, bits_per_sample=16, sample_rate=44100,
                 channel_mask=0x3):
        from audiotools import pcm
        self.channels, self.bits_per_sample = channels, bits_per_sample
        self.sample_rate, self.channel_mask = sample_rate, channel_mask
        self.closed = False
        self._lists, value = [], 0
        for n in list(reads) + [0]:
            samples = np.arange(value, value + n * channels, dtype=np.int32) % 100
            value += n * channels
            self._lists.append(pcm.FrameList._wrap(samples, channels, bits_per_sample))

    def read(self, pcm_frames):
        return self._lists.pop(0) if len(self._lists) > 1 else self._lists[0]

    def close(self):
        self.closed = True


def test_drain_regular_and_irregular_reads():
    from audiotools import encoders
    readers = [StubReader([256, 256, 100]), StubReader([256, 100, 256]), StubReader([]),
               StubReader([256])]
    pcm, tracks = encoders._drain(readers, 256, 2, 16)
    assert [(t[0], t[1]) for t in tracks] == [(0, 612), (612, 612), (1224, 0), (1224, 256)]
    assert tracks[0][2] is None and tracks[2][2] is None and tracks[3][2] is None
    assert tracks[1][2].dtype == np.uint32 and list(tracks[1][2]) == [256, 100, 256]
    assert pcm.dtype == np.int16 and len(pcm) == 2 * 1480
    assert list(pcm[:6]) == [0, 1, 2, 3, 4, 5] and list(pcm[1224:1228]) == [0, 1, 2, 3]
    assert not any(r.closed for r in readers)


@pytest.mark.parametrize("bits,dtype", [(8, np.int16), (16, np.int16), (24, np.int32)])
def test_drain_sample_container(bits, dtype):
    from audiotools import encoders
    pcm, _ = encoders._drain([StubReader([10, 3], bits_per_sample=bits)], 10, 2, bits)
    assert pcm.dtype == dtype and len(pcm) == 26
    pcm, _ = encoders._drain([], 10, 2, bits)
    assert pcm.dtype == dtype and len(pcm) == 0


def test_drain_raises_what_it_is_given_for_irregular_reads():
    from audiotools import encoders
    second = StubReader([5])
    with pytest.raises(ValueError, match="^whole blocks$"):
        encoders._drain([StubReader([10, 3, 10]), second], 10, 2, 16,
                        irregular=ValueError("whole blocks"))
    assert len(second._lists) == 2     # raised before the next reader was read
    pcm, tracks = encoders._drain([StubReader([10, 3])], 10, 2, 16,
                                  irregular=ValueError("whole blocks"))
    assert tracks == [(0, 13, None)]


RATE3 = "all pcmreaders of a batch must share channels, bits-per-sample and sample rate"
BITS2 = "all pcmreaders of a batch must share channels and bits-per-sample"
MASK4 = ("all pcmreaders of a batch must share channels, channel mask, bits-per-sample and "
         "sample rate")


def _batch_calls():
    from audiotools import encoders
    return {
        "flac": (lambda n, r: encoders.encode_flac_batch(n, r, 4096, 8, 0, 4), RATE3,
                 ("channels", "bits_per_sample", "sample_rate")),
        "oggflac": (lambda n, r: encoders.encode_oggflac_batch(n, r, 4096, 8, 0, 4), RATE3,
                    ("channels", "bits_per_sample", "sample_rate")),
        "alac": (lambda n, r: encoders.encode_alac_batch(n, r, 4096, 10, 40, 14), BITS2,
                 ("channels", "bits_per_sample")),
        "tta": (lambda n, r: encoders.encode_tta_batch(n, r), RATE3,
                ("channels", "bits_per_sample", "sample_rate")),
        "shn": (lambda n, r: encoders.encode_shn_batch(n, r, False, True, [b""] * len(n)),
                BITS2, ("channels", "bits_per_sample")),
        "wavpack": (lambda n, r: encoders.encode_wavpack_batch(n, r, 4096), MASK4,
                    ("channels", "channel_mask", "bits_per_sample", "sample_rate")),
    }


OTHER = {"channels": 1, "bits_per_sample": 24, "sample_rate": 48000, "channel_mask": 0x4}


@pytest.mark.parametrize("codec", ["flac", "oggflac", "alac", "tta", "shn", "wavpack"])
def test_batch_format_mismatch_messages(tmp_path, codec):
    """every attribute a codec's batch must share, differing in the second
    reader: the parent's ValueError text, raised before anything is read,
    opened or sent to a GPU"""
    call, message, attrs = _batch_calls()[codec]
    for attr in attrs:
        value = OTHER[attr]
        if codec == "shn" and attr == "bits_per_sample":
            value = 8
        readers = [StubReader([10]), StubReader([10], **{attr: value})]
        names = [str(tmp_path / ("%s_%s_%d" % (codec, attr, k))) for k in range(2)]
        with pytest.raises(ValueError) as e:
            call(names, readers)
        assert str(e.value) == message
        assert all(len(r._lists) == 2 and not r.closed for r in readers)
        assert not list(tmp_path.iterdir())
    with pytest.raises(ValueError) as e:
        call([str(tmp_path / "one")], [StubReader([10]), StubReader([10])])
    assert str(e.value) == ("files and pcmreaders differ in length" if codec in ("alac", "tta")
                            else "filenames and pcmreaders differ in length")


def test_shared_format_values():
    from audiotools import encoders
    readers = [StubReader([1], 2, 16, 44100, 0x3), StubReader([1], 2, 16, 44100, 0x3)]
    assert encoders._shared_format(readers, ("channels", "channel_mask", "bits_per_sample",
                                             "sample_rate")) == (2, 3, 16, 44100)


def test_write_images(tmp_path):
    """open file objects are written to, names are opened in turn"""
    import io
    from audiotools import encoders

    class Res(object):
        def __init__(self, out_offset, nbytes):
            self.out_offset, self.bytes = out_offset, nbytes

    out = np.arange(16, dtype=np.uint8)
    results = [Res(0, 3), Res(4, 0), Res(8, 5)]
    files = [io.BytesIO() for _ in results]
    encoders._write_images(files, out, results)
    assert [f.getvalue() for f in files] == [bytes([0, 1, 2]), b"", bytes([8, 9, 10, 11, 12])]
    names = [str(tmp_path / ("f%d" % k)) for k in range(3)]
    encoders._write_images(names, out, results)
    assert [open(n, "rb").read() for n in names] == [f.getvalue() for f in files]
