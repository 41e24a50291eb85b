"""GPU: DVD-Audio titles (csrc/aob_decode.hip) through the C ABI and the
Python layers over it, against the numpy port (aob_port.py) and the
reference's vectors (golden/dvda_vectors.json).

A batch is a list of AOB images, one title each, laid into one byte buffer;
the port's answers for a batch are computed once and shared.  The output
buffer starts 16 bytes into its allocation and has room behind the last
title, so canaries sit before, between (the padding up to every title's
16-byte boundary) and after the outputs."""
import hashlib
import json
import os

import numpy as np
import pytest

import aob_port as port
import dvda_build as build
import dvda_cases as cases
from audiotools import _atgpu

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dvda_vectors.json")
FIELDS = ["status", "stop_sector", "sample_rate", "bits_per_sample", "channels", "channel_mask",
          "channel_assignment", "good_frames"]
SECTOR_FIELDS = ["status", "payload_offset", "payload_length", "codec_id", "group_1_bps",
                 "group_1_rate", "channel_assignment"]
GUARD = 64  # canary samples before and after the outputs


@pytest.fixture(scope="module")
def golden():
    return cases.load_golden(GOLDEN)


def sized_spec(seed, bits, channels, frames, pattern, rate=0, leftover=5):
    """a spec that holds exactly `frames` frames: the pattern's payload sizes
    in turn until the bytes (whole chunks and `leftover` more) are placed"""
    chunk = bits // 8 * channels * 2
    total = frames // 2 * chunk + min(leftover, chunk - 1)
    sizes, i = [], 0
    while total > 0 or not sizes:
        n = min(pattern[i % len(pattern)], total)
        sizes.append(n)
        total -= n
        i += 1
    return cases.spec(seed, bits, channels, sizes, rate=rate)


class Batch(object):
    """images -> the byte buffer, the title table and the port's answers"""

    def __init__(self, images):
        self.images = images
        self.titles, parts, pos = [], [], 0
        for k, img in enumerate(images):
            self.titles.append((pos, len(img) // build.SECTOR))
            parts.append(img)
            pos += len(img)
            if k % 3 == 0:   # not every title starts on a sector boundary
                parts.append(b"\xee" * 16)
                pos += 16
        self.data = np.frombuffer(b"".join(parts), dtype=np.uint8)
        self.want = [port.decode(img) for img in images]

    def run(self, eng, fmt, want_sectors=False):
        """-> (results, per-title sample arrays, whole output with guards,
        expected whole output, sector table or None)"""
        dtype = np.int16 if fmt == _atgpu.PCM_S16 else np.int32
        d_bytes = eng.device_alloc(max(16, self.data.nbytes))
        eng.copy_to_device(d_bytes, self.data)
        d_pcm = None
        try:
            scan = _atgpu.aob_scan_device(d_bytes, self.data.nbytes, self.titles, fmt,
                                          want_sectors)
            total = scan[1]
            canary = (np.arange(total + 2 * GUARD, dtype=np.int64) * 2654435761 >> 9).astype(dtype)
            d_pcm = eng.device_alloc(canary.nbytes)
            eng.copy_to_device(d_pcm, canary)
            res = _atgpu.aob_decode_device(d_bytes, self.data.nbytes, self.titles,
                                           d_pcm + GUARD * canary.itemsize, fmt, total)
            got = eng.copy_to_host(np.empty_like(canary), d_pcm)
        finally:
            eng.device_free(d_bytes)
            if d_pcm:
                eng.device_free(d_pcm)
        expect = canary.copy()
        outs = []
        for r, s, (w, x, _) in zip(res, scan[0], self.want):
            assert [getattr(r, f) for f in FIELDS] == [getattr(s, f) for f in FIELDS]
            assert r.sample_offset == s.sample_offset
            assert r.sample_offset % (16 // canary.itemsize) == 0
            n = r.good_frames * r.channels
            o = GUARD + r.sample_offset
            outs.append(got[o:o + n])
            if len(x) == n:
                expect[o:o + n] = x.astype(dtype)
        return res, outs, got, expect, scan[2] if want_sectors else None

    def check(self, res, outs, got, expect):
        for k, (r, (w, x, _)) in enumerate(zip(res, self.want)):
            assert {f: getattr(r, f) for f in FIELDS} == w, k
            assert len(outs[k]) == len(x), k
        bad = np.nonzero(got != expect)[0]
        assert not len(bad), "first wrong sample at %d of %d" % (bad[0], len(got))


def check_sectors(table, batch):
    pos = 0
    for k, (_, _, recs) in enumerate(batch.want):
        for i, rec in enumerate(recs):
            t = table[pos + i]
            assert {f: getattr(t, f) for f in SECTOR_FIELDS} == rec, (k, i)
        pos += len(recs)
    assert pos == len(table)


def frame_counts():
    t = _atgpu.aob_tile_frames()
    return [0, 2, t - 2, t, t + 2, 2 * t - 2, 2 * t, 2 * t + 2]


@pytest.fixture(scope="module")
def layout_batches():
    """per integer format: every layout it holds at every frame count round
    one and two tiles, over the straddling payload patterns"""
    out = {}
    for fmt, bit_list in (("s16", (16,)), ("s32", (16, 24))):
        images, seed = [], 0
        for bits in bit_list:
            for ch in range(1, 7):
                for n in frame_counts():
                    seed += 1
                    pattern = [cases.STRADDLE2, cases.STRADDLE2B][seed % 2]
                    if n == 2:
                        pattern = cases.TINY
                    images.append(build.aob_image(
                        sized_spec(seed, bits, ch, n, pattern, leftover=seed % 7))[0])
        # one tile spread over thousands of sectors of 0, 1 and 7 bytes
        t = _atgpu.aob_tile_frames()
        images.append(build.aob_image(sized_spec(999, bit_list[-1], 6, t + 2, cases.TINY))[0])
        out[fmt] = Batch(images)
    return out


@pytest.mark.parametrize("fmt", ["s16", "s32"])
def test_layouts_and_tile_edges(gpu_engine, layout_batches, fmt):
    bt = layout_batches[fmt]
    code = _atgpu.PCM_S16 if fmt == "s16" else _atgpu.PCM_S32
    res, outs, got, expect, table = bt.run(gpu_engine, code, want_sectors=True)
    bt.check(res, outs, got, expect)
    check_sectors(table, bt)
    counts = sorted(set(r.good_frames for r in res))
    assert counts == sorted(set(frame_counts())), counts
    assert set(_atgpu.aob_kernel_times()) == {"sectors", "layout", "pcm"}


@pytest.fixture(scope="module")
def golden_batch(golden):
    names = sorted(golden["titles"])
    images = []
    for name in names:
        v = golden["titles"][name]
        img, _ = cases.case_image(v["spec"], v["first"])
        images.append(img[v["first"] * build.SECTOR:])
    return names, Batch(images)


def answer(r, samples, pts):
    """a GPU result in the reference's terms: [stderr, md5[:16], bytes]"""
    raw, err, _ = port.answer_from({f: getattr(r, f) for f in FIELDS}, samples, pts)
    return [err, hashlib.md5(raw).hexdigest()[:16], len(raw)]


def test_golden_titles(gpu_engine, golden, golden_batch):
    names, bt = golden_batch
    res, outs, got, expect, table = bt.run(gpu_engine, _atgpu.PCM_S32, want_sectors=True)
    bt.check(res, outs, got, expect)
    check_sectors(table, bt)
    for name, r, x in zip(names, res, outs):
        v = golden["titles"][name]
        assert v["returncode"] == 0
        assert answer(r, x, v["pts"]) == [v["stderr"], v["md5"][:16], v["bytes"]], name


def ragged_images():
    rng = np.random.default_rng(300)
    images = []
    for k in range(300):
        bits = (16, 24)[int(rng.integers(2))]
        ch = int(rng.integers(1, 7))
        sizes = [int(rng.choice([0, 1, 7, 35, 500, 1001, 1990, 2000]))
                 for _ in range(int(rng.integers(1, 7)))]
        img = build.aob_image(cases.spec(1000 + k, bits, ch, sizes,
                                         rate=int(rng.choice([0, 1, 2, 8, 9, 10]))))[0]
        if k % 9 == 4:    # a damaged pack header somewhere in the title
            s = int(rng.integers(len(sizes)))
            img = build.flip(img, 8 * (s * build.SECTOR + 3) + 7)
        images.append(img)
    return images


def test_ragged_batch_of_300(gpu_engine):
    bt = Batch(ragged_images())
    first = bt.run(gpu_engine, _atgpu.PCM_S32)
    bt.check(*first[:4])
    assert len(set(r.status for r in first[0])) >= 2
    assert len(set((r.bits_per_sample, r.channels) for r in first[0])) >= 12
    again = bt.run(gpu_engine, _atgpu.PCM_S32)
    assert np.array_equal(first[2], again[2])
    assert [[getattr(r, f) for f in FIELDS] for r in first[0]] == \
        [[getattr(r, f) for f in FIELDS] for r in again[0]]


@pytest.mark.parametrize("name", sorted(cases.flip_specs()))
def test_flip_sweep(gpu_engine, golden, name):
    """every single-bit flip of the header bytes in one batch, a clean copy
    after every eighth"""
    sweep = golden["sweeps"][name]
    assert sweep["spec"] == json.loads(json.dumps(cases.flip_specs()[name]))
    clean, x = build.aob_image(sweep["spec"])
    assert sweep["bits"] == build.header_bits(sweep["spec"]) and len(sweep["bits"]) == 1808
    images, which = [], []
    for k, bit in enumerate(sweep["bits"]):
        images.append(build.flip(clean, bit))
        which.append(k)
        if k % 8 == 7:
            images.append(clean)
            which.append(None)
    bt = Batch(images)
    res, outs, got, expect, table = bt.run(gpu_engine, _atgpu.PCM_S32, want_sectors=True)
    bt.check(res, outs, got, expect)
    check_sectors(table, bt)
    compared = 0
    for r, out, k in zip(res, outs, which):
        if k is None:
            assert r.status == port.OK and np.array_equal(out, x)
            continue
        bit = str(sweep["bits"][k])
        if bit in sweep["set_aside"]:
            continue
        for j, (pts, (rc, err, md5, n)) in enumerate(zip(sweep["pts"], sweep["flips"][k])):
            if j == 1 and bit in sweep["replay"]:
                continue
            assert rc == 0 and answer(r, out, pts) == [err, md5, n], (bit, pts)
            compared += 1
    assert compared >= 2 * 1808 * 0.98 - len(sweep["replay"])


def test_mlp_and_unknown_first_packets(gpu_engine):
    specs = cases.first_packet_cases()
    bt = Batch([build.aob_image(s)[0] for _, s in specs])
    res, outs, got, expect, table = bt.run(gpu_engine, _atgpu.PCM_S32, want_sectors=True)
    bt.check(res, outs, got, expect)
    check_sectors(table, bt)
    assert [r.status for r in res] == [port.MLP, port.UNKNOWN_CODEC, port.MLP]
    assert all(t.status == 0 and t.payload_length for t in table)


def test_capacity_and_format_errors(gpu_engine):
    eng = gpu_engine
    img16 = build.aob_image(cases.spec(1, 16, 2, [2000, 2000]))[0]
    img24 = build.aob_image(cases.spec(2, 24, 2, [2000, 2000]))[0]
    data = np.frombuffer(img16 + img24, dtype=np.uint8)
    titles = [(0, 2), (len(img16), 2)]
    d_bytes = eng.device_alloc(data.nbytes)
    d_pcm = eng.device_alloc(1 << 16)
    try:
        eng.copy_to_device(d_bytes, data)
        res, total = _atgpu.aob_scan_device(d_bytes, data.nbytes, titles, _atgpu.PCM_S32)
        with pytest.raises(_atgpu.ATGError) as e:
            _atgpu.aob_decode_device(d_bytes, data.nbytes, titles, d_pcm, _atgpu.PCM_S32,
                                     total - 1)
        assert e.value.status == _atgpu.ATG_ERR_CAPACITY
        with pytest.raises(_atgpu.ATGError) as e:
            _atgpu.aob_decode_device(d_bytes, data.nbytes, titles, d_pcm, _atgpu.PCM_S16,
                                     1 << 14)
        assert e.value.status == _atgpu.ATG_ERR_INVALID and "24-bit" in str(e.value)
    finally:
        eng.device_free(d_bytes)
        eng.device_free(d_pcm)
    res, pcm = _atgpu.aob_decode_host(data, titles)
    for r, img in zip(res, (img16, img24)):
        w, x, _ = port.decode(img)
        assert r.good_frames == w["good_frames"]
        assert np.array_equal(pcm[r.sample_offset:r.sample_offset + len(x)], x)


# ------------------------------------------------------------ Python layers
def _frames(x, channels, a, n):
    return x[a * channels:(a + n) * channels]


@pytest.fixture(scope="module")
def disc(tmp_path_factory):
    """two titles over two AOB files; the second title's last track asks for
    more frames than its sectors hold"""
    from audiotools import dvda
    path = str(tmp_path_factory.mktemp("AUDIO_TS"))
    s1 = cases.spec(31, 16, 2, cases.STRADDLE2 * 3, rate=0, **cases.PADS)
    s2 = cases.spec(32, 24, 6, cases.STRADDLE2B * 4, rate=1)
    n2 = cases.frames_of(s2)
    info = build.write_disc(path, [(s1, [1600, 800, 1200]), (s2, [320, 160, (n2 - 480) // 16 * 16 + 64])],
                            split_at=7)
    return dvda.DVDAudio(path), info


def test_dvda_title_tracks_and_reads(gpu_engine, disc):
    from audiotools import decoders
    d, info = disc
    title = d[0][0]
    x, ch = info[0]["samples"], 2
    for size in (4096, 4095, 333):
        r = title.to_pcm()
        assert (r.sample_rate, r.channels, r.pcm_frames) == (0, 0, 0)
        got = []
        for track in title:
            r.next_track(track.pts_length)
            assert (r.sample_rate, r.bits_per_sample, r.channels, r.channel_mask) == \
                (48000, 16, 2, 3)
            with pytest.raises(ValueError, match="current track has not been exhausted"):
                r.next_track(1)
            parts = []
            while r.pcm_frames:
                f = r.read(size)
                assert 0 < f.frames <= size
                parts.append(np.asarray(f.samples))
            assert r.read(size).frames == 0
            got.append(np.concatenate(parts))
        r.close()
        for (a, n, _), g in zip(info[0]["tracks"], got):
            assert np.array_equal(g, _frames(x, ch, a, n))
    with pytest.raises(IOError):
        decoders.DVDA_Title(d.audio_ts_path, 2, 0, 1)
    with pytest.raises(ValueError):
        decoders.DVDA_Title(d.audio_ts_path, 1, 0, 1, cdrom="/dev/null")


def test_dvda_title_error_order(gpu_engine, tmp_path):
    """a bad sector: the whole frames before it are delivered, then IOError"""
    from audiotools import decoders
    s = cases.spec(33, 24, 2, [2000, 1999, 1001, 7, 1500])
    img, x = build.aob_image(s)
    img = build.flip(img, 8 * (3 * build.SECTOR + 2) + 7)     # sector 3's sync
    (tmp_path / "ATS_01_1.AOB").write_bytes(img)
    good = (2000 + 1999 + 1001) // 12 * 2
    r = decoders.DVDA_Title(str(tmp_path), 1, 0, 4)
    r.next_track(cases.pts_for(good + 100, 48000))
    parts = []
    with pytest.raises(IOError, match="I/O reading PCM packet"):
        while True:
            parts.append(np.asarray(r.read(4096).samples))
    assert np.array_equal(np.concatenate(parts), x[:good * 2])
    # a first sector that does not parse, and an MLP-typed title
    (tmp_path / "ATS_01_1.AOB").write_bytes(build.flip(img, 31))
    with pytest.raises(IOError, match="initialization packet"):
        decoders.DVDA_Title(str(tmp_path), 1, 0, 4).next_track(100)
    mlp = build.aob_image(cases.first_packet_cases()[0][1])[0]
    (tmp_path / "ATS_01_1.AOB").write_bytes(mlp)
    with pytest.raises(ValueError, match="MLP"):
        decoders.DVDA_Title(str(tmp_path), 1, 0, 2).next_track(100)


def test_decode_dvda_batch_over_two_aobs(gpu_engine, disc):
    from audiotools import decoders
    d, info = disc
    t1, t2 = d[0]
    out = decoders.decode_dvda_batch(
        [t1, t2, (d.audio_ts_path, 1, t2[0].first_sector, t2[-1].last_sector)])
    whole = open(d.files["ATS_01_1.AOB"], "rb").read() + open(d.files["ATS_01_2.AOB"], "rb").read()
    for (r, x), first in zip(out, (0, info[1]["first_sector"], info[1]["first_sector"])):
        w, want, _ = port.decode(whole, first)
        assert {f: getattr(r, f) for f in FIELDS} == w
        assert np.array_equal(x, want)
    # title 1 runs on into title 2's sectors; its own frames come first
    n1 = len(info[0]["samples"])
    assert np.array_equal(out[0][1][:n1], info[0]["samples"])
    assert np.array_equal(out[1][1], info[1]["samples"])
    batch = decoders.decode_dvda_batch([t2], on_device=True)
    try:
        r = batch.results[0]
        got = gpu_engine.copy_to_host(np.empty(batch.total_samples, np.int32), batch.d_pcm)
        assert np.array_equal(got[r.sample_offset:r.sample_offset + len(out[1][1])], out[1][1])
    finally:
        batch.close()


class _WindowReader(object):
    """a PCMReader over frames [a, a + n) of a title's samples"""

    def __init__(self, x, a, n, rate, channels, mask, bits):
        self.x, self.pos, self.end = x, a, a + n
        self.sample_rate, self.channels, self.channel_mask, self.bits_per_sample = \
            rate, channels, mask, bits

    def read(self, frames):
        from audiotools import pcm
        n = min(frames, self.end - self.pos)
        out = pcm.FrameList._wrap(self.x[self.pos * self.channels:(self.pos + n) * self.channels],
                                  self.channels, self.bits_per_sample)
        self.pos += n
        return out

    def close(self):
        pass


def test_tracks_to_flac_batch(gpu_engine, disc, tmp_path):
    from audiotools import DecodingError, dvda
    from audiotools.flac import FlacAudio
    d, info = disc
    tracks = [t for title in d[0] for t in title]
    targets = [str(tmp_path / ("t%d.flac" % k)) for k in range(len(tracks))]
    out = dvda.tracks_to_flac_batch(tracks, targets, compression="8")
    assert isinstance(out[-1], DecodingError) and not os.path.exists(targets[-1])
    k = 0
    for title, ti in zip(d[0], info):
        for track, (a, n, _) in zip(title, ti["tracks"]):
            if k < len(tracks) - 1:
                assert isinstance(out[k], FlacAudio), out[k]
                ref = str(tmp_path / ("ref%d.flac" % k))
                FlacAudio.from_pcm(ref, _WindowReader(ti["samples"], a, n, title.sample_rate,
                                                      title.channels, title.channel_mask,
                                                      title.bits_per_sample),
                                   "8", total_pcm_frames=n)
                assert open(targets[k], "rb").read() == open(ref, "rb").read(), k
            k += 1
