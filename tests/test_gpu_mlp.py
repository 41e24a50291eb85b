"""GPU: MLP titles of DVD-Audio discs (csrc/mlp_decode.hip) through the C ABI
and the Python layers over it, against the Python port (mlp_port.py) and the
reference's vectors (golden/mlp_vectors.json).

A batch is a list of AOB images, one title each, laid into one byte buffer.
The output buffer starts GUARD samples into its allocation and has room
behind the last title, so canaries sit before, between (the padding up to
every title's 16-byte boundary) and after the outputs.

The ABI's sample is the reference's value sign-wrapped to the title's bits;
the reference's stand-alone decoder clips instead, so a vector whose port
answer leaves the range ("clip" in the golden file) is held to the port
alone."""
import hashlib
import json
import os

import numpy as np
import pytest

import aob_port
import dvda_build
import dvda_cases
import mlp_cases as cases
import mlp_port as port
from audiotools import _atgpu

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_vectors.json")
FIELDS = ["status", "stop_sector", "stop_unit", "access_units", "sample_rate", "bits_per_sample",
          "channels", "channel_mask", "channel_assignment", "substreams", "good_frames"]
UNIT_FIELDS = ["offset", "size", "end_sector", "flags", "status", "data_start"]
GUARD = 64


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def run_batch(eng, images, firsts, fmt=_atgpu.PCM_S32, want_units=False):
    """-> (results, per-title sample arrays, whole output with guards, the
    canary it was filled with, unit table or None)"""
    titles, parts, pos = [], [], 0
    for k, (img, first) in enumerate(zip(images, firsts)):
        titles.append((pos + first * 2048, len(img) // 2048 - first))
        parts.append(img)
        pos += len(img)
        if k % 3 == 0:   # not every title starts on a sector boundary
            parts.append(b"\xee" * 16)
            pos += 16
    data = np.frombuffer(b"".join(parts), dtype=np.uint8)
    dtype = np.int16 if fmt == _atgpu.PCM_S16 else np.int32
    d_bytes = eng.device_alloc(max(16, data.nbytes))
    eng.copy_to_device(d_bytes, data)
    d_pcm = None
    try:
        scan = _atgpu.mlp_scan_device(d_bytes, data.nbytes, titles, fmt, want_units)
        total = scan[1]
        canary = (np.arange(total + 2 * GUARD, dtype=np.int64) * 2654435761 >> 9).astype(dtype)
        d_pcm = eng.device_alloc(canary.nbytes)
        eng.copy_to_device(d_pcm, canary)
        res = _atgpu.mlp_decode_device(d_bytes, data.nbytes, titles,
                                       d_pcm + GUARD * canary.itemsize, fmt, total)
        got = eng.copy_to_host(np.empty_like(canary), d_pcm)
    finally:
        eng.device_free(d_bytes)
        if d_pcm:
            eng.device_free(d_pcm)
    outs = []
    for r, s in zip(res, scan[0]):
        assert [getattr(r, f) for f in FIELDS] == [getattr(s, f) for f in FIELDS]
        assert r.sample_offset == s.sample_offset
        assert r.sample_offset % (16 // canary.itemsize) == 0
        o = GUARD + r.sample_offset
        outs.append(got[o:o + r.good_frames * r.channels])
    return res, outs, got, canary, scan[2] if want_units else None


def check_canaries(res, got, canary):
    """nothing but the titles' own sample ranges was written"""
    keep = np.ones(len(got), dtype=bool)
    for r in res:
        o = GUARD + r.sample_offset
        keep[o:o + r.good_frames * r.channels] = False
    bad = np.nonzero(keep & (got != canary))[0]
    assert not len(bad), "sample %d outside every title was written" % bad[0]


def check_golden(r, x, rec, name):
    """one title against its golden record: the port's answer, and the
    reference's where it has one"""
    p = rec["port"]         # cases.PORT_KEYS' values, clip, the samples' MD5
    assert [getattr(r, k) for k in cases.PORT_KEYS] == p[:-2], name
    assert hashlib.md5(x.astype("<i4").tobytes()).hexdigest()[:16] == p[-1], name
    assert rec["spec"] == cases.spec_digest(next(s for s in cases.title_cases()
                                                 if s["name"] == name))
    if "set_aside" in rec or p[-2]:
        return 0
    rc, _, md5, size = rec["ref"]
    assert rc == 0, name
    raw = aob_port.pcm_bytes(x, r.bits_per_sample)[:size] if r.bits_per_sample else b""
    assert len(raw) == size and hashlib.md5(raw).hexdigest()[:16] == md5, name
    return 1


@pytest.fixture(scope="module")
def title_batch():
    specs = cases.title_cases() + cases.other_cases()
    images = [cases.image_of(s) for s in specs]
    want = [port.decode(img, first) for img, first in images]
    return specs, images, want


def test_vectors_int32(gpu_engine, golden, title_batch):
    specs, images, want = title_batch
    res, outs, got, canary, _ = run_batch(gpu_engine, [i for i, _ in images],
                                          [f for _, f in images])
    compared = 0
    for s, r, x, (w, y, _) in zip(specs, res, outs, want):
        assert {f: getattr(r, f) for f in FIELDS} == {f: w[f] for f in FIELDS}, s["name"]
        assert np.array_equal(x, y), s["name"]
        if s["name"] in golden["titles"]:
            compared += check_golden(r, x, golden["titles"][s["name"]], s["name"])
    check_canaries(res, got, canary)
    assert compared >= len(golden["titles"]) - 6
    assert set(r.status for r in res) == set(range(17)) - {port.EOF}


def test_vectors_int16_and_empty(gpu_engine, title_batch):
    specs, images, want = title_batch
    pick = [k for k, s in enumerate(specs) if s["bits"] == 16]
    imgs = [images[k][0] for k in pick] + [b""]
    res, outs, got, canary, _ = run_batch(gpu_engine, imgs, [images[k][1] for k in pick] + [0],
                                          _atgpu.PCM_S16)
    for k, r, x in zip(pick, res, outs):
        w, y, _ = want[k]
        assert {f: getattr(r, f) for f in FIELDS} == {f: w[f] for f in FIELDS}, specs[k]["name"]
        assert x.dtype == np.int16 and np.array_equal(x, y.astype(np.int16)), specs[k]["name"]
    assert res[-1].status == port.EOF and res[-1].good_frames == 0
    check_canaries(res, got, canary)
    # a 24-bit title does not fit int16
    s24 = next(k for k, s in enumerate(specs) if s["bits"] == 24)
    with pytest.raises(_atgpu.ATGError) as e:
        run_batch(gpu_engine, [images[s24][0]], [images[s24][1]], _atgpu.PCM_S16)
    assert e.value.status == _atgpu.ATG_ERR_INVALID


@pytest.mark.parametrize("name", sorted(cases.flip_specs()))
def test_damage_sweep(gpu_engine, golden, name):
    """every flip of the sweep in one batch, a clean copy after every 32"""
    sweep = golden["sweeps"][name]
    spec = cases.flip_specs()[name]
    assert sweep["spec"] == cases.spec_digest(spec)
    img, _ = cases.image_of(spec)
    bits = cases.flip_bits(spec)
    assert len(bits) == sweep["n_bits"]
    rows = cases.unpack_flips(sweep)
    assert len(rows) == len(bits)
    images, which = [], []
    for k, bit in enumerate(bits):
        images.append(dvda_build.flip(img, bit))
        which.append(k)
        if k % 32 == 31:
            images.append(img)
            which.append(None)
    res, outs, got, canary, _ = run_batch(gpu_engine, images, [0] * len(images))
    clean, clean_x, _ = port.decode(img)
    assert clean["status"] == port.OK and clean["good_frames"]
    compared = 0
    for r, x, k in zip(res, outs, which):
        if k is None:
            assert {f: getattr(r, f) for f in FIELDS} == {f: clean[f] for f in FIELDS}
            assert np.array_equal(x, clean_x)
            continue
        # the golden answer's digest covers the result, the samples and, for
        # flag "p", the reference's stderr and PCM bytes (cases.outcome)
        flag = rows[k][0]
        d = {f: getattr(r, f) for f in FIELDS}
        answer = port.answer_from(d, x, cases.ask_pts(d)) if flag == "p" else None
        assert cases.outcome(d, x, flag, answer) == rows[k], (name, bits[k])
        compared += flag == "p"
    check_canaries(res, got, canary)
    assert compared >= 0.95 * len(bits)


def test_ragged_batch_twice(gpu_engine, title_batch):
    """about 100 mixed titles, failing ones among them, in a shuffled order;
    a second run gives the same bytes"""
    specs, images, want = title_batch
    order = np.random.default_rng(5).permutation(2 * len(specs))[:100] % len(specs)
    imgs = [images[k][0] for k in order]
    firsts = [images[k][1] for k in order]
    res, outs, got, canary, _ = run_batch(gpu_engine, imgs, firsts)
    for k, r, x in zip(order, res, outs):
        w, y, _ = want[k]
        assert {f: getattr(r, f) for f in FIELDS} == {f: w[f] for f in FIELDS}, specs[k]["name"]
        assert np.array_equal(x, y), specs[k]["name"]
    check_canaries(res, got, canary)
    res2, _, got2, _, _ = run_batch(gpu_engine, imgs, firsts)
    assert np.array_equal(got, got2)
    assert [r.sample_offset for r in res] == [r.sample_offset for r in res2]


def test_unit_table(gpu_engine, title_batch):
    specs, images, want = title_batch
    res, _, _, _, table = run_batch(gpu_engine, [i for i, _ in images], [f for _, f in images],
                                    want_units=True)
    pos = 0
    for s, r, (w, _, units) in zip(specs, res, want):
        assert r.access_units == len(units), s["name"]
        for i, u in enumerate(units):
            t = table[pos + i]
            assert {f: getattr(t, f) for f in UNIT_FIELDS} == {f: u[f] for f in UNIT_FIELDS}, \
                (s["name"], i)
            assert list(t.substream_end) == u["substream_end"], (s["name"], i)
            assert list(t.substream_flags) == u["substream_flags"], (s["name"], i)
        pos += len(units)
    assert pos == len(table) and pos > 300
    times = _atgpu.mlp_kernel_times()
    assert list(times) == ["sectors", "layout", "gather", "walk", "check", "parse", "resolve",
                           "store", "filter", "output"]
    assert all(ms >= 0 for ms in times.values()) and times["filter"] > 0


def test_host_entry_and_capacity(gpu_engine, title_batch):
    specs, images, want = title_batch
    k = next(i for i, s in enumerate(specs) if s["name"] == "straddle2")
    img = images[k][0]
    w, y, _ = want[k]
    res, out = _atgpu.mlp_decode_host(img, [(0, len(img) // 2048)], len(y) + 8)
    assert res[0].status == port.OK and np.array_equal(out[:len(y)], y)
    assert not out[len(y):].any()
    with pytest.raises(_atgpu.ATGError) as e:
        _atgpu.mlp_decode_host(img, [(0, len(img) // 2048)], len(y) - 1)
    assert e.value.status == _atgpu.ATG_ERR_CAPACITY


PCM_SPEC = dvda_cases.spec(3, 16, 2, [2000, 2000], rate=0)


def disc(path, names, tracks):
    """an AUDIO_TS directory of one titleset whose titles are the named cases'
    images ("pcm": a packed-PCM title); tracks: frames per track of each title
    -> (whole image, first sector of each title)"""
    by_name = dict((s["name"], s) for s in cases.title_cases())
    image, ifo, firsts = b"", [], []
    for name, frames in zip(names, tracks):
        img = dvda_build.aob_image(PCM_SPEC)[0] if name == "pcm" else \
            cases.image_of(by_name[name])[0]
        first = len(image) // 2048
        rows, pts = [], 0
        for n in frames:
            ticks = n * 90000 // 48000
            assert ticks * 48000 == n * 90000
            rows.append((pts, ticks, first, first + len(img) // 2048 - 1))
            pts += ticks
        ifo.append({"pts_length": pts, "tracks": rows})
        firsts.append(first)
        image += img
    os.makedirs(path, exist_ok=True)
    for name, data in (("ATS_01_1.AOB", image), ("AUDIO_TS.IFO", dvda_build._ifo_audio_ts(1)),
                       ("ATS_01_0.IFO", dvda_build._ifo_ats(ifo))):
        with open(os.path.join(path, name), "wb") as f:
            f.write(data)
    return image, firsts


def test_dvda_title_and_mixed_batch(gpu_engine, tmp_path):
    """a PCM title and two MLP titles in one decode_dvda_batch; DVDA_Title's
    windows and its errors.  A title runs on to the titleset's last sector,
    as in the reference, so the port decodes the same range."""
    from audiotools import decoders
    path = str(tmp_path / "AUDIO_TS")
    image, firsts = disc(path, ["pcm", "plain-2-1-16", "bad-crc"], [[96], [48, 48], [32]])
    n = len(image) // 2048
    got = decoders.decode_dvda_batch([(path, 1, f, n - 1) for f in firsts])
    w, x, _ = aob_port.decode(image, firsts[0])
    assert got[0][0].status == w["status"] and got[0][0].mlp_status is None
    assert got[0][0].good_frames == w["good_frames"] and np.array_equal(got[0][1], x)
    for k in (1, 2):
        w, x, _ = port.decode(image, firsts[k])
        r = got[k][0]
        assert r.status == _atgpu.DVDA_MLP and r.mlp_status == w["status"]
        assert {f: getattr(r, f) for f in FIELDS if f != "status"} == \
            {f: w[f] for f in FIELDS if f != "status"}
        assert np.array_equal(got[k][1], x) and len(x)
    # title 1 decodes on through title 2's units up to its CRC error
    assert got[1][0].good_frames == 96 + 64 and got[2][0].good_frames == 64
    assert got[2][0].mlp_status == _atgpu.MLP_CRC8_MISMATCH and got[2][0].stop_unit == 4

    x = got[1][1]
    t = decoders.DVDA_Title(path, 1, firsts[1], n - 1)
    assert (t.sample_rate, t.channels, t.pcm_frames) == (0, 0, 0)
    t.next_track(90)
    assert (t.sample_rate, t.bits_per_sample, t.channels, t.channel_mask) == (48000, 16, 2, 3)
    with pytest.raises(ValueError, match="current track has not been exhausted"):
        t.next_track(1)
    a = np.concatenate([np.asarray(t.read(40).samples), np.asarray(t.read(4096).samples)])
    assert np.array_equal(a, x[:96]) and t.pcm_frames == 0 and t.read(10).frames == 0
    t.next_track(90)
    assert np.array_equal(np.asarray(t.read(4096).samples), x[96:192])
    # the reference's message and type at the read that needs the failing
    # unit, after the frames before it
    t.next_track(9000)
    assert np.array_equal(np.asarray(t.read(4096).samples), x[192:])
    with pytest.raises(ValueError, match="CRC8 mismatch decoding MLP substream"):
        t.read(1)
    # a bad sector under an MLP title
    path = str(tmp_path / "B")
    image, _ = disc(path, ["bad-sector"], [[8]])
    t = decoders.DVDA_Title(path, 1, 0, len(image) // 2048 - 1)
    t.next_track(9000)
    parts = []
    with pytest.raises(IOError, match="I/O reading MLP packet"):
        while True:
            parts.append(np.asarray(t.read(4096).samples))
    w, x, _ = port.decode(image)
    assert w["status"] == port.BAD_SECTOR and len(x)
    assert np.array_equal(np.concatenate(parts), x)
    # no major sync
    path = str(tmp_path / "C")
    image, _ = disc(path, ["plain-2-1-16"], [[8]])
    bad = bytearray(image)
    bad[image.index(b"\xf8\x72\x6f\xbb")] = 0
    with open(os.path.join(path, "ATS_01_1.AOB"), "wb") as f:
        f.write(bytes(bad))
    with pytest.raises(ValueError, match="MLP stream does not start with a major sync"):
        decoders.DVDA_Title(path, 1, 0, len(image) // 2048 - 1).next_track(100)


def test_tracks_to_flac_batch(gpu_engine, tmp_path):
    """FLAC files from device PCM of MLP titles, byte-identical to
    FlacAudio.from_pcm over a reader of the same frames"""
    from audiotools import DecodingError, dvda
    from audiotools.flac import FlacAudio
    from test_gpu_dvda import _WindowReader
    path = str(tmp_path / "AUDIO_TS")
    image, firsts = disc(path, ["pcm", "filters-16", "bad-crc"], [[96], [64, 64], [32, 64]])
    d = dvda.DVDAudio(path)
    tracks = [t for title in d[0] for t in title]
    assert len(tracks) == 5
    targets = [str(tmp_path / ("t%d.flac" % k)) for k in range(5)]
    out = dvda.tracks_to_flac_batch(tracks, targets, compression="8")
    assert isinstance(out[4], DecodingError) and not os.path.exists(targets[4])
    for k, (title, a, n) in enumerate([(0, 0, 96), (1, 0, 64), (1, 64, 64), (2, 0, 32)]):
        assert isinstance(out[k], FlacAudio), out[k]
        if title:
            w, x, _ = port.decode(image, firsts[title])
        else:
            w, x, _ = aob_port.decode(image, firsts[title])
        ref = str(tmp_path / ("ref%d.flac" % k))
        FlacAudio.from_pcm(ref, _WindowReader(x, a, n, w["sample_rate"], w["channels"],
                                              w["channel_mask"], w["bits_per_sample"]),
                           "8", total_pcm_frames=n)
        assert open(targets[k], "rb").read() == open(ref, "rb").read(), k
