"""GPU: the Ogg FLAC batch decoder (ogg_demux.hip + flac_decode.hip) against
the REFERENCE's oggflacdec as recorded in tests/golden/oggflac_vectors.json,
against tests/oggflac_port.py for the fields the reference does not print
(page and packet counts, the failing page) and for the cases on which the
reference aborts, and against the native FLAC decode of the same frames.
Every group of cases goes through the decoder as one batch."""
import functools
import hashlib

import numpy as np
import pytest

import oggflac_cases as cases
import oggflac_port as op
import oracle_port

pytestmark = pytest.mark.gpu
GOLD = cases.load_golden()


def decode(images):
    from audiotools import decoders
    out = decoders.decode_oggflac_batch(images)
    assert len(out) == len(images)
    return out


def gpu_class(r):
    if r.status not in (0, op.FD_MD5):
        return "flac:%d" % r.status
    if r.ogg_status:
        return "header" if r.ogg_status >= op.OGG_PACKET_BYTE else "ogg:%d" % r.ogg_status
    return "flac:16" if r.status == op.FD_MD5 else ""


def gpu_row(r, samples):
    """the decoder's answer in the golden file's terms; the PCM bytes are
    hashed here, from the fetched samples"""
    raw = oracle_port.pcm_bytes(samples, r.bits_per_sample) if len(samples) else b""
    c = gpu_class(r)
    return [0 if c == "" else 1, c, len(raw), hashlib.md5(raw).hexdigest()]


def check_against_port(image, r, samples, where):
    d = op.decode(image)
    assert (r.status, r.ogg_status) == (d["status"], d["ogg_status"]), where
    assert np.array_equal(samples, d["samples"]), where
    assert bytes(r.md5) == d["md5"], where
    assert (r.n_frames, r.pages, r.packets, r.header_packets) == \
        (d["n_frames"], d["pages"], d["packets"], d["header_packets"]), where
    assert (r.fail_page, r.fail_offset) == (d["fail_page"], d["fail_offset"]), where


@functools.lru_cache(maxsize=None)
def single():
    built = cases.single_cases()
    names = sorted(built)
    return built, dict(zip(names, decode([built[n] for n in names])))


def test_layout_matrix():
    """5-packet, 36-packet and 700-frame sources in 1/2/8 channels x 8/16/24
    bit, pages of 1, 7 and 255 segments and a seeded random 1..40: status,
    PCM and MD5 equal the record, the port and the native decode"""
    from audiotools import decoders
    built, got = single()
    # (one native batch per source: their channel counts differ)
    native = {s: decoders.decode_flac_batch([cases.source(s)])[0] for s in cases.source_names()}
    n = 0
    for name in sorted(built):
        if not name.startswith("matrix:"):
            continue
        rec = GOLD["single"][name]
        r, samples, sizes = got[name]
        assert gpu_row(r, samples) == [rec["returncode"], rec["class"], rec["bytes"], rec["md5"]], name
        assert rec["returncode"] == 0
        check_against_port(built[name], r, samples, name)
        st, si, pcm = native[name.split(":")[1]]
        assert st == 0 and np.array_equal(samples, pcm), name
        assert bytes(r.streaminfo_md5) == bytes(si.md5), name
        assert int(sizes.sum()) == r.pcm_frames
        n += 1
    assert n == 11 * 4


def test_lacing_edges_ignored_fields_stream_ends_and_headers():
    """packets of 765, 65,025 and 70,004 bytes, a 98 KB frame over two pages,
    a zero-segment page, junk tails, an empty packet, two frames in a packet,
    cut packets; scrambled serial and sequence numbers; streams without an
    end-of-stream page, with garbage after it, with total_samples 0, a zero
    and a wrong MD5; every first-packet error"""
    built, got = single()
    seen = set()
    for name in sorted(built):
        if name.startswith("matrix:"):
            continue
        rec = GOLD["single"][name]
        r, samples, _ = got[name]
        check_against_port(built[name], r, samples, name)
        if "set_aside" in rec:  # the reference aborts: the port's FD_EOF holds
            assert r.status == op.FD_EOF and name in ("lacing:cut1", "lacing:cut2")
        else:
            assert gpu_row(r, samples) == [rec["returncode"], rec["class"], rec["bytes"],
                                           rec["md5"]], name
        seen.add(gpu_class(r))
    one = lambda n: gpu_class(got[n][0])  # noqa: E731
    assert one("lacing:junk_tail") == "" and one("ignored:scrambled") == ""
    assert one("lacing:packet765") == one("lacing:packet65025") == one("lacing:packet70004") == ""
    assert one("lacing:bigframe") == "" and got["lacing:bigframe"][0].n_frames == 1
    assert one("lacing:empty_packet") == "flac:15" and got["lacing:empty_packet"][0].n_frames == 2
    assert one("lacing:two_frames") == "flac:16"
    assert one("lacing:cut100") == "flac:15"
    assert one("end:no_eos") == "ogg:4" and got["end:no_eos"][0].n_frames == 6
    assert one("end:garbage") == one("end:total0") == one("end:md5_zero") == ""
    assert one("end:unfinished_packet") == ""
    assert one("end:md5_wrong") == "flac:16"
    assert {"", "header", "ogg:1", "ogg:2", "ogg:3", "ogg:4", "ogg:5"} <= seen


@pytest.mark.parametrize("sweep", ["raw_flips", "raw_truncations"])
def test_raw_damage(sweep):
    """all 1,760 single-bit flips and all 220 truncations of a 220-byte
    image, each sweep as one batch: status and PCM equal the record for every
    case, nothing set aside"""
    images = cases.SWEEPS[sweep]()
    rec = GOLD["sweeps"][sweep]
    assert not rec["set_aside"] and len(images) == len(rec["rows"])
    for k, (img, (r, samples, _)) in enumerate(zip(images, decode(images))):
        row = gpu_row(r, samples)
        row[3] = row[3][:16]
        assert row == rec["rows"][k], (sweep, k)
        if k % 8 == 0:
            check_against_port(img, r, samples, (sweep, k))


def test_damage_under_valid_pages():
    """every single-bit flip of every packet, re-checksummed: 1,288 cases in
    one batch; the 37 on which the reference aborts (2.9 %, cap 5 %) are held
    to the port"""
    images = cases.packet_flips()
    rec = GOLD["sweeps"]["packet_flips"]
    aside = rec["set_aside"]
    assert len(images) == len(rec["rows"]) == 1288
    assert len(aside) == 37 and len(aside) * 20 <= len(images)
    for k, (img, (r, samples, _)) in enumerate(zip(images, decode(images))):
        if str(k) in aside:
            check_against_port(img, r, samples, k)
            assert r.status == op.FD_EOF
            continue
        row = gpu_row(r, samples)
        row[3] = row[3][:16]
        assert row == rec["rows"][k], k


def test_tone8_packet_flips():
    """the first 4,000 bit flips of the second audio packet of tone8.flac in
    one batch; none is set aside"""
    images = cases.tone8_flips()
    rec = GOLD["sweeps"]["tone8_flips"]
    assert not rec["set_aside"] and len(rec["rows"]) == len(images) == 4000
    for k, (r, samples, _) in enumerate(decode(images)):
        row = gpu_row(r, samples)
        row[3] = row[3][:16]
        assert row == rec["rows"][k], k
        assert r.n_frames == 1


def test_isolation():
    """one damaged stream of each Ogg failure kind, and one whose last page's
    lacing promises 65 KB past the end of the batch buffer, each between two
    valid streams: the neighbours' PCM and MD5 are unchanged"""
    pk, _ = op.flac_packets(cases.source("tone8"))
    good = op.mux(pk, segs_per_page=40, seed=3)
    alone = decode([good])[0]
    assert gpu_class(alone[0]) == ""
    h = cases.header_cases()
    # the last page's header and a lacing table of 255 x 255 with no body
    pages, _, _, _ = op.read_pages(good)
    last = pages[-1][0]
    liar = good[:last] + op.page([255] * 255, b"", flags=4)
    bad = [h["header:page_magic"], h["header:page_version"], h["header:page_crc"],
           cases.edge_cases()["end:no_eos"], h["header:no_packets"], h["header:packet_byte"], liar]
    want = ["ogg:1", "ogg:2", "ogg:3", "ogg:4", "ogg:5", "header", "ogg:4"]
    for b, cls in zip(bad, want):
        # the damaged stream last as well: its claim then points past the buffer
        for batch in ([good, b, good], [good, good, b]):
            res = decode(batch)
            for i, img in enumerate(batch):
                r, samples, _ = res[i]
                if img is good:
                    assert gpu_class(r) == "" and bytes(r.md5) == bytes(alone[0].md5)
                    assert np.array_equal(samples, alone[1])
                else:
                    assert gpu_class(r) == cls
                    check_against_port(img, r, samples, cls)


def test_host_and_device_entries_agree():
    import torch
    from audiotools import _atgpu
    built = cases.edge_cases()
    names = ["lacing:bigframe", "lacing:cut100", "end:md5_wrong", "ignored:scrambled"]
    data, tracks = _atgpu.oggflac_pack([built[n] for n in names])
    dec = _atgpu.decoder()
    pcm, res, sizes = dec.decode_oggflac(data, tracks)
    buf = torch.frombuffer(bytearray(data + bytes(64)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    dres, d_pcm, ns = dec.decode_oggflac_device(buf.data_ptr(), len(data), tracks)
    assert ns == len(pcm)
    out = torch.empty(max(1, ns), dtype=torch.int32, device="cuda")
    _atgpu.engine().copy_device(out.data_ptr(), d_pcm, 4 * ns)
    assert np.array_equal(out.cpu().numpy()[:ns], pcm)
    fields = [f for f, _ in _atgpu.OggFlacDecResult._fields_ if f not in ("md5", "streaminfo_md5")]
    assert all(r.sample_offset == r.pcm_offset * r.channels for r in res)
    for a, b in zip(res, dres):
        assert [getattr(a, f) for f in fields] == [getattr(b, f) for f in fields]
        assert bytes(a.md5) == bytes(b.md5)
    times = dec.kernel_times()
    assert list(times)[-3:] == ["ogg_walk", "ogg_crc", "ogg_gather"]


def test_batch_of_three_and_limits():
    from audiotools import _atgpu
    built = cases.edge_cases()
    imgs = [built["lacing:packet765"], cases.header_cases()["header:short20"],
            built["lacing:junk_tail"]]
    res = decode(imgs)
    assert [gpu_class(r) for r, _, _ in res] == ["", "header", ""]
    for img, (r, samples, _) in zip(imgs, res):
        check_against_port(img, r, samples, "batch")
    # an image beyond ATG_OGG_MAX_IMAGE_BYTES is refused before any launch
    t = _atgpu.oggflac_dec_track(0, _atgpu.OGG_MAX_IMAGE_BYTES + 1)
    with pytest.raises(_atgpu.ATGError) as e:
        _atgpu.decoder().decode_oggflac(bytes(16), [t])
    assert e.value.status == _atgpu.ATG_ERR_UNSUPPORTED
    assert decode([]) == []
