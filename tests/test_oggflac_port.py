"""CPU: tests/oggflac_port.py -- the Ogg FLAC decode contract in Python, which
the GPU tests compare against -- gives what the REFERENCE's oggflacdec gave
for every record of tests/golden/oggflac_vectors.json (made by
tests/golden/make_oggflac_golden.py): return code, message class, byte count
and md5 of the PCM.  The cases on which oggflacdec dies of a signal (a frame
whose subframes end within the last two bytes of its packet: it reads the
CRC-16 outside its error handler and aborts) are recorded by reason and are
FD_EOF here.  Where oracle/_ref/oggflacdec exists the comparison is also made
live."""
import hashlib
import os
import subprocess

import pytest

import oggflac_cases as cases
import oggflac_port as op

HERE = os.path.dirname(os.path.abspath(__file__))
REF_BIN = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "oggflacdec")
GOLD = cases.load_golden()


def outcome(image):
    d = op.decode(image)
    return d, [op.returncode(d), op.golden_class(d), len(d["pcm"]),
               hashlib.md5(d["pcm"]).hexdigest()]


def test_checksum_forms_agree():
    data = bytes((37 * k + (k >> 3)) & 0xFF for k in range(3001))
    assert op.ogg_crc(data) == op.ogg_crc_bytewise(data)
    assert op.ogg_crc(data[1000:], op.ogg_crc(data[:1000])) == op.ogg_crc_bytewise(data)
    # the page checksum of a known page: an empty end-of-stream page
    assert op.page([], b"", flags=4)[22:26] == op.ogg_crc_bytewise(
        op.page([], b"", flags=4, checksum=0)).to_bytes(4, "little")


def test_single_cases_match_reference():
    built = cases.single_cases()
    assert sorted(built) == sorted(GOLD["single"])
    for name, img in sorted(built.items()):
        rec = GOLD["single"][name]
        assert hashlib.sha256(img).hexdigest() == rec["sha256"], name
        d, got = outcome(img)
        if "set_aside" in rec:
            assert d["status"] == op.FD_EOF, name
            continue
        assert got == [rec["returncode"], rec["class"], rec["bytes"], rec["md5"]], name


@pytest.mark.parametrize("sweep", sorted(cases.SWEEPS))
def test_sweeps_match_reference(sweep):
    images = cases.SWEEPS[sweep]()
    rec = GOLD["sweeps"][sweep]
    assert len(images) == len(rec["rows"])
    for k, img in enumerate(images):
        d, got = outcome(img)
        if str(k) in rec["set_aside"]:
            assert d["status"] == op.FD_EOF, (sweep, k)
            continue
        got[3] = got[3][:16]
        assert got == rec["rows"][k], (sweep, k)


def test_bases_and_counts():
    """what the generator measured with oggflacdec: every raw flip and
    truncation is caught by the container, nothing set aside there or among
    the tone8 flips; 37 of the 1,288 packet flips (2.9 %, cap 5 %) make the
    reference abort"""
    img = cases.damage_base()[1]
    assert len(img) == GOLD["bases"]["damage_base_bytes"] == 220
    assert hashlib.sha256(img).hexdigest() == GOLD["bases"]["damage_base"]
    c = GOLD["counts"]
    assert c["raw_flips"]["cases"] == 1760 and c["raw_flips"]["set_aside"] == 0
    assert c["raw_flips"]["classes"] == {"ogg:3": 1654, "ogg:1": 64, "ogg:4": 26, "ogg:2": 16}
    assert c["raw_truncations"]["classes"] == {"ogg:4": 220}
    assert c["packet_flips"]["cases"] == 1288 and c["packet_flips"]["set_aside"] == 37
    assert c["packet_flips"]["set_aside"] * 20 <= c["packet_flips"]["cases"]
    assert set(GOLD["sweeps"]["packet_flips"]["set_aside"].values()) == {"reference: signal:-6"}
    assert c["tone8_flips"]["cases"] == cases.TONE8_FLIPS and c["tone8_flips"]["set_aside"] == 0
    for sweep in c:
        rows = GOLD["sweeps"][sweep]["rows"]
        assert all(r[0] in (0, 1) or str(k) in GOLD["sweeps"][sweep]["set_aside"]
                   for k, r in enumerate(rows))


@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/oggflacdec not built")
def test_live_against_reference(tmp_path):
    path = str(tmp_path / "d.oga")
    todo = list(cases.edge_cases().items()) + list(cases.header_cases().items())
    todo += [("flip%d" % k, img) for k, img in enumerate(cases.packet_flips()) if k % 16 == 0]
    for name, img in todo:
        with open(path, "wb") as f:
            f.write(img)
        p = subprocess.run([REF_BIN, path], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        d = op.decode(img)
        if p.returncode < 0:
            assert d["status"] == op.FD_EOF, name
        else:
            assert (op.returncode(d), d["pcm"]) == (p.returncode, p.stdout), name
