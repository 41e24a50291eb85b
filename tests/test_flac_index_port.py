"""CPU: the Python restatement of the frame index's listing rule
(flac_index_port) against the reference decoder's frame walk
(oracle_port.decode_frames): over a whole stream's frame region the port
lists every frame the reference walks, with its block size and the sample it
starts at, and nothing else.  Then the rule's edges on cut and damaged
ranges."""
import os

import pytest

import flac_index_port as port
import oracle_port

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = (["fixtures/tone%d.flac" % k for k in range(1, 9)] +
            ["fixtures/flac-allframes.flac", "fixtures/flac-seektable.flac", "fixtures/1s.flac",
             "fixtures/1m.flac", "fixtures/1h.flac", "tone.flac"])


def load(name):
    return open(os.path.join(HERE, "golden", name), "rb").read()


def walked(data):
    """-> (si, [(byte offset from the first frame, first sample, block size)])
    of the reference's walk"""
    rc, _, _, si = oracle_port.read_metadata(data)
    assert rc == 0
    got = oracle_port.decode_frames(data, si)
    assert got["code"] == 0
    out, sample = [], 0
    for off, bs in got["offsets"]:
        out.append((off, sample, bs))
        sample += bs
    return si, out


@pytest.mark.parametrize("name", FIXTURES)
def test_whole_stream_lists_every_frame(name):
    data = load(name)
    si, want = walked(data)
    assert want
    got = port.index_range(data, si.frames_offset, len(data) - si.frames_offset, si)
    if name.endswith("flac-allframes.flac"):
        # a hand-made stream: every header carries frame number 0, so no frame
        # follows another, and each is closed by the stream's end instead
        # (whole frames in a row leave a zero residue)
        assert [e[1] for e in got] == [0] * len(want)
        want = [(off, 0, bs) for off, _, bs in want]
    assert got == want


def test_one_hour_of_silence_has_many_frames_per_segment():
    data = load("fixtures/1h.flac")
    si, want = walked(data)
    assert len(want) == 879 and len(data) < 65536


def test_cut_frames_are_absent():
    data = load("fixtures/tone2.flac")
    si, want = walked(data)
    f0 = si.frames_offset
    a, b = want[3][0], want[9][0]
    # from inside frame 2 to inside frame 9: frames 3..8 whole
    got = port.index_range(data, f0 + a - 5, (b + 7) - (a - 5), si)
    assert got == [(off - (a - 5), s, bs) for off, s, bs in want[3:9]]
    # the range's end stands in for a successor: frames 3..8 again, ending exactly
    got = port.index_range(data, f0 + a, b - a, si)
    assert got == [(off - a, s, bs) for off, s, bs in want[3:9]]
    assert port.index_range(data, f0 + a + 1, want[4][0] - a - 1, si) == []
    assert port.index_range(data, f0, 0, si) == []


def test_junk_after_a_frame():
    data = load("fixtures/tone2.flac")
    si, want = walked(data)
    f0, cut = si.frames_offset, si.frames_offset + want[1][0]
    bent = data[:cut] + b"\0\0" + data[cut:]
    got = port.index_range(bent, f0, len(bent) - f0, si)
    # zero bytes leave the zero residue at frame 0's end as it is, so frame 1's
    # header still closes it: starts are promised, lengths are not
    assert got == want[:1] + [(off + 2, s, bs) for off, s, bs in want[1:]]
    # other junk breaks the residue: frame 0 goes, the rest stay
    bent = data[:cut] + b"\x5a\xa5" + data[cut:]
    got = port.index_range(bent, f0, len(bent) - f0, si)
    assert got == [(off + 2, s, bs) for off, s, bs in want[1:]]


def test_a_wrong_number_is_not_followed():
    data = bytearray(load("fixtures/tone2.flac"))
    si, want = walked(bytes(data))
    f0 = si.frames_offset
    # frames 0..4, then frames 6..: frame 4's successor carries number 6
    a, b = f0 + want[5][0], f0 + want[6][0]
    bent = bytes(data[:a] + data[b:])
    got = port.index_range(bent, f0, len(bent) - f0, si)
    firsts = [e[1] for e in got]
    assert want[4][1] not in firsts and want[3][1] in firsts and want[6][1] in firsts
