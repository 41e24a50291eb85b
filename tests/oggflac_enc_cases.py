"""The Ogg FLAC *encoder* cases shared by tests/golden/make_oggflac_enc_golden.py
and the tests.  A case is one track: a tests/signals.py signal, FLAC-8 options
with its block size and padding, the Ogg options, and optionally explicit
frame sizes.  BATCH is the one call of 70 tracks; each of its tracks is a
case of its own for the port and the golden file."""
import functools
import json
import os

import numpy as np

import oggflac_mux_port as mp
import oracle_port
import signals

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "oggflac_enc_vectors.json")
RATE = 44100
DEFAULT = dict(page_segments=255, page_per_packet=True)
FILLED = dict(page_segments=255, page_per_packet=False)
BATCH_SERIAL = 0xFFFFFFF0
BATCH_TRACKS = 70
# the 255 k frame: one 256-sample stereo tone frame whose byte count the seed
# decides; make_oggflac_enc_golden.py searches seeds from 0 and records the
# first that gives a multiple of 255
MULT255 = dict(kind="tone", frames=256, ch=2, bps=16, block=256)


class Case(object):
    def __init__(self, name, kind, frames, ch, bps, seed, block, padding=4096, ogg=None,
                 frame_sizes=None, serial=0x1000):
        self.name, self.kind, self.frames, self.ch, self.bps = name, kind, frames, ch, bps
        self.seed, self.block, self.padding = seed, block, padding
        self.ogg = dict(DEFAULT, serial_number=serial, channel_mask=0)
        self.ogg.update(ogg or {})
        self.frame_sizes = frame_sizes

    def flac_options(self):
        o = dict(oracle_port.PRESETS["8"])
        o.update(block_size=self.block, padding_size=self.padding)
        return o

    def pcm(self):
        return _pcm(self.kind, self.frames, self.ch, self.bps, self.seed)

    def port(self):
        return _port(self)


@functools.lru_cache(maxsize=None)
def _pcm(kind, frames, ch, bps, seed):
    if not frames:
        return np.zeros(0, np.int32)
    x = signals.make(kind, frames, ch, bps, seed=seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _port(case):
    return mp.encode(case.pcm(), case.ch, case.bps, RATE, case.ogg,
                     frame_sizes=case.frame_sizes, **case.flac_options())


def mult255_seed():
    """the recorded seed of the 255 k case (None before the golden exists)"""
    if not os.path.exists(GOLDEN):
        return None
    with open(GOLDEN) as f:
        return json.load(f).get("mult255_seed")


def batch_lengths():
    """70 tracks of 0 .. 3000 PCM frames, an empty one in the middle"""
    n = [(k * 3000) // (BATCH_TRACKS - 1) for k in range(BATCH_TRACKS)]
    n[0], n[35], n[-1] = 0, 0, 3000
    n[1], n[2] = 1, 257
    return n


@functools.lru_cache(maxsize=None)
def batch_cases():
    return tuple(Case("batch:%02d" % t, "tone" if t % 3 else "noise", n, 2, 16, 500 + t, 256,
                 serial=BATCH_SERIAL + t) for t, n in enumerate(batch_lengths()))


@functools.lru_cache(maxsize=None)
def single_cases(seed255=-1):
    if seed255 == -1:
        seed255 = mult255_seed()
    c = []
    for ch in (1, 2, 8):
        for bps in (8, 16, 24):
            for lname, lay in (("default", DEFAULT), ("filled", FILLED)):
                c.append(Case("matrix:%dx%d:%s" % (ch, bps, lname), "tone", 700, ch, bps,
                              ch * 100 + bps, 192, ogg=lay))
    for S in (1, 2, 7, 255):
        for ppp in (True, False):
            c.append(Case("cuts:s%d:%s" % (S, "pp" if ppp else "fill"), "noise", 256 * 5 + 7, 2,
                          16, 11, 256, ogg=dict(page_segments=S, page_per_packet=ppp)))
    for S in (1, 255):
        c.append(Case("pad251:s%d" % S, "tone", 700, 2, 16, 12, 192, padding=251,
                      ogg=dict(page_segments=S)))
    if seed255 is not None:
        for lname, lay in (("default", DEFAULT), ("s1", dict(page_segments=1)),
                           ("filled", FILLED)):
            c.append(Case("mult255:%s" % lname, MULT255["kind"], MULT255["frames"],
                          MULT255["ch"], MULT255["bps"], seed255, MULT255["block"], ogg=lay))
    c.append(Case("pad0", "tone", 700, 2, 16, 13, 192, padding=0))
    c.append(Case("pad4096", "tone", 700, 2, 16, 14, 192, padding=4096))
    c.append(Case("pad70000", "tone", 700, 2, 16, 15, 192, padding=70000))
    c.append(Case("pad70000:s7", "tone", 700, 2, 16, 15, 192, padding=70000,
                  ogg=dict(page_segments=7)))
    c.append(Case("mask6x24", "tone", 700, 6, 24, 16, 192, ogg=dict(channel_mask=0x060F)))
    for lname, lay in (("default", DEFAULT), ("filled", FILLED)):
        c.append(Case("big8x24:%s" % lname, "noise", 4608 * 2 + 100, 8, 24, 17, 4608, ogg=lay))
    c.append(Case("big65535", "tone", 65535, 1, 16, 18, 65535))
    c.append(Case("empty", "tone", 0, 2, 16, 19, 4096))
    c.append(Case("one", "tone", 1, 2, 16, 20, 4096))
    c.append(Case("sizes", "tone", 5101, 2, 16, 21, 4096, frame_sizes=(4096, 1000, 5)))
    return tuple(c)


def all_cases(seed255=-1):
    return list(single_cases(seed255)) + list(batch_cases())


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
