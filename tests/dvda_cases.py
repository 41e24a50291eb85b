"""The DVD-Audio case list shared by the golden generator
(golden/make_dvda_golden.py), the CPU tests and the GPU tests.  A case is a
builder spec (dvda_build.aob_image) with the sector the title starts at, the
PTS ticks asked of the reference and, for the generator, how the image is
split over AOB files."""
import dvda_build as B

# payload bytes per sector.  STRADDLE2: chunks cross one sector boundary;
# TINY: payloads of 0, 1 and 7 bytes, so a chunk of up to 36 bytes is spread
# over three and more sectors
STRADDLE2 = [2000, 1999, 1001, 7]
STRADDLE2B = [2000, 1990, 35, 37]
TINY = [7, 1, 0, 1, 7, 7, 0, 0, 1, 1, 7, 1, 7, 0, 7, 1, 1, 1, 7, 7]
PADS = dict(pad1=[0, 3, 0, 0, 1], pad2=[9, 12, 9, 9, 9], stuffing=[0, 7, 2, 0, 0])


def spec(seed, bits, channels, payloads, rate=0, **kw):
    d = dict(seed=seed, bits=bits, assignment=B.ASSIGNMENT[channels], rate=rate,
             payloads=list(payloads))
    d.update(kw)
    return d


def frames_of(s):
    chunk = s["bits"] // 8 * B.CHANNELS[s["assignment"]] * 2
    return sum(s["payloads"]) // chunk * 2


def pts_for(frames, rate):
    """PTS ticks that aob.c's round(ticks * rate / 90000) turns into `frames`"""
    p = (frames * 90000 + rate // 2) // rate
    for t in (p, p - 1, p + 1):
        if t >= 0 and (2 * t * rate + 90000) // 180000 == frames:
            return t
    raise ValueError((frames, rate))


def flip_specs():
    """the two 5-sector images of the flip sweeps: 226 non-payload bytes each"""
    return {"s16x2": spec(101, 16, 2, [2000, 1993, 1001, 7, 1500], rate=8, **PADS),
            "s24x6": spec(102, 24, 6, STRADDLE2B + [1500], rate=1, **PADS)}


def title_cases():
    """[(name, spec, first sector, frames asked or None for `all but one
    chunk`, split)] -- every case asks for fewer frames than the sectors
    hold, so the reference's replay of its last packet stays out"""
    out = []
    for bits in (16, 24):
        for ch in range(1, 7):
            out.append(("layout-%d-%d" % (bits, ch),
                        spec(bits + ch, bits, ch, STRADDLE2 + [0, 1, 500], **PADS)))
            out.append(("tiny-%d-%d" % (bits, ch), spec(40 + bits + ch, bits, ch, TINY * 2)))
    out.append(("straddle2b-24-6", spec(1, 24, 6, STRADDLE2B * 3, rate=1)))
    out.append(("one-sector", spec(2, 16, 2, [2001])))
    out.append(("two-sectors", spec(3, 24, 2, [2006, 13])))
    out.append(("five-sectors", spec(4, 24, 3, [2012, 2006, 2001, 1999, 1987])))
    out.append(("forty-sectors", spec(5, 24, 5, [1980 - 7 * (i % 5) for i in range(41)],
                                      rate=10, **PADS)))
    out.append(("rate-44100", spec(6, 16, 2, [2000, 2000, 2000], rate=8)))
    out.append(("decoy-and-extras", spec(
        7, 16, 2, [600, 700, 800], before={"0": [(0xBF, 40)], "1": [(0xBE, 0), (0xE0, 100)]},
        after={"1": [(0xBF, 10)], "2": [(0xBB, 18)]}, decoy={"1": 300, "2": 64})))
    cases = []
    for name, s in out:
        n = frames_of(s)
        for tag, ask in (("below", n // 2 | 1), ("at", n), ("chunk-below", n - 2)):
            if ask >= 0:
                cases.append((name + ":" + tag, s, 0, ask, None))
    s = spec(8, 24, 4, STRADDLE2 * 2)
    cases.append(("start-at-3", s, 3, frames_of(s) - 2, None))
    s = spec(9, 16, 6, STRADDLE2 * 3)
    cases.append(("two-aobs", s, 0, frames_of(s) - 2, 5))
    cases.append(("two-aobs-start-at-3", s, 3, 100, 5))
    return cases


def first_packet_cases():
    """MLP-typed and unknown first packets (port and GPU only: the reference
    decodes MLP, which is not built yet)"""
    return [("mlp-first", spec(20, 16, 2, [1000, 900, 800], codec=0xA1, pad2=[6, 9, 9])),
            ("unknown-first", spec(21, 16, 2, [1000, 900, 800], codec=0x80, pad2=[4, 9, 9])),
            ("mlp-first-no-pad2", spec(22, 24, 2, [1234, 5], codec=0xA1, pad2=[0, 9]))]


def case_image(s, first):
    """the image a case's title sits in: `first` sectors of another title,
    then the spec's own"""
    img, x = B.aob_image(s)
    if first:
        lead, _ = B.aob_image(spec(99, 16, 2, [100] * first))
        img = lead + img
    return img, x


# ------------------------------------------------------- the golden file
def pack_golden(titles, sweeps):
    """the generator's records in the form kept on disk: a case's spec once
    under its base name, a sweep's answers as runs of [index per request ..., count]
    into the list of its distinct answers, and the count of its flipped bits (the bits themselves
    follow from the spec: dvda_build.header_bits)"""
    specs, packed_titles, packed_sweeps = {}, {}, {}
    for name, v in titles.items():
        base = name.split(":")[0]
        assert specs.setdefault(base, v["spec"]) == v["spec"]
        packed_titles[name] = {k: x for k, x in v.items() if k != "spec"}
    for name, v in sweeps.items():
        outcomes, runs = [], []
        for row in v["flips"]:
            for one in row:
                if one not in outcomes:
                    outcomes.append(one)
            key = [outcomes.index(one) for one in row]
            if runs and runs[-1][:-1] == key:
                runs[-1][-1] += 1
            else:
                runs.append(key + [1])
        packed_sweeps[name] = dict({k: x for k, x in v.items() if k not in ("bits", "flips")},
                                   n_bits=len(v["bits"]), outcomes=outcomes, flips=runs)
    return {"specs": specs, "titles": packed_titles, "sweeps": packed_sweeps}


def load_golden(path):
    """golden/dvda_vectors.json unpacked: titles[case] with its "spec";
    sweeps[name] with "bits" and, per bit, "flips" rows of one [return code,
    stderr, md5[:16], bytes] per entry of "pts" """
    import json
    with open(path) as f:
        d = json.load(f)
    for name, v in d["titles"].items():
        v["spec"] = d["specs"][name.split(":")[0]]
    for v in d["sweeps"].values():
        v["bits"] = B.header_bits(v["spec"])
        assert len(v["bits"]) == v["n_bits"]
        v["flips"] = [[v["outcomes"][i] for i in run[:-1]]
                      for run in v["flips"] for _ in range(run[-1])]
        assert len(v["flips"]) == v["n_bits"]
    return d
