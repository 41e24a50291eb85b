"""The MLP case list shared by the golden generator (golden/make_mlp_golden.py),
the CPU tests and the GPU tests.  A case is a compact spec; expand() turns it
into the explicit title of tests/mlp_build.py, image_of() into an AOB image.

spec: seed, bits, rate (code), channels, substreams, split (channels of
substream 0), check, units, frames (per unit), every (a major sync and a
restart header every so many units), payloads, first (the title's first
sector), aobs (sectors in the first AOB file), plan (which features the
blocks carry) and the plan's own keys.
"""
import dvda_build
import mlp_build

STRADDLE2 = [2000, 1999, 1001, 7, 1500]
SMALL = [300, 290, 310]
TINY = [40, 7, 1, 0, 1, 7, 7, 0, 0, 1, 1, 7, 1, 7, 0, 7, 1, 1, 1, 7, 7]


def spec(name, seed, bits=16, channels=2, plan="plain", **kw):
    d = dict(name=name, seed=seed, bits=bits, channels=channels, plan=plan, rate=0,
             substreams=1, check=False, units=6, frames=16, every=4, payloads=SMALL, first=0)
    d.update(kw)
    return d


def ranges(s):
    """[(min, max, mmc)] per substream"""
    ch = s["channels"]
    if s["substreams"] == 1:
        return [(0, ch - 1, ch - 1)]
    a = s.get("split", max(1, ch // 2))
    return [(0, a - 1, a - 1), (a, ch - 1, ch - 1)]


def chan(s, c, u):
    """channel parameters of the plan at a restart header"""
    amp = s["bits"] - 5
    plan = s["plan"]
    p = {"codebook": 0, "lsbs": min(24, amp + 3)}
    if plan == "codebooks":
        p = {"codebook": 1 + (c + u) % 3, "lsbs": 2 + c % 3, "offset": 37 * c - 50}
    if plan in ("fir-restart", "filters") and u > 0:
        p.update(filters(s, c, u))
    if plan == "quant":
        p["lsbs"] = min(24, amp + 3)
        p["offset"] = -3 + c
    return p


def filters(s, c, u):
    """FIR and IIR parameters; the orders cycle over 0..8 with the channel
    and the unit, their sum at most 8, the shifts mixed"""
    fo = s.get("fir", (u + 3 * c) % 9)
    io = s.get("iir", (8 - fo) * ((u + c) % 2))
    shift = 7 + (c + u) % 3
    out = {}
    if fo:
        out["fir"] = {"order": fo, "shift": shift, "bits": 8, "cshift": c % 2,
                      "coef": [((29 * (i + 1) * (c + 2)) % 61) - 30 for i in range(fo)]}
    else:
        out["fir"] = {"order": 0}
    if io:
        out["iir"] = {"order": io, "shift": shift if fo and (u % 2) else (0 if fo else shift),
                      "bits": 7, "coef": [((17 * (i + 3)) % 41) - 20 for i in range(io)],
                      "state": {"bits": 9, "shift": 2,
                                "vals": [((i * 37 + c) % 200) - 100 for i in range(io)]}}
        if s.get("iir_state") is False:
            del out["iir"]["state"]
    else:
        out["iir"] = {"order": 0}
    return out


def restart_block(s, k, u, n):
    lo, hi, mmc = ranges(s)[k]
    blk = {"n": n, "amp": s["bits"] - 5,
           "restart": {"min": lo, "max": hi, "mmc": mmc, "noise_shift": s.get("noise_shift", 0),
                       "seed": (s["seed"] * 7919 + u * 104729) & 0x7FFFFF},
           "chan": dict((str(c), chan(s, c, u)) for c in range(lo, hi + 1))}
    plan = s["plan"]
    if plan == "codebooks":
        blk["symbols"] = list(range(18))
    if plan == "matrix" and k == s["substreams"] - 1:
        blk["matrices"] = matrices(s, mmc)
        blk["restart"]["noise_shift"] = 3
    if plan == "quant":
        blk["quant"] = [(c + u) % 4 for c in range(hi + 1)]
        blk["out_shift"] = [(2 * c + u) % 5 for c in range(mmc + 1)]
    if plan == "flags":
        # no block size, matrix, shift or offset fields from here on
        blk["flags"] = [1, 0, 1, 1, 1, 0, 0, 0]
        blk["n"] = 8
    return blk


def matrices(s, mmc):
    out = []
    for m in range(min(3, mmc + 1)):
        frac = [14, 6, 0][m]
        coef = [None] * (mmc + 3)
        coef[(m + 1) % (mmc + 1)] = -3 if frac else 1
        coef[m % (mmc + 1)] = (1 << frac) - 1 if frac else 1
        coef[mmc + 1 + m % 2] = 2 if frac else -1
        out.append({"out": m % (mmc + 1), "frac": frac, "bypass": (m + 1) % 2, "coef": coef})
    return out


def expand(s):
    """-> (title dict for mlp_build.build_stream, stream bytes)"""
    plan = s["plan"]
    title = dict(bits=s["bits"], rate=s["rate"], substreams=s["substreams"],
                 check=s["check"], units=[],
                 assignment=s.get("assignment", dvda_build.ASSIGNMENT[s["channels"]]))
    n = s["frames"]
    for u in range(s["units"]):
        head = u % s["every"] == 0
        unit = {"sync": head, "blocks": []}
        for k in range(s["substreams"]):
            lo, hi, mmc = ranges(s)[k]
            if plan in ("filters", "block2", "restart-inline") and n >= 16:
                # two blocks per unit; the second one changes parameters
                first = restart_block(s, k, u, n // 2) if head else {"absent": True}
                second = {"n": n - n // 2, "amp": s["bits"] - 5}
                if plan == "restart-inline" and u % 2:
                    second = restart_block(s, k, u + 100, n - n // 2)
                elif plan == "filters":
                    second["chan"] = dict((str(c), dict(chan(s, c, 0), **filters(s, c, u + 1)))
                                          for c in range(lo, hi + 1))
                else:
                    second["quant"] = [(c + u) % 3 for c in range(hi + 1)]
                    second["out_shift"] = [(c + u) % 3 for c in range(mmc + 1)]
                    second["chan"] = dict((str(c), dict(chan(s, c, 0), offset=u - 2 + c))
                                          for c in range(lo, hi + 1))
                if not head:
                    first = {"n": n // 2, "amp": s["bits"] - 5}
                blocks = [first, second]
            else:
                blocks = [restart_block(s, k, u, n) if head else {"absent": True}]
            unit["blocks"].append(blocks)
        title["units"].append(unit)
    damage(s, title)
    stream = mlp_build.build_stream(title, s["seed"])
    if s.get("partial"):
        stream = stream[:-s["partial"]]
    if s.get("no_sync"):
        stream = stream[:4] + b"\0" + stream[5:]
    return title, stream


def damage(s, title):
    """the plan keys that make an error status"""
    bad = s.get("bad")
    if not bad:
        return
    u = title["units"][s.get("at", 2)]
    u0 = title["units"][s.get("at", 2) // s["every"] * s["every"]]
    blk = u0["blocks"][0][0]
    if bad == "sync":
        title["units"][s["every"]]["sync_fields"] = {"rate": 1}
    elif bad == "sync-count":
        title["units"][s["every"]]["sync_fields"] = {"count": 3}
    elif bad == "extraword":
        u["extraword"] = (0,)
    elif bad == "restart":
        blk["restart"]["sync"] = 0x18F4
    elif bad == "block-size":
        blk["block_size"] = 7
    elif bad == "matrix":
        blk["matrices"] = [{"out": 7, "frac": 0, "coef": []}]
    elif bad == "fir-order":
        blk["chan"]["0"]["fir"] = {"order": 9}
    elif bad == "code":
        blk["chan"]["0"].update(codebook=2, lsbs=1)
        blk["symbols"] = [3, 4, -1]
    elif bad == "filter-sum":
        blk["chan"]["0"].update(
            fir={"order": 5, "shift": 3, "bits": 4, "coef": [1] * 5},
            iir={"order": 4, "shift": 3, "bits": 4, "coef": [1] * 4,
                 "state": {"bits": 4, "shift": 0, "vals": [0] * 4}})
    elif bad == "parity":
        u["bad_parity"] = 0
    elif bad == "crc":
        u["bad_crc"] = s["substreams"] - 1
    elif bad == "short":
        u["ends"] = [4000, 4000]
    elif bad == "words":
        u["words"] = 1
    elif bad == "frames":
        blk["chan"] = dict((c, {"codebook": 0, "lsbs": 0}) for c in blk["chan"])
        u0["blocks"][0] = [dict(blk, n=500)] + [{"absent": True}] * 9
    elif bad == "channels":
        blk["restart"].update(max=0, mmc=0)
        blk["chan"] = {"0": blk["chan"]["0"]}
    else:
        raise ValueError(bad)


def image_of(s):
    """-> (image, first sector of the title)"""
    _, stream = expand(s)
    img = mlp_build.image(stream, s["payloads"], **s.get("sector", {}))
    if s.get("bad_sector") is not None:
        b = bytearray(img)
        b[s["bad_sector"] * 2048 + 2] ^= 0xFF
        img = bytes(b)
    if s["first"]:
        lead, _ = dvda_build.aob_image(dict(seed=99, bits=16, assignment=1, rate=0,
                                            payloads=[100] * s["first"]))
        img = lead + img
    return img, s["first"]


def title_cases():
    out = []
    for ch, nss in ((1, 1), (2, 1), (3, 1), (6, 1), (2, 2), (3, 2), (6, 2)):
        for bits in (16, 24):
            out.append(spec("plain-%d-%d-%d" % (ch, nss, bits), 10 * ch + nss + bits, bits, ch,
                            substreams=nss, check=bool(ch % 2), rate=[0, 1, 8][(ch + bits) % 3]))
    out.append(spec("straddle2", 1, 24, 6, units=30, frames=40, every=8, payloads=STRADDLE2,
                    check=True))
    out.append(spec("straddle3", 2, 16, 2, units=12, frames=24, payloads=TINY, check=True))
    out.append(spec("codebooks", 3, 24, 3, plan="codebooks", frames=40, units=6, every=1))
    out.append(spec("codebooks-2ss", 4, 16, 4, plan="codebooks", frames=24, units=4, every=2,
                    substreams=2, check=True))
    out.append(spec("filters", 5, 24, 3, plan="filters", frames=24, units=20, every=5))
    out.append(spec("filters-16", 6, 16, 2, plan="filters", frames=16, units=12, every=3,
                    check=True, substreams=2))
    out.append(spec("fir-restart", 7, 24, 2, plan="fir-restart", frames=16, units=8, every=2))
    out.append(spec("block2", 8, 24, 3, plan="block2", frames=20, units=8, every=4))
    out.append(spec("restart-inline", 9, 16, 2, plan="restart-inline", frames=16, units=8))
    out.append(spec("quant", 11, 24, 4, plan="quant", frames=12, units=6, every=2))
    out.append(spec("flags", 12, 16, 2, plan="flags", frames=8, units=6, every=3))
    out.append(spec("matrix", 13, 24, 3, plan="matrix", frames=16, units=8, every=4))
    out.append(spec("matrix-6-2ss", 14, 24, 6, plan="matrix", frames=8, units=6, every=2,
                    substreams=2, split=2, check=True))
    out.append(spec("matrix-16-1", 15, 16, 1, plan="matrix", frames=9, units=3, every=1))
    out.append(spec("partial", 16, 16, 2, partial=9))
    out.append(spec("one-unit", 17, 16, 1, units=1, frames=8, payloads=[2000]))
    out.append(spec("start-at-3", 18, 24, 2, first=3, check=True))
    out.append(spec("two-aobs", 19, 16, 2, units=12, aobs=2))
    out.append(spec("two-aobs-start-at-3", 20, 16, 2, units=12, first=3, aobs=4))
    for i, bad in enumerate(("sync", "sync-count", "extraword", "restart", "block-size", "matrix",
                             "fir-order", "code", "filter-sum", "parity", "crc", "short", "words",
                             "frames", "channels")):
        out.append(spec("bad-" + bad, 30 + i, 16, 2, bad=bad, at=4, units=8, every=2,
                        check=bad in ("parity", "crc"), payloads=[100, 90, 110]))
    out.append(spec("bad-crc-2ss", 50, 24, 4, bad="crc", at=3, substreams=2, check=True))
    out.append(spec("bad-sector", 51, 16, 2, bad_sector=2, units=12, payloads=[150]))
    out.append(spec("iir-no-state", 52, 16, 2, plan="filters", frames=16, units=4,
                    iir_state=False, fir=0, iir=3))
    return out


def other_cases():
    """titles the reference has no answer for (port and GPU only)"""
    return [spec("not-mlp", 60, sector={"codec": 0x80}),
            spec("no-major-sync", 61, no_sync=True)]


def flip_specs():
    """the two small images of the damage sweeps"""
    return {"check": spec("flip-check", 70, 16, 2, plan="block2", frames=16, units=4, every=2,
                          check=True, payloads=[60, 50, 1, 70]),
            "nocheck": spec("flip-nocheck", 71, 24, 3, plan="matrix", frames=8, units=4, every=2,
                            payloads=[80, 7, 90])}


def flip_bits(s):
    """every bit of the stream bytes of the first two units, and every header
    byte of the sectors (dvda_build.header_bits' rule) -> bit numbers of the
    image"""
    _, stream = expand(s)
    img, _ = image_of(s)
    words = lambda p: ((stream[p] & 15) << 8 | stream[p + 1]) * 2
    cover = words(0) + words(words(0))
    bits, pos = [], 0
    for sec in range(len(img) // 2048):
        d = img[sec * 2048:(sec + 1) * 2048]
        at = 14 + (d[13] & 7)
        head = 6 + 3 + d[at + 8] + 4 + d[at + 9 + d[at + 8] + 3]
        length = ((d[at + 4] << 8) | d[at + 5]) + 6 - head
        keep = list(range(at + head)) + [at + head + i for i in range(length) if pos + i < cover]
        keep += range(at + head + length, at + head + length + 6)
        pos += length
        bits += [8 * (sec * 2048 + b) + k for b in keep for k in range(8)]
    return bits


# ------------------------------------------------------- the golden file
# A sweep keeps one short string per distinct answer: a flag and eight hex
# digits of an MD5 over the title's result, its samples and, for "p", the
# reference's answer (stderr text and PCM bytes).  Flags: "p" the reference's
# answer counts; "a" set aside (the reference died, timed out, or a stated
# limit); "c" a sample leaves the title's bits (the ABI wraps, the reference
# clips); "n" typed not-MLP (the result does not carry the codec id).
PORT_KEYS = ("status", "stop_unit", "stop_sector", "good_frames", "access_units")


def ask_pts(res):
    """the PTS ticks asked of the reference for a title with this result:
    the frame count nearest at or below its frames when it decodes, 1000
    frames past them when it fails"""
    import aob_port
    ok = res["status"] == 0
    rate = res["sample_rate"] or 48000
    frames = res["good_frames"] + (0 if ok else 1000)
    pts = frames * 90000 // rate
    while ok and pts and aob_port.track_frames(pts, rate) > frames:
        pts -= 1
    while not ok and aob_port.track_frames(pts, rate) < frames:
        pts += 1
    return pts


def spec_digest(s):
    import hashlib
    import json
    return hashlib.md5(json.dumps(s, sort_keys=True).encode()).hexdigest()[:10]


def outcome(res, x, flag, answer=None):
    """res: a dict with PORT_KEYS; x: int32 samples; answer: (PCM bytes,
    stderr) of the reference, or of mlp_port.answer_from over a decoder's
    result, for flag "p" """
    import hashlib
    import json
    h = hashlib.md5(json.dumps([int(res[k]) for k in PORT_KEYS]).encode())
    h.update(x.astype("<i4").tobytes())
    if flag == "p":
        h.update(answer[1].encode())
        h.update(answer[0])
    return flag + h.hexdigest()[:8]


def unpack_flips(sweep):
    """a sweep's answers, one per flipped bit: "flips" holds an index into
    "outcomes" per bit, or [index, count] for a run"""
    out = []
    for f in sweep["flips"]:
        out += [sweep["outcomes"][f]] if isinstance(f, int) else [sweep["outcomes"][f[0]]] * f[1]
    return out
