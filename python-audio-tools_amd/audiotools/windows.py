"""audiotools.windows — any span of a file without the rest of it.

Every other batch entry decodes whole files.  decode_windows_batch takes one
window (start, length, in PCM frames at the source's rate) per row, finds the
bytes that cover it and the first unit that can be decoded on its own, uploads
only those bytes and decodes only those units:

  flac     the SEEKTABLE points round the window bound the bytes (the whole
           frame region where there is none); the frame index
           (csrc/flac_index.hip) then lists the frame starts inside them and
           the row starts at the last listed frame at or before `start`
  tta      frame start // block, its byte from the seektable's sizes
  alac     frameset start // max_samples_per_frame, its byte from stsz
  wavpack  the last block set whose block_index <= start
  pcm      (WAV, AIFF, AU) byte arithmetic on the data chunk
  oggflac, shn   no table to start from: decoded whole, then viewed

plan_window is the arithmetic alone (pure Python over the _Header that
batchfiles._open returns); this module imports no torch.  Everything runs on
the default device.
"""

import bisect
import ctypes
from collections import namedtuple

import numpy as np

from . import _atgpu
from . import pcmfiles
from .batchfiles import _open, _read

__all__ = ["Plan", "WindowBatch", "plan_window", "refine_flac", "decode_windows_batch"]

# byte_start / byte_end: the bytes of header.image to upload; unit: the first
# unit to decode (flac: the byte of header.image its first frame is at, tta:
# frame, alac: frameset, wavpack: set, pcm: PCM frame, else 0); first_sample:
# the PCM frame that unit starts with; lead: decoded frames to drop in front;
# keep: frames of the window; decode: the frames asked of the decoder, whole
# units from first_sample on; exact: only the units of the window are decoded
Plan = namedtuple("Plan", "kind exact byte_start byte_end unit first_sample lead keep decode")

_FD_MD5 = 16  # ATG_FD_*: the statuses below it name the frame that stopped the decode
PLACEHOLDER = 0xFFFFFFFFFFFFFFFF  # a SEEKTABLE point that points nowhere
_WHOLE = ("oggflac", "shn")


def _clip(total, start, length):
    """the window cut to the stream -> (start, keep)"""
    start, total = int(start), int(total)
    if start < 0 or (length is not None and int(length) < 0):
        raise ValueError("a window's start and length must not be negative")
    if start >= total:
        return start, 0
    return start, total - start if length is None else min(int(length), total - start)


def flac_seekpoints(header):
    """the SEEKTABLE of a FLAC _Header as read_metadata gives it"""
    return _atgpu.read_metadata(header.image, max(1, header.info.n_seekpoints))[2]


def _flac_points(seekpoints, body_bytes, total):
    """usable points, ascending: (sample, byte offset from the first frame)"""
    pts = sorted(set((int(s), int(b)) for s, b, _ in seekpoints
                     if int(s) != PLACEHOLDER and int(s) < total and int(b) < body_bytes))
    out = []
    for s, b in pts:  # a table that runs backwards is not trusted past that point
        if out and (b < out[-1][1] or s == out[-1][0]):
            break
        out.append((s, b))
    return out


def source_tables(header):
    """what plan_window derives from a file's tables, made once per source:
    the byte prefix sums of the True Audio / ALAC unit sizes, a WavPack
    table's block_index and set columns"""
    if header.kind in ("tta", "alac"):
        sizes = np.asarray(header.info[1], dtype=np.uint64)
        return {"prefix": np.concatenate([np.zeros(1, np.uint64), np.cumsum(sizes)])}
    if header.kind == "wavpack":
        info, blocks = header.info
        n = int(info.n_blocks) - int(info.tail_blocks)
        return {"index": np.array([blocks[k].block_index for k in range(n)], dtype=np.int64),
                "set": np.array([blocks[k].set for k in range(n)], dtype=np.int64)}
    return {}


def plan_window(header, start, length=None, seekpoints=None, tables=None):
    """Plan of the window [start, start + length) of a file (`header`: the
    _Header batchfiles._open returns; length None: to the end).  The window is
    cut to the stream; one that starts at or past the end keeps 0 frames and
    covers no bytes.  seekpoints: a FLAC file's SEEKTABLE where the caller
    has read it already; tables: source_tables(header) likewise.  ValueError
    for a negative start or length."""
    kind = header.kind
    if tables is None:
        tables = source_tables(header)
    start, keep = _clip(header.total_frames, start, length)
    if keep == 0:
        return Plan(kind, kind not in _WHOLE, 0, 0, 0, start, 0, 0, 0)
    end = start + keep
    if kind == "flac":
        si = header.info
        body = len(header.image) - int(si.frames_offset)
        pts = _flac_points(flac_seekpoints(header) if seekpoints is None else seekpoints,
                           body, int(si.total_samples))
        samples = [s for s, _ in pts]
        k = bisect.bisect_right(samples, start) - 1
        s0, b0 = pts[k] if k >= 0 else (0, 0)
        k = bisect.bisect_right(samples, end)
        s1, b1 = pts[k] if k < len(pts) else (int(si.total_samples), body)
        f0 = int(si.frames_offset)
        # whole frames: a frame cut short by the count fails its CRC-16
        return Plan(kind, True, f0 + b0, f0 + b1, f0 + b0, s0, start - s0, keep, s1 - s0)
    if kind == "tta":
        info, sizes = header.info
        block = int(info.block_size)
        first, last = start // block, (end - 1) // block
        prefix = tables["prefix"]
        last = min(last, len(sizes) - 1)
        if first > last:
            return Plan(kind, True, 0, 0, first, first * block, 0, 0, 0)
        b0 = int(info.frames_offset) + int(prefix[first])
        b1 = int(info.frames_offset) + int(prefix[last + 1])
        whole = min((last + 1) * block, int(info.total_pcm_frames)) - first * block
        return Plan(kind, True, b0, b1, first, first * block, start - first * block, keep, whole)
    if kind == "alac":
        info, sizes = header.info
        per = int(info.max_samples_per_frame)
        if per == 0 or len(sizes) == 0:  # no stsz: the serial walk from mdat's start
            return Plan(kind, False, int(info.mdat_offset), len(header.image), 0, 0, start, keep,
                        int(info.total_frames))
        first, last = start // per, min((end - 1) // per, len(sizes) - 1)
        if first > last:
            return Plan(kind, True, 0, 0, first, first * per, 0, 0, 0)
        prefix = tables["prefix"]
        b0 = int(info.mdat_offset) + int(prefix[first])
        b1 = int(info.mdat_offset) + int(prefix[last + 1])
        whole = min((last + 1) * per, int(info.total_frames)) - first * per
        return Plan(kind, True, b0, b1, first, first * per, start - first * per, keep, whole)
    if kind == "wavpack":
        info, blocks = header.info
        index, sets = tables["index"], tables["set"]
        # the table ascends: the last set that starts at or before the window
        last = int(np.searchsorted(index, start, side="right")) - 1
        if last < 0:
            return Plan(kind, True, 0, 0, 0, 0, 0, 0, 0)
        first = int(np.searchsorted(sets, sets[last], side="left"))
        stop = int(np.searchsorted(index, end, side="left"))
        b0 = int(blocks[first].offset)
        b1 = max(int(blocks[k].offset) + 32 + int(blocks[k].size) for k in range(first, stop))
        s0 = int(blocks[first].block_index)
        s1 = int(blocks[stop - 1].block_index) + int(blocks[stop - 1].block_samples)
        return Plan(kind, True, b0, b1, int(blocks[first].set), s0, start - s0, keep, s1 - s0)
    if kind == "pcm":
        i = header.info
        per = i.channels * (i.bits_per_sample // 8)
        keep = max(0, min(end, int(i.frames)) - start)  # a truncated data chunk ends sooner
        if keep == 0:
            return Plan(kind, True, 0, 0, start, start, 0, 0, 0)
        b0 = int(i.data_offset) + start * per
        return Plan(kind, True, b0, b0 + keep * per, start, start, 0, keep, keep)
    # oggflac, shn: decoded whole
    return Plan(kind, False, 0, len(header.image), 0, 0, start, keep, int(header.total_frames))


def refine_flac(plan, entries):
    """a FLAC Plan started at the last listed frame at or before the window
    and ended at the first listed frame at or past its end.  entries: the
    frame index of the plan's bytes, [(byte_offset from plan.byte_start,
    first_sample, block_size)] ascending by byte.  Entries count only as far
    as they run on from each other (a stream whose headers all carry one
    number lists frames the planner cannot place); with none that serves, the
    plan stands."""
    if plan.keep == 0:
        return plan
    start, end = plan.first_sample + plan.lead, plan.first_sample + plan.lead + plan.keep
    at, reach = None, None
    for off, sample, bs in entries:
        if reach is not None and sample < reach:
            break
        if sample < plan.first_sample:
            continue
        reach = sample + bs
        if sample <= start:
            at = (off, sample)
        elif sample >= end:
            return _cut(plan, at, (off, sample))
    return _cut(plan, at, None)


def _cut(plan, at, stop):
    """plan from the entry `at` to the entry `stop` (byte offset, sample), each
    None to keep the plan's own end"""
    b1, s1 = plan.byte_end, plan.first_sample + plan.decode
    if stop is not None:
        b1, s1 = plan.byte_start + stop[0], stop[1]
    off, sample = (0, plan.first_sample) if at is None else at
    return plan._replace(byte_start=plan.byte_start + off, byte_end=b1,
                         unit=plan.byte_start + off, first_sample=sample,
                         lead=plan.first_sample + plan.lead - sample, decode=s1 - sample)


def _merge(spans):
    """[(b0, b1)] -> the disjoint pieces that cover them, ascending"""
    out = []
    for b0, b1 in sorted(s for s in spans if s[1] > s[0]):
        if out and b0 <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b1)
        else:
            out.append([b0, b1])
    return out


class WindowBatch(object):
    """the rows of one decode_windows_batch call, in device memory until
    close().  rows[k] is a DevicePcm (int32, interleaved: device pointer,
    sample offset, frames), None for a row with an error; sample_rate,
    channels, bits_per_sample and channel_mask are lists with one entry per
    row (0 for a source that could not be opened); errors[k] is the row's
    DecodingError or None; stats[k] is a dict of uploaded_bytes (the bytes
    that cover the row's window), decoded_frames and exact (False where the
    format has no table to start from and the whole stream was decoded).
    uploaded_total is what the call uploaded: rows that share a source share
    the union of their bytes."""

    def __init__(self, n):
        self.rows = [None] * n
        self.sample_rate, self.channels = [0] * n, [0] * n
        self.bits_per_sample, self.channel_mask = [0] * n, [0] * n
        self.errors = [None] * n
        self.stats = [dict(uploaded_bytes=0, decoded_frames=0, exact=True) for _ in range(n)]
        self.uploaded_total = 0
        self._free = []

    def fetch(self, k):
        """row k in host memory: int32, interleaved; the row's error raises"""
        if self.errors[k] is not None:
            raise self.errors[k]
        row = self.rows[k]
        out = np.empty(row.frames * self.channels[k], dtype=np.int32)
        if out.size:
            _atgpu.engine().copy_to_host(out, row.d_pcm + 4 * row.sample_offset)
        return out

    def close(self):
        eng = _atgpu.engine() if self._free else None
        for d in self._free:
            eng.device_free(d)
        self._free = []
        self.rows = [None] * len(self.rows)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _per_row(value, n, what):
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != n:
            raise ValueError("%s has %d entries for %d rows" % (what, len(value), n))
        return [None if v is None else int(v) for v in value]
    return [None if value is None else int(value)] * n


def _name(source):
    return source if isinstance(source, str) else "<%d-byte image>" % len(source)


class _Row(object):
    __slots__ = ("k", "src", "name", "header", "plan", "tables", "slot", "nbytes")


def _track_flac(r, at):
    h, p = r.header, r.plan
    t = _atgpu.DecTrack()
    t.data_offset, t.data_bytes = at, r.nbytes
    t.total_samples = p.decode
    t.sample_rate, t.channels = h.info.sample_rate, h.info.channels
    t.bits_per_sample, t.max_block_size = h.info.bits_per_sample, h.info.max_block_size
    return t  # md5 left zero: unchecked


def _track_tta(r, at):
    info, sizes = r.header.info
    p = r.plan
    block = int(info.block_size)
    n = (p.lead + p.keep + block - 1) // block
    t = _atgpu.tta_dec_track(at, r.nbytes, info, sizes[p.unit:p.unit + n])
    t.start = 0
    t.remaining = p.decode  # whole frames: a frame's CRC-32 stands behind its last sample
    return t


def _track_alac(r, at):
    info, sizes = r.header.info
    p = r.plan
    if not p.exact:
        return _atgpu.alac_dec_track(at, r.nbytes, info, start=0)
    per = int(info.max_samples_per_frame)
    n = (p.lead + p.keep + per - 1) // per  # whole framesets
    return _atgpu.alac_dec_track(at, r.nbytes, info, start=0, remaining=p.decode,
                                 frameset_bytes=sizes[p.unit:p.unit + n])


def _track_wavpack(r, at):
    info, blocks = r.header.info
    p = r.plan
    end = p.first_sample + p.lead + p.keep
    first = int(np.searchsorted(r.tables["set"], p.unit, side="left"))
    stop = int(np.searchsorted(r.tables["index"], end, side="left"))
    picked = [blocks[k] for k in range(first, stop)]
    table = (_atgpu.WvBlock * max(1, len(picked)))()
    for j, b in enumerate(picked):
        ctypes.memmove(ctypes.byref(table[j]), ctypes.byref(b), ctypes.sizeof(_atgpu.WvBlock))
        table[j].offset = int(b.offset) - p.byte_start
    t = _atgpu.WvDecTrack()
    t._blocks = table
    t.data_offset, t.data_bytes = at, r.nbytes
    t.blocks, t.n_blocks, t.tail_blocks = table, len(picked), 0
    t.channels, t.bits_per_sample = info.channels, info.bits_per_sample
    t.end_status, t.check_md5 = 0, 0
    return t


def _track_oggflac(r, at):
    return _atgpu.oggflac_dec_track(at, r.nbytes)


def _track_shn(r, at):
    return _atgpu.shn_dec_track(at, r.nbytes, r.header.info)


def _result(kind, res, channels):
    """-> (ok, sample offset, frames) of a decoder's result"""
    if kind == "flac":
        # pcm_frames counts the frames before the one that raised `status`
        # (flac_decode.hip stops it at the first bad frame), so with a status
        # of a frame (CRC, EOF, a bad header: all below FD_MD5) the caller's
        # "the window's frames came out" means the stop lies past the window;
        # FD_MD5 counts every frame and is refused outright
        return res.status < _FD_MD5, res.pcm_offset * channels, res.pcm_frames
    if kind == "oggflac":
        return res.status == 0 and res.ogg_status == 0, res.sample_offset, res.pcm_frames
    if kind == "shn":
        return res.status == _atgpu.SHN_END_OF_STREAM, res.pcm_offset, res.pcm_frames
    return res.status == 0, res.sample_offset, res.pcm_frames


def _decoder(kind):
    if kind in ("flac", "oggflac"):
        dec = _atgpu.decoder()
        return dec, (dec.decode_device if kind == "flac" else dec.decode_oggflac_device)
    dec = getattr(_atgpu, {"alac": "alac_decoder", "tta": "tta_decoder",
                           "wavpack": "wv_decoder", "shn": "shn_decoder"}[kind])()
    return dec, dec.decode_device


# in this order, as batchfiles._Batch decodes
_KINDS = ("flac", "oggflac", "alac", "tta", "wavpack", "shn")


def decode_windows_batch(sources, starts, lengths=None):
    """one window of each source -> WindowBatch.  sources: filenames or byte
    images of FLAC, Ogg FLAC, ALAC, True Audio, WavPack, Shorten, WAV, AIFF
    or Sun AU, told apart by magic; a source may appear in many rows and is
    read and opened once.  starts, lengths: an int or one per row, in PCM
    frames at the source's rate; a length of None runs to the end.  A window
    past the end is cut, one that starts at or past the end gives an empty
    row and no error; a negative start or length raises ValueError before any
    GPU work.

    Only the bytes that cover a row's window are uploaded (rows of one source
    share the union of theirs) and only its units are decoded, one decode
    call per format (FLAC: one per channel count among the rows): see
    plan_window.  Only the frames decoded are checked:
    damage outside the window is not an error, damage inside it is that row's
    DecodingError and stops nothing.  The stream's MD5 is never checked for a
    window, not even for one that spans the whole stream."""
    out, rows, _ = plan_rows(sources, starts, lengths)
    return decode_rows(out, rows)


def plan_rows(sources, starts, lengths=None):
    """the host half of decode_windows_batch: every distinct source read and
    opened once and every row planned -> (WindowBatch with the rows'
    parameters, the errors of sources that cannot be opened and the empty
    rows filled in; the rows still to decode; the _Header (or None) of every
    row).  No GPU work; ValueError as decode_windows_batch raises it."""
    from . import DecodingError
    from .pcmconverter import DevicePcm
    sources = list(sources)
    n = len(sources)
    starts = _per_row(starts, n, "starts")
    lengths = _per_row(lengths, n, "lengths")
    for s, l in zip(starts, lengths):
        if s is None or s < 0 or (l is not None and l < 0):
            raise ValueError("a window's start and length must not be negative")
    out = WindowBatch(n)
    # every distinct source read and opened once
    index, headers, points, tables = {}, [], [], []
    rows, row_headers = [], []
    for k, source in enumerate(sources):
        key = source if isinstance(source, str) else id(source)
        if key not in index:
            image = _read(source)
            index[key] = len(headers)
            headers.append(None if image is None else _open(image))
            points.append(None)
            tables.append(None)
        i = index[key]
        h = headers[i]
        row_headers.append(h)
        if h is None:
            out.errors[k] = DecodingError("%s cannot be opened as audio" % _name(source))
            continue
        out.sample_rate[k], out.channels[k] = h.sample_rate, h.channels
        out.bits_per_sample[k], out.channel_mask[k] = h.bits_per_sample, h.channel_mask
        if tables[i] is None:  # once per source, whatever its rows
            tables[i] = source_tables(h)
            points[i] = flac_seekpoints(h) if h.kind == "flac" else []
        r = _Row()
        r.k, r.src, r.name, r.header, r.tables = k, i, _name(source), h, tables[i]
        r.plan = plan_window(h, starts[k], lengths[k], points[i], tables[i])
        out.stats[k]["exact"] = r.plan.exact
        out.stats[k]["uploaded_bytes"] = r.plan.byte_end - r.plan.byte_start
        if r.plan.keep == 0:
            out.rows[k] = DevicePcm(None, _atgpu.PCM_S32, 0, 0)
            continue
        rows.append(r)
    return out, rows, row_headers


def decode_rows(out, rows):
    """the device half: plan_rows' WindowBatch and rows -> the WindowBatch decoded"""
    from . import DecodingError
    from .pcmconverter import DevicePcm
    if not rows:
        return out
    eng = _atgpu.engine()
    try:
        _run(out, rows, eng, DecodingError, DevicePcm)
    except Exception:
        out.close()
        raise
    return out


def _run(out, rows, eng, DecodingError, DevicePcm):
    headers = {r.src: r.header for r in rows}
    # the union of every source's bytes, 16-byte aligned pieces of one buffer
    pieces, pos = {}, 0
    for i in sorted(set(r.src for r in rows)):
        for b0, b1 in _merge([(r.plan.byte_start, r.plan.byte_end) for r in rows if r.src == i]):
            pieces[(i, b0)] = (pos, b0, b1)
            out.uploaded_total += b1 - b0
            pos += (b1 - b0 + 15) // 16 * 16
    blob = np.zeros(pos + 64, dtype=np.uint8)
    by_src = {}
    for (i, b0), (at, _, b1) in pieces.items():
        blob[at:at + b1 - b0] = np.frombuffer(headers[i].image, dtype=np.uint8, count=b1 - b0,
                                              offset=b0)
        by_src.setdefault(i, []).append((b0, b1, at))
    first_byte = {}
    for i in by_src:
        by_src[i].sort()
        first_byte[i] = [b0 for b0, _, _ in by_src[i]]
    d_up = eng.device_alloc(len(blob))
    out._free.append(d_up)
    eng.copy_to_device(d_up, blob)

    def where(src, byte):
        """the place in the upload of byte `byte` of source `src`"""
        b0, b1, at = by_src[src][bisect.bisect_right(first_byte[src], byte) - 1]
        assert b0 <= byte < b1, "a row outside its source's pieces"
        return at + byte - b0

    # FLAC: the frame index over each distinct range, then the rows refined
    flac = [r for r in rows if r.header.kind == "flac"]
    if flac:
        spans = sorted(set((r.src, r.plan.byte_start, r.plan.byte_end) for r in flac
                           if r.plan.byte_end > r.plan.byte_start))
        table = [_atgpu.flac_index_range(where(i, b0), b1 - b0, headers[i].info)
                 for i, b0, b1 in spans]
        found = [[] for _ in spans]
        for rng, off, sample, bs in _atgpu.flac_index_device(d_up, len(blob), table):
            found[rng].append((off, sample, bs))
        lookup = {s: f for s, f in zip(spans, found)}
        for r in flac:
            si = r.header.info
            # fixed blocking with differing sizes: the frame numbers place nothing
            if si.min_block_size == si.max_block_size:
                r.plan = refine_flac(r.plan, lookup.get((r.src, r.plan.byte_start,
                                                         r.plan.byte_end), []))
    # WAV, AIFF, AU: unpacked from where they lie
    pcm_rows = [r for r in rows if r.header.kind == "pcm"]
    if pcm_rows:
        slot, runs = 0, []
        for r in pcm_rows:
            i = r.header.info
            runs.append((i, (where(r.src, r.plan.byte_start), r.plan.keep * i.channels, slot)))
            r.slot = slot
            slot += (r.plan.keep * i.channels + 3) // 4 * 4
        d_pcm = eng.device_alloc(4 * max(slot, 4))
        out._free.append(d_pcm)
        pcmfiles.unpack_groups([i for i, _ in runs], [x for _, x in runs], d_up,
                               len(blob) // 16 * 16, d_pcm, _atgpu.PCM_S32, max(slot, 4))
        for r in pcm_rows:
            out.rows[r.k] = DevicePcm(d_pcm, _atgpu.PCM_S32, r.slot, r.plan.keep)
            out.stats[r.k]["decoded_frames"] = r.plan.keep
    # the compressed formats: every row's own bytes gathered into a buffer of
    # disjoint 16-byte aligned images (rows of one source overlap in the
    # upload), then one decode call per format.  FLAC results place a row by
    # its PCM frame, which is a whole number only among rows of one channel
    # count: one call per channel count there
    groups = []
    for kind in _KINDS:
        mine = [r for r in rows if r.header.kind == kind]
        counts = sorted(set(r.header.channels for r in mine)) if kind == "flac" else [None]
        groups += [(kind, [r for r in mine if c is None or r.header.channels == c])
                   for c in counts if mine]
    for kind, mine in groups:
        pos = 0
        for r in mine:
            r.nbytes = r.plan.byte_end - r.plan.byte_start
            r.slot = pos
            pos += (r.nbytes + 15) // 16 * 16 + 16
        d_in = eng.device_alloc(pos + 64)
        try:
            for r in mine:
                if r.nbytes:
                    eng.copy_device(d_in + r.slot, d_up + where(r.src, r.plan.byte_start), r.nbytes)
            make = globals()["_track_" + kind]
            dec, call = _decoder(kind)
            res, d_pcm, total = call(d_in, pos, [make(r, r.slot) for r in mine])
            keep = eng.device_alloc(4 * max(total, 4))
            out._free.append(keep)
            if total:
                eng.copy_device(keep, d_pcm, 4 * total)
        finally:
            eng.device_free(d_in)
        for r, x in zip(mine, res):
            ok, at, frames = _result(kind, x, r.header.channels)
            p = r.plan
            out.stats[r.k]["decoded_frames"] = int(frames)
            # FLAC decodes on to the next frame start the index lists (see
            # _result), and a stream decoded whole runs to its end: damage
            # past the window shows in the status alone and is not the window's
            if frames < p.lead + p.keep or (p.exact and not ok):
                out.errors[r.k] = DecodingError("%s does not decode cleanly in the window"
                                                % r.name)
                continue
            out.rows[r.k] = DevicePcm(keep, _atgpu.PCM_S32, at + p.lead * r.header.channels,
                                      p.keep)
