"""audiotools.dvda — DVD-Audio discs: the disc structure of the reference's
audiotools/dvda.py restated for Python 3, over the GPU title decoder
(decoders.DVDA_Title, csrc/aob_decode.hip).

  DVDAudio(audio_ts_path)   AUDIO_TS.IFO and every ATS_XX_0.IFO parsed: the
                            titlesets' DVDATitle lists (.titlesets, [i]), the
                            upper-cased file inventory (.files) and the AOB
                            sector inventory (.aob_sectors)
  DVDATitle                 .tracks, .pts_length, info(), total_frames(),
                            to_pcm() -> decoders.DVDA_Title
  DVDATrack                 .first_pts .pts_length .first_sector .last_sector,
                            total_frames(), sectors()
  InvalidDVDA               with the reference's messages (text.py ERR_DVDA_*)
  tracks_to_flac_batch      dvda2track's job: tracks -> .flac files, decoded
                            and encoded on the device

Listing a disc needs no GPU: a title's attributes are read from its first
sector in plain Python, as the reference's __parse_info__ reads them.
Not here: CPPM (cdrom_device other than None raises ValueError) and
metadata_lookup (network).  to_pcm() passes the title's own titleset where
the reference hard-codes 1.
"""

import decimal
import os
import re
import struct

from . import DecodingError, EncodingError
from . import _atgpu

ERR_DVDA_IOERROR_AUDIO_TS = u"unable to open AUDIO_TS.IFO"
ERR_DVDA_INVALID_AUDIO_TS = u"invalid AUDIO_TS.IFO"
ERR_DVDA_IOERROR_ATS = u"unable to open ATS_%2.2d_0.IFO"
ERR_DVDA_INVALID_ATS = u"invalid ATS_%2.2d_0.IFO"
ERR_DVDA_INVALID_SECTOR_POINTER = u"invalid sector pointer"
ERR_DVDA_NO_TRACK_SECTOR = u"unable to find track sector in AOB files"
ERR_DVDA_INVALID_AOB_SYNC = u"invalid AOB sync bytes"
ERR_DVDA_INVALID_AOB_MARKER = u"invalid AOB marker bits"
ERR_DVDA_INVALID_AOB_START = u"invalid AOB packet start code"


class InvalidDVDA(Exception):
    pass


def _read(f, n):
    """n bytes or the IOError the reference's bitstream reader raises"""
    data = f.read(n)
    if len(data) != n:
        raise IOError("I/O error reading stream")
    return data


class DVDAudio(object):
    """an entire DVD-Audio disc: .titlesets[i] is the list of DVDATitle
    objects of one titleset, each of which holds DVDATrack objects"""

    SECTOR_SIZE = 2048
    PTS_PER_SECOND = 90000

    def __init__(self, audio_ts_path, cdrom_device=None):
        if cdrom_device is not None:
            raise ValueError("CPPM-protected discs are not supported: cdrom_device must be None")
        self.audio_ts_path = audio_ts_path
        self.cdrom_device = None
        # an inventory of AUDIO_TS files by upper-case name
        self.files = dict((name.upper(), os.path.join(audio_ts_path, name))
                          for name in os.listdir(audio_ts_path))
        self.titleset_numbers = list(self.__titlesets__())
        # the AOBs' [start, end) sectors, before the titles that look into them
        self.titleset_aobs = {}
        self.aob_sectors = []
        for titleset in self.titleset_numbers:
            pos, rows = 0, []
            for path in aob_paths(self.files, titleset):
                n = os.path.getsize(path) // DVDAudio.SECTOR_SIZE
                rows.append((path, pos, pos + n))
                pos += n
            self.titleset_aobs[titleset] = rows
            for _, start, end in rows:
                last = self.aob_sectors[-1][1] if self.aob_sectors else 0
                self.aob_sectors.append((last, last + (end - start)))
        self.titlesets = [self.__titles__(titleset) for titleset in self.titleset_numbers]

    def __getitem__(self, key):
        return self.titlesets[key]

    def __len__(self):
        return len(self.titlesets)

    def __titlesets__(self):
        """valid audio titleset numbers from AUDIO_TS.IFO"""
        try:
            f = open(self.files["AUDIO_TS.IFO"], "rb")
        except (KeyError, IOError):
            raise InvalidDVDA(ERR_DVDA_IOERROR_AUDIO_TS)
        with f:
            # 12b 32u 12P 32u 16u 4P 16u 16u 8u 4P 8u 32u 10P 8u 8u 40b
            head = _read(f, 12 + 4 + 12 + 4 + 2 + 4 + 2 + 2 + 1 + 4 + 1 + 4 + 10 + 1 + 1 + 40)
            if head[:12] != b"DVDAUDIO-AMG":
                raise InvalidDVDA(ERR_DVDA_INVALID_AUDIO_TS)
            audio_titlesets = head[63]
            for titleset in range(1, audio_titlesets + 1):
                if (("ATS_%2.2d_0.IFO" % titleset) in self.files and
                        ("ATS_%2.2d_1.AOB" % titleset) in self.files):
                    yield titleset

    def __titles__(self, titleset):
        """the DVDATitle objects of a titleset, from its ATS_XX_0.IFO"""
        try:
            f = open(self.files["ATS_%2.2d_0.IFO" % titleset], "rb")
        except (KeyError, IOError):
            raise InvalidDVDA(ERR_DVDA_IOERROR_ATS % titleset)
        with f:
            if f.read(12) != b"DVDAUDIO-ATS":
                raise InvalidDVDA(ERR_DVDA_INVALID_ATS % titleset)
            f.seek(DVDAudio.SECTOR_SIZE)
            title_count, _ = struct.unpack(">H2xI", _read(f, 8))
            title_offsets = [struct.unpack(">B3xI", _read(f, 8))[1] for _ in range(title_count)]
            titles = []
            for title_number, title_offset in enumerate(title_offsets):
                f.seek(DVDAudio.SECTOR_SIZE + title_offset)
                tracks, indexes, track_length, pointers_table = struct.unpack(
                    ">2xBBI4xH2x", _read(f, 16))
                timestamps = [struct.unpack(">4xBxII6x", _read(f, 20)) for _ in range(tracks)]
                f.seek(DVDAudio.SECTOR_SIZE + title_offset + pointers_table)
                pointers = [struct.unpack(">III", _read(f, 12)) for _ in range(indexes)]
                if len(pointers) > 1 and set(p[0] for p in pointers[1:]) != set([0x01000000]):
                    raise InvalidDVDA(ERR_DVDA_INVALID_SECTOR_POINTER)
                pointers = [None] + pointers
                title = DVDATitle(dvdaudio=self, titleset=titleset, title=title_number + 1,
                                  pts_length=track_length, tracks=[])
                for number, (stamp, following) in enumerate(zip(timestamps, timestamps[1:])):
                    index_number, first_pts, pts_length = stamp
                    title.tracks.append(DVDATrack(
                        dvdaudio=self, titleset=titleset, title=title, track=number + 1,
                        first_pts=first_pts, pts_length=pts_length,
                        first_sector=pointers[index_number][1],
                        last_sector=pointers[following[0] - 1][2]))
                if timestamps:
                    index_number, first_pts, pts_length = timestamps[-1]
                    title.tracks.append(DVDATrack(
                        dvdaudio=self, titleset=titleset, title=title, track=len(timestamps),
                        first_pts=first_pts, pts_length=pts_length,
                        first_sector=pointers[index_number][1], last_sector=pointers[-1][2]))
                title.__parse_info__()
                titles.append(title)
            return titles


def aob_paths(files, titleset):
    """the titleset's ATS_XX_1.AOB ... in order, from an upper-cased inventory"""
    pattern = re.compile("ATS_%2.2d_\\d\\.AOB$" % titleset)
    return [files[key] for key in sorted(files) if pattern.match(key)]


def find_aobs(audio_ts, titleset):
    """[(path, sectors)] of ATS_XX_1.AOB, ATS_XX_2.AOB ... as far as they
    are there, looked up without regard to case (aob.c open_sector_reader);
    IOError with ENOENT when the first is missing"""
    files = dict((name.upper(), os.path.join(audio_ts, name)) for name in os.listdir(audio_ts))
    out = []
    for i in range(1, 10):
        path = files.get("ATS_%2.2d_%d.AOB" % (titleset, i))
        if path is None:
            break
        out.append((path, os.path.getsize(path) // DVDAudio.SECTOR_SIZE))
    if not out:
        import errno
        raise IOError(errno.ENOENT, os.strerror(errno.ENOENT), audio_ts)
    return out


def read_sectors(aobs, first, count=None):
    """sectors [first, first + count) of the AOBs' sectors end to end (to
    their end when count is None); a file's remainder below 2048 bytes is
    not part of them"""
    parts, pos = [], 0
    last = sum(n for _, n in aobs) if count is None else first + count
    for path, n in aobs:
        a, b = max(first, pos), min(last, pos + n)
        if a < b:
            with open(path, "rb") as f:
                f.seek((a - pos) * DVDAudio.SECTOR_SIZE)
                parts.append(_read(f, (b - a) * DVDAudio.SECTOR_SIZE))
        pos += n
    return b"".join(parts)


class DVDATitle(object):
    """one title: DVDATrack objects through [i]"""

    def __init__(self, dvdaudio, titleset, title, pts_length, tracks):
        self.dvdaudio = dvdaudio
        self.titleset = titleset
        self.title = title
        self.pts_length = pts_length
        self.tracks = tracks
        self.sample_rate = 0
        self.channels = 0
        self.channel_mask = 0
        self.bits_per_sample = 0
        self.stream_id = 0

    def __parse_info__(self):
        """sample rate, channels, mask, bits and codec id from the first
        sector of the title's first track"""
        if len(self.tracks) == 0:
            return
        track_sector = self[0].first_sector
        for path, start, end in self.dvdaudio.titleset_aobs[self.titleset]:
            if start <= track_sector < end:
                break
        else:
            raise ValueError(ERR_DVDA_NO_TRACK_SECTOR)
        with open(path, "rb") as f:
            f.seek((track_sector - start) * DVDAudio.SECTOR_SIZE)
            head = _read(f, 14)
            bits = "{:0112b}".format(int.from_bytes(head, "big"))
            _read(f, int(bits[109:112], 2))
            if head[:4] != b"\x00\x00\x01\xba":
                raise InvalidDVDA(ERR_DVDA_INVALID_AOB_SYNC)
            if (bits[32:34], bits[37], bits[53], bits[69], bits[79], bits[102:104]) != \
                    ("01", "1", "1", "1", "1", "11"):
                raise InvalidDVDA(ERR_DVDA_INVALID_AOB_MARKER)
            # skip packets until one of stream 0xBD
            while True:
                start_code, stream_id, length = struct.unpack(">3sBH", _read(f, 6))
                if start_code != b"\x00\x00\x01":
                    raise InvalidDVDA(ERR_DVDA_INVALID_AOB_START)
                if stream_id == 0xBD:
                    break
                _read(f, length)
            pad1 = _read(f, 3)[2]
            _read(f, pad1)
            stream_id = _read(f, 3)[0]
            if stream_id == 0xA0:   # PCM: 8u 16u 8u 4u 4u 4u 4u 8u 8u
                p = _read(f, 8)
                group1_bps, group1_rate, assignment = p[4] >> 4, p[5] >> 4, p[7]
            else:                   # MLP: pad2, 4p 12u 16p 24u 8u 4u 4u 4u 4u 11u 5u 48u
                _read(f, _read(f, 1)[0])
                p = _read(f, 18)
                group1_bps, group1_rate, assignment = p[8] >> 4, p[9] >> 4, p[11] & 0x1F
            self.sample_rate = DVDATrack.SAMPLE_RATE[group1_rate]
            self.channels = DVDATrack.CHANNELS[assignment]
            self.channel_mask = DVDATrack.CHANNEL_MASK[assignment]
            self.bits_per_sample = DVDATrack.BITS_PER_SAMPLE[group1_bps]
            self.stream_id = stream_id

    def __len__(self):
        return len(self.tracks)

    def __getitem__(self, index):
        return self.tracks[index]

    def __repr__(self):
        return "DVDATitle(%s)" % ",".join(
            "%s=%s" % (key, getattr(self, key))
            for key in ["titleset", "title", "pts_length", "tracks"])

    def info(self):
        """(sample_rate, channels, channel_mask, bits_per_sample, codec id)"""
        return (self.sample_rate, self.channels, self.channel_mask, self.bits_per_sample,
                self.stream_id)

    def to_pcm(self):
        """a decoders.DVDA_Title over the title's sectors; its next_track()
        takes each track's PTS ticks in turn"""
        from .decoders import DVDA_Title
        return DVDA_Title(audio_ts=self.dvdaudio.audio_ts_path, titleset=self.titleset,
                          start_sector=self.tracks[0].first_sector,
                          end_sector=self.tracks[-1].last_sector)

    def total_frames(self):
        """the title's PCM frames, its PTS length rounded up"""
        return int((decimal.Decimal(self.pts_length) / DVDAudio.PTS_PER_SECOND *
                    self.sample_rate).quantize(decimal.Decimal(1), rounding=decimal.ROUND_UP))


class DVDATrack(object):
    """one track of a title"""

    SAMPLE_RATE = [48000, 96000, 192000, 0, 0, 0, 0, 0, 44100, 88200, 176400, 0, 0, 0, 0, 0]
    CHANNELS = [1, 2, 3, 4, 3, 4, 5, 3, 4, 5, 4, 5, 6, 4, 5, 4, 5, 6, 5, 5, 6] + [0] * 11
    CHANNEL_MASK = [0x4, 0x3, 0x103, 0x33, 0xB, 0x10B, 0x3B, 0x7, 0x107, 0x37, 0xF, 0x10F, 0x3F,
                    0x107, 0x37, 0xF, 0x10F, 0x3F, 0x3B, 0x37, 0x3F] + [0] * 11
    BITS_PER_SAMPLE = [16, 20, 24] + [0] * 13

    def __init__(self, dvdaudio, titleset, title, track, first_pts, pts_length, first_sector,
                 last_sector):
        self.dvdaudio = dvdaudio
        self.titleset = titleset
        self.title = title
        self.track = track
        self.first_pts = first_pts
        self.pts_length = pts_length
        self.first_sector = first_sector
        self.last_sector = last_sector

    def __repr__(self):
        return "DVDATrack(%s)" % ", ".join(
            "%s=%s" % (attr, getattr(self, attr))
            for attr in ["titleset", "title", "track", "first_pts", "pts_length",
                         "first_sector", "last_sector"])

    def total_frames(self):
        """the track's PCM frames, its PTS length rounded up"""
        return int((decimal.Decimal(self.pts_length) / DVDAudio.PTS_PER_SECOND *
                    self.title.sample_rate).quantize(decimal.Decimal(1),
                                                     rounding=decimal.ROUND_UP))

    def sectors(self):
        """(aob_file, start_sector, end_sector) for each AOB file the track's
        data lies in, in reading order; the sectors count within the file and
        end_sector is one past the last"""
        first, last = self.first_sector, self.last_sector + 1
        for path, start, end in self.dvdaudio.titleset_aobs[self.titleset]:
            a, b = max(first, start), min(last, end)
            if a < b:
                yield (path, a - start, b - start)


def track_frames(pts_ticks, sample_rate):
    """the frames a decoder hands out for a track of pts_ticks:
    (unsigned)round(pts_ticks * sample_rate / 90000) as aob.c computes it"""
    return (2 * int(pts_ticks) * sample_rate + DVDAudio.PTS_PER_SECOND) // \
        (2 * DVDAudio.PTS_PER_SECOND)


class _Stream(object):
    """what convert._finish reads of a converter plan"""

    def __init__(self, channels, bits_per_sample, sample_rate):
        self.channels, self.bits_per_sample, self.sample_rate = \
            channels, bits_per_sample, sample_rate


def tracks_to_flac_batch(tracks, targets, compression=None):
    """DVDATrack tracks[k] -> the FLAC file targets[k].  The tracks' titles
    are decoded once each in one call (decoders.decode_dvda_batch, PCM left
    on the device), every track's window of its title is encoded from there
    (Engine.encode_device), and every image is finished as FlacAudio.from_pcm
    finishes it: the file is the one FlacAudio.from_pcm(targets[k], <reader
    over the window>, compression, total_pcm_frames=<its frames>) writes.
    A track's window starts where the tracks before it in its title end and
    holds round(pts_length * sample_rate / 90000) frames.
    -> per track a FlacAudio, or the DecodingError / EncodingError instance
    of a track that could not be read or written (no target is left for it
    and the others go on)."""
    import numpy as np
    from .convert import _finish
    from .decoders import decode_dvda_batch
    from .flac import (COMPRESSION_PRESETS, DEFAULT_COMPRESSION, FlacAudio, padding_for,
                       target_layout)
    tracks, targets = list(tracks), list(targets)
    if len(tracks) != len(targets):
        raise ValueError("tracks and targets differ in length")
    if compression is None or compression not in FlacAudio.COMPRESSION_MODES:
        compression = DEFAULT_COMPRESSION
    preset = COMPRESSION_PRESETS[compression]
    titles = []
    for t in tracks:
        if not any(t.title is x for x in titles):
            titles.append(t.title)
    results = [None] * len(tracks)
    eng = _atgpu.engine()
    batch = decode_dvda_batch(titles, on_device=True)
    free = []
    try:
        groups = {}
        for k, (track, target) in enumerate(zip(tracks, targets)):
            i = next(i for i, x in enumerate(titles) if x is track.title)
            r = batch.results[i]
            if not r.decodes:
                why = DVDA_STATUS_TEXT[r.status] if r.mlp_status is None else \
                    "MLP status %d" % r.mlp_status
                results[k] = DecodingError("title %d of titleset %d does not decode: %s" % (
                    track.title.title, track.titleset, why))
                continue
            start = sum(track_frames(t.pts_length, r.sample_rate)
                        for t in track.title.tracks[:track.title.tracks.index(track)])
            frames = track_frames(track.pts_length, r.sample_rate)
            if start + frames > r.good_frames:
                results[k] = DecodingError(
                    "track %d of title %d needs frames %d to %d of the %d that decode" % (
                        track.track, track.title.title, start, start + frames, r.good_frames))
                continue
            try:
                mask = target_layout(target, r.channels, r.channel_mask)
            except EncodingError as err:
                results[k] = err
                continue
            pad = padding_for(frames, r.sample_rate * 10)
            groups.setdefault((i, pad), []).append((k, start, frames, mask))
        for (i, pad), members in groups.items():
            r = batch.results[i]
            try:
                opts = _atgpu.make_options(padding_size=pad, **preset)
                rows = [(start, frames, None) for _, start, frames, _ in members]
                _, nb = eng.bounds(opts, rows, r.channels, r.bits_per_sample)
                d_out = eng.device_alloc(max(16, nb))
                free.append(d_out)
                encoded = eng.encode_device(opts, batch.d_pcm + 4 * r.sample_offset,
                                            _atgpu.PCM_S32, rows, r.channels, r.bits_per_sample,
                                            r.sample_rate, d_out, nb)
                out = eng.copy_to_host(np.empty(max(1, nb), dtype=np.uint8), d_out)
            except _atgpu.ATGError as err:
                for k, _, _, _ in members:
                    results[k] = EncodingError(str(err))
                continue
            plan = _Stream(r.channels, r.bits_per_sample, r.sample_rate)
            for (k, _, frames, mask), res in zip(members, encoded):
                results[k] = _finish(targets[k], out[res.out_offset:res.out_offset + res.bytes]
                                     .tobytes(), res.status, plan, mask, frames,
                                     preset["block_size"])
        return results
    finally:
        for d in free:
            eng.device_free(d)
        batch.close()


DVDA_STATUS_TEXT = {
    _atgpu.DVDA_OK: "decoded",
    _atgpu.DVDA_BAD_SECTOR: "bad sector",
    _atgpu.DVDA_EOF: "no sectors",
    _atgpu.DVDA_UNKNOWN_CODEC: "unknown codec ID",
    _atgpu.DVDA_MLP: "an MLP title",
    _atgpu.DVDA_UNSUPPORTED: "unsupported PCM stream attributes",
}
