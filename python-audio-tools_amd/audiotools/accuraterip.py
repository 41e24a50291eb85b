"""audiotools.accuraterip — AccurateRip disc ids, response parsing and batch
verification on the MI355X.

`DiscID` is the reference's (audiotools/accuraterip.py:21-67).
`parse_response` is the parsing loop of its perform_lookup (:101-116) over
bytes the caller already holds; this module does no network access.
`match` compares a checksum with a track's entries as trackverify does
(trackverify:177-184).

`checksum_batch` runs accuraterip.hip over a batch of tracks: v1 and v2 per
track and, for max_offset = K, v1 at every drive read offset in [-K, K].
`verify_flac_batch` decodes whole albums of .flac images in one GPU batch,
leaves the PCM on the device and checksums it there.  No CPU path.
"""

import collections
import struct

import numpy as np

from . import _atgpu

AR_NOT_FOUND = -1
AR_MISMATCH = -2


class DiscID(object):
    def __init__(self, track_numbers, track_offsets, lead_out_offset, freedb_disc_id):
        """track_numbers is a list of track numbers, starting from 1;
        track_offsets their offsets in CD frames, typically starting from
        0; lead_out_offset the lead-out's, in CD frames; freedb_disc_id a
        value int() accepts"""
        assert len(track_numbers) == len(track_offsets)
        self.__track_numbers__ = track_numbers
        self.__track_offsets__ = track_offsets
        self.__lead_out_offset__ = lead_out_offset
        self.__freedb_disc_id__ = freedb_disc_id

    def track_numbers(self):
        return self.__track_numbers__[:]

    def id1(self):
        return sum(self.__track_offsets__) + self.__lead_out_offset__

    def id2(self):
        return (sum(n * max(o, 1) for (n, o) in
                    zip(self.__track_numbers__, self.__track_offsets__)) +
                (max(self.__track_numbers__) + 1) * self.__lead_out_offset__)

    def freedb_disc_id(self):
        return int(self.__freedb_disc_id__)

    def __str__(self):
        return "dBAR-%(tracks)3.3d-%(id1)8.8x-%(id2)8.8x-%(freedb)8.8x.bin" % \
            {"tracks": len(self.__track_numbers__),
             "id1": self.id1(),
             "id2": self.id2(),
             "freedb": int(self.__freedb_disc_id__)}

    def __repr__(self):
        return "AccurateRipDiscID(%s, %s, %s, %s)" % \
            (repr(self.__track_numbers__),
             repr(self.__track_offsets__),
             repr(self.__lead_out_offset__),
             repr(self.__freedb_disc_id__))


def parse_response(data, disc_id):
    """the body of an AccurateRip response -> {track_number: [(confidence,
    crc, crc2), ...]} for disc_id's tracks (numbered from 1), empty lists
    where nothing matched.

    Chunks are a 13-byte little-endian header (track count, id1, id2,
    freedb id) followed by 9 bytes per track.  As in the reference, a chunk
    whose ids differ from disc_id's has its entries left unread, so the next
    13 bytes -- the start of those entries -- are taken as a header; so is
    the entry of a track number disc_id does not list.  Parsing stops where
    the data runs out; an entry cut short is dropped."""
    data = bytes(data)
    matches = dict((n, []) for n in disc_id.track_numbers())
    pos = 0
    while pos + 13 <= len(data):
        track_count, id1, id2, freedb = struct.unpack_from("<BIII", data, pos)
        pos += 13
        if (id1 == disc_id.id1() and id2 == disc_id.id2() and
                freedb == disc_id.freedb_disc_id()):
            for track_number in range(1, track_count + 1):
                if track_number in matches:
                    if pos + 9 > len(data):
                        return matches
                    matches[track_number].append(struct.unpack_from("<BII", data, pos))
                    pos += 9
    return matches


def match(checksum, ar_matches):
    """the confidence of the first entry whose crc equals checksum,
    AR_MISMATCH when entries exist and none does, AR_NOT_FOUND without
    entries"""
    if len(ar_matches) > 0:
        for (confidence, ar_checksum, _crc2) in ar_matches:
            if checksum == ar_checksum:
                return confidence
        return AR_MISMATCH
    return AR_NOT_FOUND


track = _atgpu.ar_track


def checksum_batch(pcm, tracks, max_offset=0, device_pcm=False):
    """AccurateRip checksums of a batch of tracks in one buffer.

    pcm: interleaved stereo 16-bit PCM as a numpy int16 or int32 array in
    host memory; with device_pcm, a (device pointer, _atgpu.PCM_S16 /
    PCM_S32) pair.  tracks: a list of `track(pcm_offset, pcm_frames,
    sample_rate, is_first, is_last, lo_frame, hi_frame)` (_atgpu.ArTrack).
    The range rule takes each track's own length, also on a disc image,
    where lo_frame / hi_frame name the whole image.
    -> ([(v1, v2)], uint32 array [track][k + max_offset]: v1 at offset k)"""
    if device_pcm:
        d_pcm, fmt = pcm
        res, table = _atgpu.accuraterip_device(d_pcm, fmt, tracks, max_offset)
    else:
        a = np.asarray(pcm)
        fmt = _atgpu.PCM_S16 if a.dtype == np.int16 else _atgpu.PCM_S32
        res, table = _atgpu.accuraterip_host(a, fmt, tracks, max_offset)
    return [(r.v1, r.v2) for r in res], table


# one track of verify_flac_batch: status the decoder's ATG_FD_* code (0 =
# decoded, MD5 verified; None when the image was not decoded), v1 / v2 None
# unless checksummed, offsets {k: v1} when max_offset > 0, match the
# confidence / AR_MISMATCH / AR_NOT_FOUND when ar_matches was given, error a
# message or None
TrackResult = collections.namedtuple("TrackResult",
                                     "status v1 v2 offsets match error")


def verify_flac_batch(albums, ar_matches=None, max_offset=0):
    """decode and checksum albums of .flac images on the GPU.

    albums: a list of albums, each a list of .flac images (bytes) in track
    order; the first image of an album is its first track, the last its
    last.  ar_matches: per album a {track_number: [(confidence, crc,
    crc2)]} dict as parse_response gives (numbers from 1), or None.

    The images are decoded in one batch per device (albums sharded over
    _atgpu.batch_devices, balanced by PCM frames); the PCM stays in device
    memory, the STREAMINFO MD5 is checked by the decoder, and the checksum
    pass reads the decoder's PCM in place.  A track that is not CD audio
    (44100 Hz, 2 channels, 16 bits) or whose decode status is not 0 gets an
    error and no checksum; images with another channel count are not
    decoded at all (status None).  A malformed header raises as
    decode_flac_batch does.
    -> per album a list of TrackResult"""
    infos = []
    for album in albums:
        row = []
        for img in album:
            rc, si, _ = _atgpu.read_metadata(img)
            if rc:
                raise ValueError("not a FLAC file") if rc == 1 else \
                    IOError("EOF while reading metadata")
            row.append(si)
        infos.append(row)
    devs = _atgpu.batch_devices()
    weights = [sum(si.total_samples for si in row) for row in infos]
    ranges = (_atgpu.shard_ranges(weights, len(devs)) if len(devs) > 1
              else [(0, len(albums))])
    ranges = ranges or [(0, 0)]

    def shard(k):
        a0, a1 = ranges[k]
        single = len(ranges) == 1
        eng = _atgpu.engine() if single else _atgpu.shard_object("engine", k, devs[k])
        dec = _atgpu.decoder() if single else _atgpu.shard_object("decoder", k, devs[k])
        parts, dtracks, where, pos = [], [], [], 0
        for a in range(a0, a1):
            for t, (img, si) in enumerate(zip(albums[a], infos[a])):
                if si.channels != 2:
                    continue
                body = bytes(img[si.frames_offset:])
                body += b"\0" * ((-len(body)) % 4)
                dtracks.append(_atgpu.dec_track(pos, len(img) - si.frames_offset, si))
                where.append((a, t))
                parts.append(body)
                pos += len(body)
        out = {}
        if not dtracks:
            return out
        blob = np.frombuffer(b"".join(parts) + b"\0" * 64, dtype=np.uint8)
        d_blob = eng.device_alloc(len(blob))
        try:
            eng.copy_to_device(d_blob, blob)
            dres, d_pcm, _ = dec.decode_device(d_blob, pos, dtracks)
            ok, artracks = [], []
            for (a, t), r in zip(where, dres):
                si = infos[a][t]
                cd = si.sample_rate == 44100 and si.bits_per_sample == 16
                if r.status == 0 and cd and r.pcm_frames:
                    ok.append((a, t, r.status))
                    artracks.append(_atgpu.ar_track(
                        r.pcm_offset, r.pcm_frames, si.sample_rate, t == 0,
                        t == len(albums[a]) - 1))
                else:
                    out[(a, t)] = (r.status, None, None, None)
            if artracks:
                res, table = _atgpu.accuraterip_device(d_pcm, _atgpu.PCM_S32, artracks,
                                                       max_offset)
                for (a, t, status), r, row in zip(ok, res, table):
                    out[(a, t)] = (status, r.v1, r.v2, row)
        finally:
            eng.device_free(d_blob)
        return out

    done = {}
    for part in _atgpu.run_shards(shard, len(ranges)):
        done.update(part)
    results = []
    for a, album in enumerate(albums):
        row = []
        for t in range(len(album)):
            si = infos[a][t]
            status, v1, v2, table = done.get((a, t), (None, None, None, None))
            error = None
            if (si.channels, si.sample_rate, si.bits_per_sample) != (2, 44100, 16):
                error = "not CD audio: %d Hz, %d channels, %d bits per sample" % (
                    si.sample_rate, si.channels, si.bits_per_sample)
            elif status != 0:
                error = "decode status %s" % status
            elif v1 is None:
                error = "empty track"
            offsets = m = None
            if v1 is not None:
                if max_offset > 0:
                    offsets = dict((k, int(table[k + max_offset]))
                                   for k in range(-max_offset, max_offset + 1))
                if ar_matches is not None:
                    entries = (ar_matches[a] or {}).get(t + 1, [])
                    m = match(v1, entries)
            row.append(TrackResult(status, v1, v2, offsets, m, error))
        results.append(row)
    return results
