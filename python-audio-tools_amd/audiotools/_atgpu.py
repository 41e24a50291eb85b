"""ctypes binding of libatgpu.so — the C ABI declared in include/atgpu.h.

The library holds the HIP kernels (gfx950) and the batch engine.  This
module only marshals arguments; it never encodes anything itself.  Missing
library => ImportError, missing GPU => ATGError(ATG_ERR_DEVICE): there is no
CPU fallback on the product path.
"""

import atexit
import ctypes
import itertools
import os
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ATGPU_LIB", os.path.join(_HERE, "libatgpu.so"))

ATG_OK = 0
ATG_ERR_INVALID = -1
ATG_ERR_UNSUPPORTED = -2
ATG_ERR_DEVICE = -3
ATG_ERR_NOMEM = -4
ATG_ERR_CAPACITY = -5

PCM_S16 = 0
PCM_S32 = 1

CONV_BPS, CONV_DOWNMIX, CONV_AVERAGE = 0, 1, 2

c_u32, c_i32, c_u64 = ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64


class FlacOptions(ctypes.Structure):
    _fields_ = [("block_size", c_u32), ("max_lpc_order", c_u32),
                ("min_residual_partition_order", c_u32),
                ("max_residual_partition_order", c_u32),
                ("mid_side", c_i32), ("adaptive_mid_side", c_i32),
                ("exhaustive_model_search", c_i32),
                ("disable_verbatim_subframes", c_i32),
                ("disable_constant_subframes", c_i32),
                ("disable_fixed_subframes", c_i32),
                ("disable_lpc_subframes", c_i32), ("padding_size", c_u32)]


class Track(ctypes.Structure):
    _fields_ = [("pcm_offset", c_u64), ("pcm_frames", c_u64),
                ("frame_sizes", ctypes.POINTER(c_u32)), ("n_frame_sizes", c_u64)]


class TrackResult(ctypes.Structure):
    _fields_ = [("out_offset", c_u64), ("bytes", c_u64),
                ("first_frame", c_u32), ("n_frames", c_u32),
                ("min_frame_bytes", c_u32), ("max_frame_bytes", c_u32),
                ("md5", ctypes.c_uint8 * 16), ("status", c_i32),
                ("reserved", c_u32)]


class StreamInfo(ctypes.Structure):
    _fields_ = [("min_block_size", c_u32), ("max_block_size", c_u32),
                ("min_frame_size", c_u32), ("max_frame_size", c_u32),
                ("sample_rate", c_u32), ("channels", c_u32),
                ("bits_per_sample", c_u32), ("channel_mask", c_u32),
                ("total_samples", c_u64), ("md5", ctypes.c_uint8 * 16),
                ("frames_offset", c_u64), ("n_seekpoints", c_u32),
                ("reserved", c_u32)]


class SeekPoint(ctypes.Structure):
    _fields_ = [("sample_number", c_u64), ("byte_offset", c_u64),
                ("samples", c_u32), ("reserved", c_u32)]


class DecTrack(ctypes.Structure):
    _fields_ = [("data_offset", c_u64), ("data_bytes", c_u64),
                ("total_samples", c_u64), ("sample_rate", c_u32),
                ("channels", c_u32), ("bits_per_sample", c_u32),
                ("max_block_size", c_u32), ("md5", ctypes.c_uint8 * 16)]


class DecResult(ctypes.Structure):
    _fields_ = [("pcm_offset", c_u64), ("pcm_frames", c_u64),
                ("first_frame", c_u32), ("n_frames", c_u32),
                ("status", c_i32), ("walk_frames", c_u32),
                ("md5", ctypes.c_uint8 * 16), ("walk_status", c_i32),
                ("reserved", c_u32), ("walk_end", c_u64)]


class OggFlacInfo(ctypes.Structure):
    _fields_ = [("si", StreamInfo), ("header_packets", c_u32), ("serial_number", c_u32),
                ("has_channel_mask", c_u32), ("reserved", c_u32)]


class OggFlacDecTrack(ctypes.Structure):
    _fields_ = [("data_offset", c_u64), ("data_bytes", c_u64)]


class OggFlacDecResult(ctypes.Structure):
    _fields_ = [("pcm_offset", c_u64), ("pcm_frames", c_u64), ("n_frames", c_u32),
                ("status", c_i32), ("ogg_status", c_i32), ("header_packets", c_u32),
                ("md5", ctypes.c_uint8 * 16), ("pages", c_u32), ("packets", c_u32),
                ("fail_page", c_u32), ("reserved", c_u32), ("fail_offset", c_u64),
                ("sample_rate", c_u32), ("channels", c_u32), ("bits_per_sample", c_u32),
                ("max_block_size", c_u32), ("total_samples", c_u64),
                ("streaminfo_md5", ctypes.c_uint8 * 16), ("sample_offset", c_u64)]


# Ogg FLAC container status (include/atgpu.h ATG_OGG_*) with the reference's
# messages (src/ogg.c ogg_strerror, src/decoders/oggflac.c:324-394); the
# IOError ones per ogg_exception (ogg.c:277-292)
OGG_OK, OGG_MAGIC, OGG_VERSION, OGG_CHECKSUM, OGG_PREMATURE_EOF, OGG_STREAM_FINISHED = range(6)
OGG_PACKET_BYTE, OGG_SIGNATURE, OGG_MAJOR_VERSION, OGG_MINOR_VERSION = 6, 7, 8, 9
OGG_FLAC_SIGNATURE, OGG_BLOCK_TYPE, OGG_STREAMINFO_EOF = 10, 11, 12
OGG_MESSAGES = {
    1: "invalid magic number", 2: "invalid stream version", 3: "checksum mismatch",
    4: "premature EOF reading Ogg stream", 5: "stream finished", 6: "invalid packet byte",
    7: "invalid Ogg signature", 8: "invalid major version", 9: "invalid minor version",
    10: "invalid fLaC signature", 11: "invalid block type",
    12: "EOF while reading STREAMINFO block",
}
OGG_IOERRORS = (4, 5, 12)
OGG_MAX_IMAGE_BYTES = 1 << 28
OGG_MAX_BATCH_BYTES = 1 << 32

# decode status codes (include/atgpu.h ATG_FD_*) and the reference's
# messages for them (src/decoders/flac.c FlacDecoder_strerror, read())
FD_OK, FD_FRAME_CRC, FD_EOF, FD_MD5 = 0, 14, 15, 16
FD_MESSAGES = {
    1: "Error", 2: "invalid sync code", 3: "invalid reserved bit",
    4: "invalid bits per sample", 5: "invalid sample rate",
    6: "invalid checksum in frame header",
    7: "frame sample rate does not match STREAMINFO sample rate",
    8: "frame channel count does not match STREAMINFO channel count",
    9: "frame bits-per-sample does not match STREAMINFO bits per sample",
    10: "frame block size exceeds STREAMINFO's maximum block size",
    11: "invalid residual partition coding method",
    12: "invalid FIXED subframe order", 13: "invalid subframe type",
    14: "invalid checksum in frame", 15: "EOF reading frame",
    16: "MD5 mismatch at end of stream",
}


OGG_PAGE_PER_PACKET = 1  # ATG_OGG_PAGE_PER_PACKET


class OggFlacEncOptions(ctypes.Structure):
    _fields_ = [("serial_number", c_u32), ("page_segments", c_u32), ("flags", c_u32),
                ("channel_mask", c_u32)]


class OggFlacTrackResult(ctypes.Structure):
    _fields_ = [("out_offset", c_u64), ("bytes", c_u64),
                ("first_frame", c_u32), ("n_frames", c_u32),
                ("min_frame_bytes", c_u32), ("max_frame_bytes", c_u32),
                ("md5", ctypes.c_uint8 * 16), ("status", c_i32),
                ("pages", c_u32), ("header_pages", c_u32), ("serial_number", c_u32)]


def oggflac_enc_options(serial_number=0, page_segments=255, page_per_packet=True,
                        channel_mask=0, flags=None):
    """atg_oggflac_enc_options; `flags` overrides page_per_packet"""
    if flags is None:
        flags = OGG_PAGE_PER_PACKET if page_per_packet else 0
    return OggFlacEncOptions(int(serial_number) & 0xFFFFFFFF, int(page_segments), int(flags),
                             int(channel_mask))


class RgTrack(ctypes.Structure):
    _fields_ = [("pcm_offset", c_u64), ("pcm_frames", c_u64), ("channels", c_u32),
                ("bits_per_sample", c_u32), ("sample_rate", c_u32), ("album", c_u32),
                ("chunk_frames", ctypes.POINTER(c_u32)), ("n_chunks", c_u64)]

    def set_chunks(self, chunks):
        """attach the read() chunk sizes (kept alive on the object)"""
        if chunks is None:
            self._chunks = None
            self.chunk_frames = None
            self.n_chunks = 0
        else:
            self._chunks = np.ascontiguousarray(chunks, dtype=np.uint32)
            self.chunk_frames = self._chunks.ctypes.data_as(ctypes.POINTER(c_u32))
            self.n_chunks = len(self._chunks)
        return self


class RgResult(ctypes.Structure):
    _fields_ = [("title_gain", ctypes.c_double), ("title_peak", ctypes.c_double),
                ("status", c_i32), ("reserved", c_u32)]


AR_FIRST, AR_LAST = 1, 2


class ArTrack(ctypes.Structure):
    _fields_ = [("pcm_offset", ctypes.c_int64), ("pcm_frames", c_u64),
                ("lo_frame", c_u64), ("hi_frame", c_u64), ("index0", c_u32),
                ("total_pcm_frames", c_u32), ("sample_rate", c_u32), ("flags", c_u32)]


class ArResult(ctypes.Structure):
    _fields_ = [("v1", c_u32), ("v2", c_u32), ("status", c_i32), ("reserved", c_u32)]


class AlacOptions(ctypes.Structure):
    _fields_ = [("block_size", c_u32), ("initial_history", c_u32),
                ("history_multiplier", c_u32), ("maximum_k", c_u32),
                ("minimum_interlacing_leftweight", c_u32),
                ("maximum_interlacing_leftweight", c_u32)]


class AlacTrackResult(ctypes.Structure):
    _fields_ = [("out_offset", c_u64), ("bytes", c_u64), ("pcm_frames", c_u64),
                ("first_frameset", c_u32), ("n_framesets", c_u32), ("status", c_i32),
                ("reserved", c_u32)]


class AlacInfo(ctypes.Structure):
    _fields_ = [("max_samples_per_frame", c_u32), ("bits_per_sample", c_u32),
                ("history_multiplier", c_u32), ("initial_history", c_u32),
                ("maximum_k", c_u32), ("channels", c_u32), ("sample_rate", c_u32),
                ("total_frames", c_u32), ("mdat_offset", c_u64), ("n_seekpoints", c_u32),
                ("reserved", c_u32)]


class AlacSeekPoint(ctypes.Structure):
    _fields_ = [("pcm_frames_offset", c_u64), ("file_offset", c_u64)]


class AlacDecTrack(ctypes.Structure):
    _fields_ = [("data_offset", c_u64), ("data_bytes", c_u64), ("start", c_u64),
                ("remaining", c_u64), ("max_samples_per_frame", c_u32),
                ("bits_per_sample", c_u32), ("history_multiplier", c_u32),
                ("initial_history", c_u32), ("maximum_k", c_u32), ("channels", c_u32),
                ("frameset_bytes", ctypes.POINTER(c_u32)), ("n_frameset_bytes", c_u64)]


class AlacDecResult(ctypes.Structure):
    _fields_ = [("sample_offset", c_u64), ("pcm_frames", c_u64), ("first_frameset", c_u32),
                ("n_framesets", c_u32), ("status", c_i32), ("channels", c_u32)]


class TtaTrackResult(ctypes.Structure):
    _fields_ = [("out_offset", c_u64), ("bytes", c_u64), ("pcm_frames", c_u64),
                ("first_frame", c_u32), ("n_frames", c_u32), ("status", c_i32),
                ("reserved", c_u32)]


class TtaInfo(ctypes.Structure):
    _fields_ = [("channels", c_u32), ("bits_per_sample", c_u32), ("sample_rate", c_u32),
                ("total_pcm_frames", c_u32), ("block_size", c_u32),
                ("total_tta_frames", c_u32), ("id3_bytes", c_u64), ("frames_offset", c_u64),
                ("stage", c_u32), ("reserved", c_u32)]


class TtaDecTrack(ctypes.Structure):
    _fields_ = [("data_offset", c_u64), ("data_bytes", c_u64), ("start", c_u64),
                ("remaining", c_u64), ("channels", c_u32), ("bits_per_sample", c_u32),
                ("block_size", c_u32), ("reserved", c_u32),
                ("frame_bytes", ctypes.POINTER(c_u32)), ("n_frame_bytes", c_u64)]


class TtaDecResult(ctypes.Structure):
    _fields_ = [("sample_offset", c_u64), ("pcm_frames", c_u64), ("first_frame", c_u32),
                ("n_frames", c_u32), ("status", c_i32), ("channels", c_u32)]


class WvInfo(ctypes.Structure):
    _fields_ = [("sample_rate", c_u32), ("bits_per_sample", c_u32), ("channels", c_u32),
                ("channel_mask", c_u32), ("total_pcm_frames", c_u32), ("n_sets", c_u32),
                ("n_blocks", c_u32), ("tail_blocks", c_u32), ("end_status", c_i32),
                ("has_md5", c_u32), ("md5", ctypes.c_uint8 * 16), ("end_offset", c_u64)]


class WvBlock(ctypes.Structure):
    _fields_ = [("offset", c_u64), ("size", c_u32), ("block_index", c_u32),
                ("block_samples", c_u32), ("flags", c_u32), ("crc", c_u32), ("set", c_u32),
                ("first_channel", c_u32), ("reserved", c_u32)]


class WvDecTrack(ctypes.Structure):
    _fields_ = [("data_offset", c_u64), ("data_bytes", c_u64),
                ("blocks", ctypes.POINTER(WvBlock)), ("n_blocks", c_u32),
                ("tail_blocks", c_u32), ("channels", c_u32), ("bits_per_sample", c_u32),
                ("end_status", c_i32), ("check_md5", c_u32), ("md5", ctypes.c_uint8 * 16)]


class WvDecResult(ctypes.Structure):
    _fields_ = [("sample_offset", c_u64), ("pcm_frames", c_u64), ("n_sets", c_u32),
                ("status", c_i32), ("channels", c_u32), ("reserved", c_u32)]


class WvEncOptions(ctypes.Structure):
    _fields_ = [("block_size", c_u32), ("correlation_passes", c_u32), ("false_stereo", c_u32),
                ("wasted_bits", c_u32), ("joint_stereo", c_u32)]


class WvTrackResult(ctypes.Structure):
    _fields_ = [("out_offset", c_u64), ("bytes", c_u64), ("pcm_frames", c_u64),
                ("first_block", c_u32), ("n_blocks", c_u32), ("status", c_i32),
                ("reserved", c_u32), ("md5", ctypes.c_uint8 * 16)]


class ShnOptions(ctypes.Structure):
    _fields_ = [("block_size", c_u32), ("is_big_endian", c_i32), ("signed_samples", c_i32),
                ("reserved", c_u32)]


class ShnTrackData(ctypes.Structure):
    _fields_ = [("header", ctypes.c_char_p), ("header_bytes", c_u64),
                ("footer", ctypes.c_char_p), ("footer_bytes", c_u64)]


class ShnTrackResult(ctypes.Structure):
    _fields_ = [("out_offset", c_u64), ("bytes", c_u64), ("pcm_frames", c_u64),
                ("n_blocks", c_u32), ("reserved", c_u32)]


class ShnInfo(ctypes.Structure):
    _fields_ = [("file_type", c_u32), ("channels", c_u32), ("block_length", c_u32),
                ("max_lpc", c_u32), ("mean_count", c_u32), ("bytes_to_skip", c_u32),
                ("bits_per_sample", c_u32), ("signed_samples", c_u32),
                ("sample_rate", c_u32), ("channel_mask", c_u32),
                ("total_pcm_frames", c_u64), ("first_command_bit", c_u64)]


class ShnDecTrack(ctypes.Structure):
    _fields_ = [("data_offset", c_u64), ("data_bytes", c_u64), ("first_command_bit", c_u64),
                ("file_type", c_u32), ("channels", c_u32), ("block_length", c_u32),
                ("max_lpc", c_u32), ("mean_count", c_u32), ("reserved", c_u32)]


class ShnDecResult(ctypes.Structure):
    _fields_ = [("pcm_offset", c_u64), ("pcm_frames", c_u64), ("verbatim_offset", c_u64),
                ("header_bytes", c_u32), ("footer_bytes", c_u32), ("status", c_i32),
                ("reserved", c_u32)]


class RsTrack(ctypes.Structure):
    _fields_ = [("pcm_offset", c_u64), ("pcm_frames", c_u64), ("in_rate", c_u32),
                ("out_rate", c_u32), ("reads", ctypes.POINTER(c_u32)), ("n_reads", c_u64)]


# ALAC decoder status (include/atgpu.h ATG_AD_*) -> (exception, message) as
# the reference raises them (src/decoders/alac.c alac_exception/strerror,
# ALACDecoder_read, pcmconv.c aa_int_to_FrameList)
AD_OK, AD_IO_ERROR, AD_NO_MDAT, AD_CHANNEL_MISMATCH = 0, 1, 9, 10
AD_INIT_MESSAGES = {1: "I/O Errror", 2: "invalid unused bits", 3: "invalid alac atom",
                    4: "invalid mdhd atom", 5: "mdia atom not found",
                    6: "stsd atom not found", 7: "mdhd atom not found",
                    8: "invalid seektable entries",
                    9: "Unable to locate 'mdat' atom in stream"}
AD_READ_MESSAGES = {1: "EOF during frame reading", 2: "invalid unused bits",
                    10: "channel length mismatch"}


# True Audio decoder status (include/atgpu.h ATG_TD_*) and the messages the
# reference raises (src/decoders/tta.c TTADecoder_init, TTADecoder_read)
TD_OK, TD_IO_ERROR, TD_CRC_MISMATCH, TD_INVALID_SIGNATURE, TD_UNSUPPORTED_FORMAT, \
    TD_FRAME_READ = range(6)
TD_HEADER_MESSAGES = {1: "I/O error reading header", 2: "CRC error reading header",
                      3: "invalid header signature", 4: "unsupported TTA format"}
TD_SEEKTABLE_MESSAGES = {1: "I/O error reading seektable", 2: "CRC error reading seektable",
                         4: "unsupported TTA format"}
TD_READ_MESSAGES = {1: "I/O error reading frame", 2: "CRC mismatch reading frame",
                    5: "I/O error during frame read"}


# WavPack decoder status (include/atgpu.h ATG_WVD_*) and the messages the
# reference raises (src/decoders/wavpack.c wavpack_strerror,
# WavPackDecoder_init, WavPackDecoder_read); IOError for 1 and 16
WVD_OK, WVD_IO_ERROR = 0, 1
WVD_BLOCK_DATA_IO, WVD_INCONSISTENT_BLOCK, WVD_MD5_MISMATCH = 16, 17, 18
WVD_MESSAGES = {1: "I/O error", 3: "invalid block header ID", 4: "invalid reserved bit",
                5: "excessive decorrelation passes", 6: "invalid decorrelation term",
                7: "missing decorrelation terms sub block",
                8: "missing decorrelation weights sub block",
                9: "missing decorrelation samples sub block",
                10: "missing entropy variables sub block", 11: "missing bitstream sub block",
                12: "missing extended integers sub block",
                13: "excessive decorrelation weight values",
                14: "invalid entropy variable count", 15: "block data CRC mismatch",
                16: "I/O error reading block data", 17: "inconsistent block header",
                18: "MD5 mismatch at end of stream", 19: "sample rate undefined",
                20: "channel count/mask undefined"}
WV_INITIAL, WV_FINAL = 1 << 11, 1 << 12


class PcmLayout(ctypes.Structure):
    """atg_pcm_layout: how a packed sample lies in its bytes"""
    _fields_ = [("bytes_per_sample", ctypes.c_uint8), ("big_endian", ctypes.c_uint8),
                ("is_signed", ctypes.c_uint8), ("reserved", ctypes.c_uint8)]


class PcmRun(ctypes.Structure):
    """atg_pcm_run: samples at byte_offset of the packed buffer <-> the
    samples from sample_offset of the integer buffer"""
    _fields_ = [("byte_offset", c_u64), ("samples", c_u64), ("sample_offset", c_u64)]


class PcmView(ctypes.Structure):
    """atg_pcm_view: view frame i is source frame window_offset + i, silence
    outside the source's src_frames frames"""
    _fields_ = [("d_pcm", ctypes.c_void_p), ("sample_offset", c_u64), ("src_frames", c_u64),
                ("window_offset", ctypes.c_int64), ("format", c_u32), ("reserved", c_u32)]


class PcmPair(ctypes.Structure):
    """atg_pcm_pair: `frames` frames of view a against view b"""
    _fields_ = [("a", PcmView), ("b", PcmView), ("frames", c_u64), ("channels", c_u32),
                ("reserved", c_u32)]


class PcmCmpResult(ctypes.Structure):
    _fields_ = [("first_mismatch", c_u64), ("offset", c_i32), ("offset_found", c_u32)]


PCM_NO_MISMATCH = (1 << 64) - 1

CHAIN_MAP, CHAIN_DOWNMIX, CHAIN_AVERAGE, CHAIN_DOWNMIX_AVERAGE = range(4)
CHAIN_SILENT = 0xFF


class PcmChainRow(ctypes.Structure):
    """atg_pcm_chain_row: one track of a converter-chain call"""
    _fields_ = [("src", PcmView), ("in_channels", c_u32), ("out_channels", c_u32),
                ("channel_op", c_u32), ("channel_mask", c_u32), ("map", ctypes.c_uint8 * 8),
                ("in_bps", c_u32), ("out_bps", c_u32), ("out_offset", c_u64),
                ("dither_bit0", c_u64)]


class AiffInfo(ctypes.Structure):
    _fields_ = [("channels", c_u32), ("bits_per_sample", c_u32), ("sample_rate", c_u32),
                ("channel_mask", c_u32), ("total_pcm_frames", c_u64),
                ("ssnd_data_offset", c_u64), ("ssnd_data_bytes", c_u64)]


class AuInfo(ctypes.Structure):
    _fields_ = [("channels", c_u32), ("bits_per_sample", c_u32), ("sample_rate", c_u32),
                ("channel_mask", c_u32), ("total_pcm_frames", c_u64), ("data_offset", c_u64),
                ("data_size", c_u64), ("data_bytes", c_u64)]


PCMF_TRUNCATED = 1
(AIFF_OK, AIFF_NOT_AIFF, AIFF_INVALID_AIFF, AIFF_INVALID_CHUNK_ID, AIFF_INVALID_CHUNK,
 AIFF_PREMATURE_SSND, AIFF_NO_SSND, AIFF_IOERROR) = range(8)
AIFF_ERRORS = {AIFF_NOT_AIFF: "not an AIFF file", AIFF_INVALID_AIFF: "invalid AIFF file",
               AIFF_INVALID_CHUNK_ID: "invalid AIFF chunk ID",
               AIFF_INVALID_CHUNK: "invalid AIFF chunk",
               AIFF_PREMATURE_SSND: "SSND chunk found before fmt",
               AIFF_NO_SSND: "SSND chunk not found",
               AIFF_IOERROR: "I/O error reading COMM chunk"}
AU_OK, AU_INVALID_HEADER, AU_UNSUPPORTED_FORMAT, AU_IOERROR = range(4)
AU_ERRORS = {AU_INVALID_HEADER: "invalid Sun AU header",
             AU_UNSUPPORTED_FORMAT: "unsupported Sun AU format",
             AU_IOERROR: "I/O error reading Sun AU header"}


class ATGError(RuntimeError):
    """failure reported by libatgpu (status code + message)"""

    def __init__(self, status, message):
        RuntimeError.__init__(self, "%s (atg status %d)" % (message, status))
        self.status = status
        self.message = message


# ---- the C ABI: one row per function include/atgpu.h declares ----------------
# name -> (restype, argtypes).  load_library() applies the rows; EXPORTS is
# their names; tests/test_signatures.py holds every row against the header.
c_int, c_f64, c_str = ctypes.c_int, ctypes.c_double, ctypes.c_char_p
P = ctypes.c_void_p
ptr = ctypes.POINTER
PP, P32, P64 = ptr(P), ptr(c_u32), ptr(c_u64)

# the shapes many components share
_CREATE = (c_int, (c_int, PP))
_DESTROY = (None, (P,))
_LAST_ERROR = (c_str, ())
_KERNEL_TIMES = (c_int, (P, ptr(c_str), ptr(ctypes.c_float), c_int))
_THREAD_TIMES = (c_int, _KERNEL_TIMES[1][1:])   # the handle-less components
_TILE = (c_u32, ())
_SET_U32 = (c_int, (P, c_u32))
_SET_INT = (c_int, (P, c_int))
_COPY = (c_int, (P, P, P, c_u64))
_FETCH_PCM = (c_int, (P, P, c_u64))                 # handle, dst, cap
_FETCH_FRAMES = (c_int, (P, P, c_u64, P, P, c_u64))  # + two per-frame arrays, cap


def _read_info(info, *tables):
    """..._read_info: image, len, info struct, then the tables it fills"""
    return (c_int, (c_str, c_u64, ptr(info)) + tables)


def _decode(tracks, results, *totals):
    """..._decode_host / ..._decode_device: handle, data, len, tracks, n, results, totals"""
    return (c_int, (P, P, c_u64, tracks, c_u32, results) + totals)


# handle, options, pcm, format, tracks, n, channels, bits, rate, out, cap
_FLAC_ENCODE = (P, ptr(FlacOptions), P, c_int, ptr(Track), c_u32, c_u32, c_u32, c_u32, P, c_u64)
_OGGFLAC_ENCODE = (c_int, _FLAC_ENCODE[:2] + (ptr(OggFlacEncOptions),) + _FLAC_ENCODE[2:] +
                   (ptr(OggFlacTrackResult), P, P))
_FLAC_FRAMES = (c_int, (P, ptr(FlacOptions), P, c_int, c_u64, P, c_u64, c_u32, c_u32, c_u32,
                        c_u64, P, c_u64, P64, P))
_ALAC_ENCODE = (c_int, (P, ptr(AlacOptions), P, c_int, ptr(Track), c_u32, c_u32, c_u32, P,
                        c_u64, ptr(AlacTrackResult), P))
_TTA_ENCODE = (c_int, (P, P, c_int, ptr(Track), c_u32, c_u32, c_u32, c_u32, P, c_u64,
                       ptr(TtaTrackResult), P, c_u64, P64))
_WV_ENCODE = (c_int, (P, P, c_int, ptr(Track), c_u32, c_u32, c_u32, c_u32, c_u32,
                      ptr(WvEncOptions), P, c_u64, ptr(WvTrackResult), P, c_u64, P64))
_SHN_ENCODE = (c_int, (P, P, c_int, ptr(Track), P, c_u32, c_u32, c_u32, ptr(ShnOptions), P,
                       c_u64, ptr(ShnTrackResult), P64))

SIGNATURES = {
    "atg_abi_version": (c_int, ()),
    "atg_last_error": _LAST_ERROR,
    "atg_pick_device": (c_int, ()),
    "atg_visible_devices": (c_int, ()),
    # engine, FLAC and Ogg FLAC encode
    "atg_engine_create": _CREATE,
    "atg_engine_create_ex": (c_int, (c_int, c_u32, PP)),
    "atg_engine_destroy": _DESTROY,
    "atg_engine_kernel_times": _KERNEL_TIMES,
    "atg_engine_set_host_chunk_bytes": (c_int, (P, c_u64)),
    "atg_engine_set_inflight": _SET_U32,
    "atg_engine_inflight": (c_u32, (P,)),
    "atg_flac_batch_bounds": (c_int, (ptr(FlacOptions), ptr(Track), c_u32, c_u32, c_u32,
                                      P64, P64)),
    "atg_flac_encode_host": (c_int, _FLAC_ENCODE + (ptr(TrackResult), P, P)),
    "atg_flac_encode_host_async": (c_int, _FLAC_ENCODE + (ptr(TrackResult), P, P, P64)),
    "atg_flac_encode_host_wait": (c_int, (P, c_u64)),
    "atg_flac_encode_device": (c_int, _FLAC_ENCODE + (ptr(TrackResult),)),
    "atg_flac_encode_device_async": (c_int, _FLAC_ENCODE + (P64,)),
    "atg_flac_encode_wait": (c_int, (P, c_u64, ptr(TrackResult))),
    "atg_flac_encode_frames": _FLAC_FRAMES,
    "atg_flac_encode_frames_batch": (c_int, _FLAC_ENCODE[:4] + (P,) + _FLAC_ENCODE[5:] +
                                     (P64, P64, P32)),
    "atg_flac_max_frames_bytes": (c_u64, (ptr(FlacOptions), c_u64, P, c_u64, c_u32, c_u32)),
    "atg_flac_stream_header": (c_u64, (ptr(FlacOptions), c_u32, c_u32, c_u32, c_u64, c_u32,
                                       c_u32, P, P, c_u64)),
    "atg_service_connect": (c_int, (c_int, c_int, PP)),
    "atg_service_close": _DESTROY,
    "atg_service_last_error": _LAST_ERROR,
    "atg_service_encode_frames": _FLAC_FRAMES,
    "atg_oggflac_batch_bounds": (c_int, (ptr(FlacOptions), ptr(OggFlacEncOptions), ptr(Track),
                                         c_u32, c_u32, c_u32, P64, P64)),
    "atg_oggflac_encode_device": _OGGFLAC_ENCODE,
    "atg_oggflac_encode_host": _OGGFLAC_ENCODE,
    # memory
    "atg_host_alloc": (c_int, (c_u64, PP)),
    "atg_host_free": (None, (P,)),
    "atg_host_gather": (c_int, (P, PP, P64, c_u64, c_u32)),
    "atg_device_alloc": (c_int, (P, c_u64, PP)),
    "atg_device_free": (c_int, (P, P)),
    "atg_copy_to_device": _COPY,
    "atg_copy_device": _COPY,
    "atg_copy_to_host": _COPY,
    # FLAC and Ogg FLAC decode
    "atg_flac_read_metadata": _read_info(StreamInfo, P, c_u32),
    "atg_decoder_create": _CREATE,
    "atg_decoder_destroy": _DESTROY,
    "atg_decoder_last_error": _LAST_ERROR,
    "atg_decoder_kernel_times": _KERNEL_TIMES,
    "atg_decoder_set_inflight": _SET_U32,
    "atg_decoder_set_frame_hypothesis": _SET_INT,
    "atg_decoder_frame_hypothesis_redos": (c_u64, (P,)),
    "atg_flac_decode_host": _decode(ptr(DecTrack), ptr(DecResult), P64, P64),
    "atg_flac_decode_fetch": _FETCH_FRAMES,
    "atg_flac_decode_device": _decode(ptr(DecTrack), ptr(DecResult), PP, P64),
    "atg_flac_decode_device_async": (c_int, (P, P, c_u64, ptr(DecTrack), c_u32, P64)),
    "atg_flac_decode_wait": (c_int, (P, c_u64, ptr(DecResult), PP, P64)),
    "atg_oggflac_read_info": _read_info(OggFlacInfo),
    "atg_oggflac_decode_host": _decode(ptr(OggFlacDecTrack), ptr(OggFlacDecResult), P64, P64),
    "atg_oggflac_decode_fetch": _FETCH_FRAMES,
    "atg_oggflac_decode_device": _decode(ptr(OggFlacDecTrack), ptr(OggFlacDecResult), PP, P64),
    # PCM conversion, ReplayGain
    "atg_pcm_convert_last_error": _LAST_ERROR,
    "atg_pcm_convert_out_channels": (c_u32, (c_int, c_u32)),
    "atg_pcm_convert_device": (c_int, (c_int, P, P, c_u64, c_u32, c_u32, c_u32, c_u32, P,
                                       c_u64, P)),
    "atg_pcm_convert_host": (c_int, (c_int, c_int, P, P, c_u64, c_u32, c_u32, c_u32, c_u32, P,
                                     c_u64, c_u64)),
    "atg_replaygain_last_error": _LAST_ERROR,
    "atg_replaygain_device": (c_int, (P, ptr(RgTrack), c_u32, c_u32, ptr(RgResult), P,
                                      ptr(c_f64), P)),
    "atg_replaygain_bound": (c_int, (c_u32, ptr(c_f64))),
    "atg_replaygain_rb_factor": (c_f64, ()),
    "atg_replaygain_rebinned_windows": (c_u64, ()),
    "atg_replaygain_set_warmup": (None, (c_int,)),
    "atg_replaygain_fallback_tracks": (c_u32, ()),
    "atg_replaygain_hist_gain": (c_int, (P, c_u32, ptr(c_f64), P)),
    "atg_replaygain_multiplier": (c_f64, (c_f64, c_f64)),
    "atg_pcm_apply_gain_device": (c_int, (P, P, c_u64, c_u32, c_u32, c_f64, c_u32, P, c_u64,
                                          P)),
    "atg_pcm_apply_gain_host": (c_int, (c_int, P, P, c_u64, c_u32, c_u32, c_f64, c_u32, P,
                                        c_u64, c_u64)),
    # AccurateRip
    "atg_accuraterip_last_error": _LAST_ERROR,
    "atg_accuraterip_device": (c_int, (P, c_int, ptr(ArTrack), c_u32, c_u32, ptr(ArResult),
                                       P, P)),
    "atg_accuraterip_host": (c_int, (c_int, P, c_int, c_u64, ptr(ArTrack), c_u32, c_u32,
                                     ptr(ArResult), P)),
    "atg_accuraterip_tile_frames": _TILE,
    # packed PCM bytes, AIFF and Sun AU headers
    "atg_pcm_bytes_last_error": _LAST_ERROR,
    "atg_pcm_unpack_device": (c_int, (P, c_u64, PcmLayout, ptr(PcmRun), c_u32, P, c_int,
                                      c_u64, P)),
    "atg_pcm_pack_device": (c_int, (P, c_int, c_u64, PcmLayout, ptr(PcmRun), c_u32, P, c_u64,
                                    P)),
    "atg_pcm_unpack_host": (c_int, (c_int, P, c_u64, PcmLayout, ptr(PcmRun), c_u32, P, c_int,
                                    c_u64)),
    "atg_pcm_pack_host": (c_int, (c_int, P, c_int, c_u64, PcmLayout, ptr(PcmRun), c_u32, P,
                                  c_u64)),
    "atg_pcm_bytes_tile_samples": _TILE,
    "atg_pcm_bytes_kernel_times": _THREAD_TIMES,
    "atg_aiff_read_info": _read_info(AiffInfo),
    "atg_au_read_info": _read_info(AuInfo),
    # PCM comparison, converter chain
    "atg_pcm_compare_last_error": _LAST_ERROR,
    "atg_pcm_compare_device": (c_int, (ptr(PcmPair), c_u32, ptr(PcmCmpResult), P)),
    "atg_pcm_offset_search_device": (c_int, (ptr(PcmPair), c_u32, c_u32, ptr(PcmCmpResult),
                                             P)),
    "atg_pcm_compare_tile_frames": _TILE,
    "atg_pcm_compare_kernel_times": _THREAD_TIMES,
    "atg_pcm_chain_last_error": _LAST_ERROR,
    "atg_pcm_chain_device": (c_int, (ptr(PcmChainRow), c_u32, P, c_int, c_u64, P, c_u64, P)),
    "atg_pcm_chain_host": (c_int, (c_int, ptr(PcmChainRow), c_u32, P, c_int, c_u64, P, c_u64)),
    "atg_pcm_chain_tile_samples": _TILE,
    "atg_pcm_chain_kernel_times": _THREAD_TIMES,
    # ALAC
    "atg_alac_last_error": _LAST_ERROR,
    "atg_alac_encoder_create": _CREATE,
    "atg_alac_encoder_destroy": _DESTROY,
    "atg_alac_encoder_kernel_times": _KERNEL_TIMES,
    "atg_alac_batch_bounds": (c_int, (P, ptr(AlacOptions), ptr(Track), c_u32, c_u32, c_u32,
                                      P64, P64)),
    "atg_alac_encode_device": _ALAC_ENCODE,
    "atg_alac_encode_host": _ALAC_ENCODE,
    "atg_alac_read_info": _read_info(AlacInfo, P, c_u32, P, c_u32, P32),
    "atg_alac_decoder_last_error": _LAST_ERROR,
    "atg_alac_decoder_create": _CREATE,
    "atg_alac_decoder_destroy": _DESTROY,
    "atg_alac_decoder_kernel_times": _KERNEL_TIMES,
    "atg_alac_decode_host": _decode(ptr(AlacDecTrack), ptr(AlacDecResult), P64, P64),
    "atg_alac_decode_fetch": _FETCH_FRAMES,
    "atg_alac_decode_device": _decode(ptr(AlacDecTrack), ptr(AlacDecResult), PP, P64),
    # True Audio
    "atg_tta_last_error": _LAST_ERROR,
    "atg_tta_encoder_create": _CREATE,
    "atg_tta_encoder_destroy": _DESTROY,
    "atg_tta_encoder_kernel_times": _KERNEL_TIMES,
    "atg_tta_encode_device": _TTA_ENCODE,
    "atg_tta_encode_host": _TTA_ENCODE,
    "atg_tta_read_info": _read_info(TtaInfo, P, c_u32, P32),
    "atg_tta_decoder_last_error": _LAST_ERROR,
    "atg_tta_decoder_create": _CREATE,
    "atg_tta_decoder_destroy": _DESTROY,
    "atg_tta_decoder_kernel_times": _KERNEL_TIMES,
    "atg_tta_decode_host": _decode(ptr(TtaDecTrack), ptr(TtaDecResult), P64),
    "atg_tta_decode_fetch": _FETCH_PCM,
    "atg_tta_decode_device": _decode(ptr(TtaDecTrack), ptr(TtaDecResult), PP, P64),
    # WavPack
    "atg_wv_read_info": _read_info(WvInfo, P, c_u32, P32),
    "atg_wv_decoder_last_error": _LAST_ERROR,
    "atg_wv_decoder_create": _CREATE,
    "atg_wv_decoder_destroy": _DESTROY,
    "atg_wv_decoder_kernel_times": _KERNEL_TIMES,
    "atg_wv_decode_host": _decode(P, P, P64),
    "atg_wv_decode_fetch": _FETCH_PCM,
    "atg_wv_decode_device": _decode(P, P, PP, P64),
    "atg_wv_encoder_last_error": _LAST_ERROR,
    "atg_wv_encoder_create": _CREATE,
    "atg_wv_encoder_destroy": _DESTROY,
    "atg_wv_encoder_kernel_times": _KERNEL_TIMES,
    "atg_wv_encode_device": _WV_ENCODE,
    "atg_wv_encode_host": _WV_ENCODE,
    # resampler
    "atg_resample_last_error": _LAST_ERROR,
    "atg_resample_output_frames": (c_u64, (c_u64, c_u32, c_u32, c_u32)),
    "atg_resample_device": (c_int, (ptr(RsTrack), c_u32, c_u32, c_u32, P, P, c_u64, P, P, P)),
    "atg_resample_host": (c_int, (c_int, ptr(RsTrack), c_u32, c_u32, c_u32, P, c_u64, P, c_u64,
                                  P, P)),
    "atg_resample_read_sizes": (ctypes.c_int64, (c_u64, c_u32, c_u32, c_u32, P, c_u64, P,
                                                 c_u64)),
    "atg_resample_kernel_times": _THREAD_TIMES,
    # Shorten
    "atg_shn_encoder_last_error": _LAST_ERROR,
    "atg_shn_encoder_create": _CREATE,
    "atg_shn_encoder_destroy": _DESTROY,
    "atg_shn_encoder_kernel_times": _KERNEL_TIMES,
    "atg_shn_encode_device": _SHN_ENCODE,
    "atg_shn_encode_host": _SHN_ENCODE,
    "atg_shn_read_info": _read_info(ShnInfo),
    "atg_shn_decoder_last_error": _LAST_ERROR,
    "atg_shn_decoder_create": _CREATE,
    "atg_shn_decoder_destroy": _DESTROY,
    "atg_shn_decoder_kernel_times": _KERNEL_TIMES,
    "atg_shn_decoder_set_index_walk": _SET_INT,
    "atg_shn_decode_host": _decode(ptr(ShnDecTrack), ptr(ShnDecResult), P64),
    "atg_shn_decode_fetch": _FETCH_PCM,
    "atg_shn_decode_fetch_verbatim": _FETCH_PCM,
    "atg_shn_decode_fetch_blocks": (c_int, (P, c_u32, P, c_u64, P64)),
    "atg_shn_decode_device": _decode(ptr(ShnDecTrack), ptr(ShnDecResult), PP, P64),
}

# every function include/atgpu.h declares (tests check the .so exports them)
EXPORTS = tuple(SIGNATURES)


# ---- DVD-Audio (include/atgpu_dvda.h, a header of its own that atgpu.h includes)
class AobTitle(ctypes.Structure):
    _fields_ = [("byte_offset", c_u64), ("n_sectors", c_u32), ("reserved", c_u32)]


class AobSector(ctypes.Structure):
    _fields_ = [("payload_offset", ctypes.c_uint16), ("payload_length", ctypes.c_uint16),
                ("status", ctypes.c_uint8), ("codec_id", ctypes.c_uint8),
                ("group_1_bps", ctypes.c_uint8), ("group_1_rate", ctypes.c_uint8),
                ("channel_assignment", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 7)]


class AobResult(ctypes.Structure):
    _fields_ = [("status", c_i32), ("stop_sector", c_u32), ("sample_rate", c_u32),
                ("bits_per_sample", c_u32), ("channels", c_u32), ("channel_mask", c_u32),
                ("channel_assignment", c_u32), ("reserved", c_u32), ("good_frames", c_u64),
                ("sample_offset", c_u64)]


AOB_SECTOR_BYTES = 2048
(DVDA_OK, DVDA_BAD_SECTOR, DVDA_EOF, DVDA_UNKNOWN_CODEC, DVDA_MLP,
 DVDA_UNSUPPORTED) = range(6)

# the prototypes of include/atgpu_dvda.h, applied by load_library() with the
# table above
DVDA_SIGNATURES = {
    "atg_aob_last_error": _LAST_ERROR,
    "atg_aob_scan_device": (c_int, (P, c_u64, ptr(AobTitle), c_u32, c_int, ptr(AobResult), P64,
                                    ptr(AobSector), c_u64, P)),
    "atg_aob_decode_device": (c_int, (P, c_u64, ptr(AobTitle), c_u32, P, c_int, c_u64,
                                      ptr(AobResult), P)),
    "atg_aob_decode_host": (c_int, (c_int, P, c_u64, ptr(AobTitle), c_u32, P, c_int, c_u64,
                                    ptr(AobResult))),
    "atg_aob_tile_frames": _TILE,
    "atg_aob_kernel_times": _THREAD_TIMES,
}


# ---- MLP titles (include/atgpu_mlp.h, included by atgpu.h after atgpu_dvda.h)
class MlpResult(ctypes.Structure):
    _fields_ = [("status", c_i32), ("stop_sector", c_u32), ("stop_unit", c_u32),
                ("access_units", c_u32), ("sample_rate", c_u32), ("bits_per_sample", c_u32),
                ("channels", c_u32), ("channel_mask", c_u32), ("channel_assignment", c_u32),
                ("substreams", c_u32), ("good_frames", c_u64), ("sample_offset", c_u64)]


class MlpUnit(ctypes.Structure):
    _fields_ = [("offset", c_u64), ("end_sector", c_u32), ("size", ctypes.c_uint16),
                ("data_start", ctypes.c_uint16), ("substream_end", ctypes.c_uint16 * 2),
                ("substream_flags", ctypes.c_uint8 * 2), ("flags", ctypes.c_uint8),
                ("status", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 8)]


(MLP_OK, MLP_NOT_MLP, MLP_NO_MAJOR_SYNC, MLP_BAD_SECTOR, MLP_EOF, MLP_IO_ERROR,
 MLP_INVALID_MAJOR_SYNC, MLP_INVALID_EXTRAWORD, MLP_INVALID_RESTART_HEADER,
 MLP_INVALID_DECODING_PARAMETERS, MLP_INVALID_MATRIX_PARAMETERS,
 MLP_INVALID_CHANNEL_PARAMETERS, MLP_INVALID_BLOCK_DATA, MLP_INVALID_FILTER_PARAMETERS,
 MLP_PARITY_MISMATCH, MLP_CRC8_MISMATCH, MLP_UNSUPPORTED) = range(17)
MLP_MAX_UNIT_FRAMES = 4096

# the prototypes of include/atgpu_mlp.h, applied by load_library() as well
MLP_SIGNATURES = {
    "atg_mlp_last_error": _LAST_ERROR,
    "atg_mlp_scan_device": (c_int, (P, c_u64, ptr(AobTitle), c_u32, c_int, ptr(MlpResult), P64,
                                    ptr(MlpUnit), c_u64, P)),
    "atg_mlp_decode_device": (c_int, (P, c_u64, ptr(AobTitle), c_u32, P, c_int, c_u64,
                                      ptr(MlpResult), P)),
    "atg_mlp_decode_host": (c_int, (c_int, P, c_u64, ptr(AobTitle), c_u32, P, c_int, c_u64,
                                    ptr(MlpResult))),
    "atg_mlp_kernel_times": _THREAD_TIMES,
}

# ---- tensors (include/atgpu_tensor.h, included by atgpu.h after atgpu_mlp.h)
class PcmToTensorRow(ctypes.Structure):
    """atg_pcm_to_tensor_row: one row of a PCM -> tensor call"""
    _fields_ = [("src", PcmView), ("channels", c_u32), ("bits_per_sample", c_u32),
                ("pad_frames", c_u64), ("out_offset", c_u64), ("channel_stride", c_u64)]


class PcmFromTensorRow(ctypes.Structure):
    """atg_pcm_from_tensor_row: one row of a tensor -> PCM call"""
    _fields_ = [("in_offset", c_u64), ("channel_stride", c_u64), ("frames", c_u64),
                ("channels", c_u32), ("bits_per_sample", c_u32), ("out_offset", c_u64)]


TENSOR_F16, TENSOR_F32, TENSOR_F64, TENSOR_I32 = range(4)
TENSOR_ELEM_BYTES = {TENSOR_F16: 2, TENSOR_F32: 4, TENSOR_F64: 8, TENSOR_I32: 4}

# the prototypes of include/atgpu_tensor.h, applied by load_library() as well
TENSOR_SIGNATURES = {
    "atg_pcm_tensor_last_error": _LAST_ERROR,
    "atg_pcm_to_tensor_device": (c_int, (ptr(PcmToTensorRow), c_u32, P, c_int, c_u64, P)),
    "atg_pcm_from_tensor_device": (c_int, (ptr(PcmFromTensorRow), c_u32, P, c_int, c_u64, P,
                                           c_int, c_u64, P)),
    "atg_pcm_tensor_tile_frames": _TILE,
    "atg_pcm_tensor_kernel_times": _THREAD_TIMES,
}

# ---- device-side dither (include/atgpu_dither.h, included by atgpu.h after atgpu_tensor.h)
class DitherRun(ctypes.Structure):
    """atg_dither_run: blocks of one stream to one place of the output"""
    _fields_ = [("stream", c_u64), ("first_block", c_u64), ("blocks", c_u64),
                ("byte_offset", c_u64)]


# the prototypes of include/atgpu_dither.h, applied by load_library() as well
DITHER_SIGNATURES = {
    "atg_dither_last_error": _LAST_ERROR,
    "atg_dither_fill_device": (c_int, (ptr(DitherRun), c_u32, c_u64, P, c_u64, P)),
    "atg_dither_tile_blocks": _TILE,
    "atg_dither_kernel_times": _THREAD_TIMES,
}

# ---- FLAC frame index (include/atgpu_flac_index.h, included by atgpu.h after atgpu_dither.h)
class FlacIndexRange(ctypes.Structure):
    """atg_flac_index_range: a byte range of frame data and its STREAMINFO"""
    _fields_ = [("data_offset", c_u64), ("data_bytes", c_u64), ("sample_rate", c_u32),
                ("channels", c_u32), ("bits_per_sample", c_u32), ("max_block_size", c_u32),
                ("min_block_size", c_u32), ("reserved", c_u32)]


class FlacIndexEntry(ctypes.Structure):
    """atg_flac_index_entry: one listed frame start"""
    _fields_ = [("byte_offset", c_u64), ("first_sample", c_u64), ("block_size", c_u32),
                ("range", c_u32)]


_FLAC_INDEX = (ptr(FlacIndexRange), c_u32, ptr(FlacIndexEntry), c_u64, P64)
# the prototypes of include/atgpu_flac_index.h, applied by load_library() as well
FLAC_INDEX_SIGNATURES = {
    "atg_flac_index_last_error": _LAST_ERROR,
    "atg_flac_index_device": (c_int, (P, c_u64) + _FLAC_INDEX + (P,)),
    "atg_flac_index_host": (c_int, (c_int, P, c_u64) + _FLAC_INDEX),
    "atg_flac_index_kernel_times": _THREAD_TIMES,
}

# ---- test probes (include/atgpu_probe.h, included by atgpu.h last)
PROBE_SIGNATURES = {
    # engine, options, pcm, format, tracks, n, channels, bits, sums, cap, window_n, window
    "atg_flac_lpc_probe_host": (c_int, _FLAC_ENCODE[:8] + (P, c_u64, c_u32, P)),
}

_lib = None
_lib_lock = threading.Lock()


def load_library():
    """dlopen libatgpu.so (built in-tree by __graft_entry__.build())"""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError("libatgpu.so not found at %s: build it with "
                              "`make -C python-audio-tools_amd/csrc` or "
                              "__graft_entry__.build()" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in (list(SIGNATURES.items()) + list(DVDA_SIGNATURES.items()) +
                                          list(MLP_SIGNATURES.items()) +
                                          list(TENSOR_SIGNATURES.items()) +
                                          list(DITHER_SIGNATURES.items()) +
                                          list(FLAC_INDEX_SIGNATURES.items()) +
                                          list(PROBE_SIGNATURES.items())):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
        return lib


def _check(lib, status, component=""):
    """raise ATGError unless status is ATG_OK, with the text of the engine's
    atg_last_error or of atg_<component>_last_error"""
    if status != ATG_OK:
        last = getattr(lib, "atg_%slast_error" % (component and component + "_"))
        raise ATGError(status, last().decode("utf-8", "replace"))


def _thread_times(fn, cap):
    """{stage: ms} of this thread's last call, from a component's
    atg_*_kernel_times `fn`"""
    names = (ctypes.c_char_p * cap)()
    ms = (ctypes.c_float * cap)()
    k = fn(names, ms, cap)
    return {names[i].decode(): float(ms[i]) for i in range(k)}


def make_options(block_size, max_lpc_order, min_residual_partition_order,
                 max_residual_partition_order, mid_side=0, adaptive_mid_side=0,
                 exhaustive_model_search=0, disable_verbatim_subframes=0,
                 disable_constant_subframes=0, disable_fixed_subframes=0,
                 disable_lpc_subframes=0, padding_size=4096):
    return FlacOptions(int(block_size), int(max_lpc_order),
                       int(min_residual_partition_order),
                       int(max_residual_partition_order), int(bool(mid_side)),
                       int(bool(adaptive_mid_side)),
                       int(bool(exhaustive_model_search)),
                       int(bool(disable_verbatim_subframes)),
                       int(bool(disable_constant_subframes)),
                       int(bool(disable_fixed_subframes)),
                       int(bool(disable_lpc_subframes)), int(padding_size))


def _track_array(tracks):
    """tracks: iterable of (pcm_offset, pcm_frames[, frame_sizes])"""
    tracks = list(tracks)
    arr = (Track * max(1, len(tracks)))()
    keep = []
    for i, t in enumerate(tracks):
        arr[i].pcm_offset = int(t[0])
        arr[i].pcm_frames = int(t[1])
        sizes = t[2] if len(t) > 2 else None
        if sizes is not None:
            s = np.ascontiguousarray(sizes, dtype=np.uint32)
            keep.append(s)
            arr[i].frame_sizes = s.ctypes.data_as(ctypes.POINTER(c_u32))
            arr[i].n_frame_sizes = len(s)
        else:
            arr[i].frame_sizes = None
            arr[i].n_frame_sizes = 0
    return arr, len(tracks), keep


# Every engine / decoder / encoder handle this process opened, by opening
# order.  At interpreter exit the atexit hook below closes those still open,
# newest first, while the interpreter and the HIP runtime are both intact:
# otherwise their destroy calls run from __del__ during module teardown (or
# never), interleaved with torch's and the HIP runtime's own teardown.  Round
# 5's two exit-time crashes came from that path.
_live_handles = weakref.WeakValueDictionary()
_handle_serial = itertools.count()


def _track_handle(obj):
    _live_handles[next(_handle_serial)] = obj


def close_all():
    """close every handle still open (newest first); registered with atexit"""
    for k in sorted(_live_handles.keys(), reverse=True):
        obj = _live_handles.get(k)
        if obj is not None:
            try:
                obj.close()
            except Exception:
                pass


atexit.register(close_all)


class _Handle(object):
    """what every libatgpu handle class shares: a handle on one device, made
    by the C function a subclass names in _create and given back by _destroy;
    _last_error and _kernel_times name that component's two other accessors"""

    _create = _destroy = _last_error = _kernel_times = None
    handle = None  # so close() and __del__ are safe after a failed create

    def __init__(self, device=0):
        self.lib = load_library()
        self.device = device
        h = ctypes.c_void_p()
        self._check(self._open(int(device), ctypes.byref(h)))
        self.handle = h
        _track_handle(self)

    def _open(self, device, out):
        return getattr(self.lib, self._create)(device, out)

    def _error(self, status):
        return ATGError(status, getattr(self.lib, self._last_error)().decode("utf-8", "replace"))

    def _check(self, status, need=None):
        """raise for a failed call; with `need` (the c_u64 an encode call
        fills) the error carries .needed, the output bytes the call asks for"""
        if status != ATG_OK:
            err = self._error(status)
            if need is not None:
                err.needed = need.value
            raise err

    def _encode_retry(self, call, cap, out=None, retry=True):
        """a host encode whose output size is known only once it ran:
        call(out pointer, cap, need reference) -> status runs into `out`, or
        into cap bytes made here, and, if it reports ATG_ERR_CAPACITY and
        `retry` holds, once more with the size it asked for -> out"""
        need = c_u64()
        buf, retry = out, retry and out is None
        for _ in range(2):
            if out is None:
                buf = np.empty(max(4, cap), dtype=np.uint8)
            st = call(buf.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(need))
            if st != ATG_ERR_CAPACITY or need.value <= cap or not retry:
                break
            cap = need.value
        self._check(st, need)
        return buf

    def close(self):
        if self.handle:
            getattr(self.lib, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def kernel_times(self):
        """{stage name: ms} of the last run, in stage order; {} before it"""
        names = (ctypes.c_char_p * 16)()
        ms = (ctypes.c_float * 16)()
        k = getattr(self.lib, self._kernel_times)(self.handle, names, ms, 16)
        return {names[i].decode(): float(ms[i]) for i in range(k)}


class TrackTable(object):
    """a batch's atg_track array, built once (batches repeat in pipelines)"""

    def __init__(self, tracks):
        self.arr, self.n, self._keep = _track_array(tracks)


def _tracks(tracks):
    """a TrackTable or an iterable of tracks -> what _track_array gives"""
    if isinstance(tracks, TrackTable):
        return tracks.arr, tracks.n, tracks._keep
    return _track_array(tracks)


def _host_pcm(pcm):
    """host PCM -> (contiguous array, PCM_S16 or PCM_S32)"""
    pcm = np.ascontiguousarray(pcm)
    if pcm.dtype == np.int16:
        return pcm, PCM_S16
    if pcm.dtype == np.int32:
        return pcm, PCM_S32
    raise TypeError("pcm must be int16 or int32")


class _DecoderHandle(_Handle):
    """what the decoder classes share.  A subclass names its track and result
    structs (_track, _result), its ..._decode_device function and, where the
    C side has a plain one, its ..._decode_fetch function; its host decode
    goes through _decode_pair."""

    _track = _result = None
    _decode_device = _decode_fetch = None

    def __init__(self, device=0):
        # a decode and the fetch of its PCM are two calls: held across the
        # pair, so that threads sharing the process-wide decoder do not
        # fetch each other's batch
        self._pair = threading.Lock()
        super().__init__(device)

    def _decode_pair(self, host, track_t, result_t, n_totals, data, tracks, fetch):
        """a host-memory decode (images 4-byte aligned in data): `host`, the
        ..._decode_host function, then fetch(results, *totals), the step that
        brings the batch to host memory, both under the pair lock.  totals
        are the n_totals counts the C call reports (samples[, frames])
        -> what fetch returns"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        n = len(tracks)
        arr = (track_t * max(1, n))(*tracks)
        res = (result_t * max(1, n))()
        totals = [c_u64() for _ in range(n_totals)]
        with self._pair:
            self._check(host(self.handle, buf.ctypes.data_as(ctypes.c_void_p), len(buf), arr, n,
                             res, *[ctypes.byref(t) for t in totals]))
            return fetch([res[i] for i in range(n)], *[t.value for t in totals])

    def _on_device(self, call, track_t, result_t, d_data, nbytes, tracks):
        n = len(tracks)
        arr = (track_t * max(1, n))(*tracks)
        res = (result_t * max(1, n))()
        dp = ctypes.c_void_p()
        ns = c_u64()
        self._check(call(self.handle, ctypes.c_void_p(d_data), nbytes, arr, n, res,
                         ctypes.byref(dp), ctypes.byref(ns)))
        return [res[i] for i in range(n)], dp.value, ns.value

    def decode_device(self, d_data, nbytes, tracks):
        """decode a batch already in device memory -> ([results], device
        pointer of the int32 PCM, interleaved samples).  The PCM stays in the
        decoder's buffer until its next call (fetch() copies it out): one
        thread at a time, no lock"""
        return self._on_device(getattr(self.lib, self._decode_device), self._track,
                               self._result, d_data, nbytes, tracks)

    def fetch(self, n_samples, out=None):
        """the last decode's PCM (n_samples int32) to host memory, into
        `out` if given"""
        pcm = np.empty(max(1, n_samples), dtype=np.int32) if out is None else out
        self._check(getattr(self.lib, self._decode_fetch)(
            self.handle, pcm.ctypes.data_as(ctypes.c_void_p), n_samples))
        return pcm[:n_samples]


class HostJob:
    """a queued host-memory encode (Engine.encode_async).

    The engine DMAs into the job's pcm / out / result arrays until the job is
    waited, so the arrays are held by the Engine (not only by this object)
    until then, and a job dropped unwaited -- an exception between submit and
    wait, a discarded result -- is waited by its finalizer."""

    def __init__(self, engine, ticket, keep, n, nf):
        self.engine, self.ticket, self.n, self.nf = engine, ticket, n, nf
        engine._inflight[ticket] = keep
        self._done = None

    def wait(self):
        if self._done is None:
            keep = self.engine._inflight.get(self.ticket)
            if keep is None:
                raise ATGError(ATG_ERR_INVALID, "host job already waited or its engine closed")
            try:
                _check(self.engine.lib, self.engine.lib.atg_flac_encode_host_wait(
                    self.engine.handle, self.ticket))
            finally:
                del self.engine._inflight[self.ticket]
            _pcm, out, res, offs, fpcm, _arr, _k = keep
            self._done = (out, [res[i] for i in range(self.n)], offs[:self.nf], fpcm[:self.nf])
        return self._done

    def __del__(self):
        if self._done is None:
            try:
                if self.engine.handle and self.ticket in self.engine._inflight:
                    self.wait()
            except Exception:
                pass


ENGINE_STREAMING = 1  # atg_engine_create_ex flag (include/atgpu.h)
ENGINE_MD5_GPU = 2  # MD5 always on GPU chains
ENGINE_MD5_HOST = 4  # MD5 always on host threads


class Engine(_Handle):
    """one libatgpu engine (streams + workspace) on one device; streaming=True
    for a process that encodes one track at a time (streams on first use,
    ATG_ENGINE_STREAMING); md5 = "auto" (the engine picks GPU chains or host
    threads per batch), "gpu" or "host" (ATG_ENGINE_MD5_GPU / _HOST)"""

    _destroy, _last_error = "atg_engine_destroy", "atg_last_error"
    _kernel_times = "atg_engine_kernel_times"

    def __init__(self, device=0, streaming=False, md5="auto"):
        self._inflight = {}  # host-job ticket -> the arrays the engine writes
        self._flags = ENGINE_STREAMING if streaming else 0
        self._flags |= {"auto": 0, "gpu": ENGINE_MD5_GPU, "host": ENGINE_MD5_HOST}[md5]
        super().__init__(device)

    def _open(self, device, out):
        return self.lib.atg_engine_create_ex(device, self._flags, out)

    def close(self):
        # atg_engine_destroy drains the device; the arrays of unwaited host
        # jobs are released only after it
        super().close()
        self._inflight.clear()

    def bounds(self, options, tracks, channels, bits_per_sample):
        arr, n, _keep = _track_array(tracks)
        nf, nb = c_u64(), c_u64()
        _check(self.lib, self.lib.atg_flac_batch_bounds(
            ctypes.byref(options), arr, n, channels, bits_per_sample,
            ctypes.byref(nf), ctypes.byref(nb)))
        return nf.value, nb.value

    def encode(self, options, pcm, tracks, channels, bits_per_sample,
               sample_rate, out=None):
        """encode a batch held in host memory.

        pcm: numpy int16 (bits <= 16) or int32 interleaved samples; out: an
        optional uint8 array of at least bounds() bytes (e.g. pinned_empty)
        the images are written to.  Page-locked pcm / out are moved by DMA
        without staging.
        Returns (out: uint8 array, results: list of TrackResult,
                 frame_offsets: uint64 array, frame_pcm: uint32 array)."""
        pcm, fmt = _host_pcm(pcm)
        tracks = list(tracks)
        nf, nb = self.bounds(options, tracks, channels, bits_per_sample)
        arr, n, keep = _track_array(tracks)
        if out is None:
            out = np.empty(max(1, nb), dtype=np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < nb:
            raise ValueError("out must be a contiguous uint8 array of >= %d bytes" % nb)
        res = (TrackResult * max(1, n))()
        offs = np.zeros(max(1, nf), dtype=np.uint64)
        fpcm = np.zeros(max(1, nf), dtype=np.uint32)
        _check(self.lib, self.lib.atg_flac_encode_host(
            self.handle, ctypes.byref(options), pcm.ctypes.data_as(ctypes.c_void_p),
            fmt, arr, n, channels, bits_per_sample, sample_rate,
            out.ctypes.data_as(ctypes.c_void_p), nb, res,
            offs.ctypes.data_as(ctypes.c_void_p), fpcm.ctypes.data_as(ctypes.c_void_p)))
        return out, [res[i] for i in range(n)], offs[:nf], fpcm[:nf]

    def encode_async(self, options, pcm, tracks, channels, bits_per_sample,
                     sample_rate, out=None):
        """queue a host-memory batch (atg_flac_encode_host_async); returns a
        HostJob whose wait() gives encode()'s (out, results, frame_offsets,
        frame_pcm).  The job keeps pcm, out and the result arrays alive
        until it is waited; jobs overlap in submission order."""
        pcm, fmt = _host_pcm(pcm)
        tracks = list(tracks)
        nf, nb = self.bounds(options, tracks, channels, bits_per_sample)
        arr, n, keep = _track_array(tracks)
        if out is None:
            out = np.empty(max(1, nb), dtype=np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < nb:
            raise ValueError("out must be a contiguous uint8 array of >= %d bytes" % nb)
        res = (TrackResult * max(1, n))()
        offs = np.zeros(max(1, nf), dtype=np.uint64)
        fpcm = np.zeros(max(1, nf), dtype=np.uint32)
        t = c_u64()
        _check(self.lib, self.lib.atg_flac_encode_host_async(
            self.handle, ctypes.byref(options), pcm.ctypes.data_as(ctypes.c_void_p),
            fmt, arr, n, channels, bits_per_sample, sample_rate,
            out.ctypes.data_as(ctypes.c_void_p), nb, res,
            offs.ctypes.data_as(ctypes.c_void_p), fpcm.ctypes.data_as(ctypes.c_void_p),
            ctypes.byref(t)))
        return HostJob(self, t.value, (pcm, out, res, offs, fpcm, arr, keep), n, nf)

    def encode_device(self, options, d_pcm, fmt, tracks, channels,
                      bits_per_sample, sample_rate, d_out, out_cap):
        """encode a batch whose PCM is already in device memory; the .flac
        images stay in device memory at d_out.  Returns the TrackResults.
        `tracks` may be a TrackTable (prepared once, reused across calls)."""
        arr, n, keep = _tracks(tracks)
        res = (TrackResult * max(1, n))()
        _check(self.lib, self.lib.atg_flac_encode_device(
            self.handle, ctypes.byref(options), ctypes.c_void_p(d_pcm), fmt, arr, n,
            channels, bits_per_sample, sample_rate, ctypes.c_void_p(d_out),
            out_cap, res))
        return [res[i] for i in range(n)]

    def lpc_probe(self, options, pcm, tracks, channels, bits_per_sample, window_n=0):
        """test probe (atg_flac_lpc_probe_host): the LPC analysis kernel's raw
        autocorrelation sums for a batch held in host memory.
        Returns (sums: float64 array [frames, candidates, max_lpc_order + 1],
        frames in track order; window: float64 array of window_n values, the
        table the kernel read for frames of window_n samples, or None)."""
        pcm, fmt = _host_pcm(pcm)
        tracks = list(tracks)
        nf, _nb = self.bounds(options, tracks, channels, bits_per_sample)
        arr, n, _keep = _track_array(tracks)
        ncand = 4 if channels == 2 and (options.mid_side or options.adaptive_mid_side) \
            else channels
        sums = np.zeros((nf, ncand, options.max_lpc_order + 1), dtype=np.float64)
        window = np.zeros(window_n, dtype=np.float64) if window_n else None
        _check(self.lib, self.lib.atg_flac_lpc_probe_host(
            self.handle, ctypes.byref(options), pcm.ctypes.data_as(ctypes.c_void_p), fmt,
            arr, n, channels, bits_per_sample, sums.ctypes.data_as(ctypes.c_void_p),
            sums.size, window_n,
            window.ctypes.data_as(ctypes.c_void_p) if window_n else None))
        return sums, window

    def oggflac_bounds(self, options, ogg_options, tracks, channels, bits_per_sample):
        arr, n, _keep = _track_array(tracks)
        nf, nb = c_u64(), c_u64()
        _check(self.lib, self.lib.atg_oggflac_batch_bounds(
            ctypes.byref(options), ctypes.byref(ogg_options), arr, n, channels,
            bits_per_sample, ctypes.byref(nf), ctypes.byref(nb)))
        return nf.value, nb.value

    def encode_oggflac(self, options, ogg_options, pcm, tracks, channels, bits_per_sample,
                       sample_rate):
        """encode a batch held in host memory to Ogg FLAC images
        (atg_oggflac_encode_host).  pcm as encode().
        Returns (out: uint8 array, results: list of OggFlacTrackResult,
                 frame_page_offsets: uint64 array, frame_pcm: uint32 array)."""
        pcm, fmt = _host_pcm(pcm)
        tracks = list(tracks)
        nf, nb = self.oggflac_bounds(options, ogg_options, tracks, channels, bits_per_sample)
        arr, n, keep = _track_array(tracks)
        out = np.empty(max(1, nb), dtype=np.uint8)
        res = (OggFlacTrackResult * max(1, n))()
        offs = np.zeros(max(1, nf), dtype=np.uint64)
        fpcm = np.zeros(max(1, nf), dtype=np.uint32)
        _check(self.lib, self.lib.atg_oggflac_encode_host(
            self.handle, ctypes.byref(options), ctypes.byref(ogg_options),
            pcm.ctypes.data_as(ctypes.c_void_p), fmt, arr, n, channels, bits_per_sample,
            sample_rate, out.ctypes.data_as(ctypes.c_void_p), nb, res,
            offs.ctypes.data_as(ctypes.c_void_p), fpcm.ctypes.data_as(ctypes.c_void_p)))
        return out, [res[i] for i in range(n)], offs[:nf], fpcm[:nf]

    def encode_oggflac_device(self, options, ogg_options, d_pcm, fmt, tracks, channels,
                              bits_per_sample, sample_rate, d_out, out_cap, n_frames=0):
        """as encode_device, to Ogg FLAC images (atg_oggflac_encode_device).
        Returns (results, frame_page_offsets, frame_pcm); the two arrays are
        filled when n_frames (oggflac_bounds' frame count) is given."""
        arr, n, keep = _tracks(tracks)
        res = (OggFlacTrackResult * max(1, n))()
        offs = np.zeros(max(1, n_frames), dtype=np.uint64)
        fpcm = np.zeros(max(1, n_frames), dtype=np.uint32)
        _check(self.lib, self.lib.atg_oggflac_encode_device(
            self.handle, ctypes.byref(options), ctypes.byref(ogg_options),
            ctypes.c_void_p(d_pcm), fmt, arr, n, channels, bits_per_sample, sample_rate,
            ctypes.c_void_p(d_out), out_cap, res,
            offs.ctypes.data_as(ctypes.c_void_p) if n_frames else None,
            fpcm.ctypes.data_as(ctypes.c_void_p) if n_frames else None))
        return [res[i] for i in range(n)], offs[:n_frames], fpcm[:n_frames]

    def encode_device_async(self, options, d_pcm, fmt, tracks, channels, bits_per_sample,
                            sample_rate, d_out, out_cap):
        """enqueue a device-memory batch; -> (ticket, n_tracks) for wait()"""
        arr, n, keep = _tracks(tracks)
        t = c_u64()
        _check(self.lib, self.lib.atg_flac_encode_device_async(
            self.handle, ctypes.byref(options), ctypes.c_void_p(d_pcm), fmt, arr, n,
            channels, bits_per_sample, sample_rate, ctypes.c_void_p(d_out), out_cap,
            ctypes.byref(t)))
        return (t.value, n)

    def wait(self, ticket):
        """TrackResults of an enqueued batch (waits for it)"""
        t, n = ticket
        res = (TrackResult * max(1, n))()
        _check(self.lib, self.lib.atg_flac_encode_wait(self.handle, t, res))
        return [res[i] for i in range(n)]

    def encode_frames(self, options, pcm, channels, bits_per_sample, sample_rate,
                      first_frame_number=0, frame_sizes=None):
        """one track's PCM (host numpy int16 / int32, interleaved) as FLAC
        frames only, numbered from first_frame_number (atg_flac_encode_frames)
        -> (frame bytes: uint8 array, per-frame byte counts: uint32 array)"""
        pcm, fmt = _host_pcm(pcm)
        frames = len(pcm) // channels
        fs = None if frame_sizes is None else np.ascontiguousarray(frame_sizes, dtype=np.uint32)
        fs_p = fs.ctypes.data_as(ctypes.c_void_p) if fs is not None else None
        nfs = len(fs) if fs is not None else 0
        cap = self.lib.atg_flac_max_frames_bytes(ctypes.byref(options), frames, fs_p, nfs,
                                                 channels, bits_per_sample)
        if not cap:
            raise ATGError(ATG_ERR_INVALID, "invalid encoder options")
        n_fr = nfs if fs is not None else (frames + options.block_size - 1) // options.block_size
        out = np.empty(max(1, cap), dtype=np.uint8)
        fb = np.zeros(max(1, n_fr), dtype=np.uint32)
        nb = c_u64()
        _check(self.lib, self.lib.atg_flac_encode_frames(
            self.handle, ctypes.byref(options), pcm.ctypes.data_as(ctypes.c_void_p), fmt,
            frames, fs_p, nfs, channels, bits_per_sample, sample_rate, int(first_frame_number),
            out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(nb),
            fb.ctypes.data_as(ctypes.c_void_p)))
        return out[:nb.value], fb[:n_fr]

    def set_inflight(self, n):
        """batches encode_device_async keeps in flight (3..32; 0 = automatic,
        the default: the first batch of a pipeline picks it, include/atgpu.h)"""
        _check(self.lib, self.lib.atg_engine_set_inflight(self.handle, int(n)))

    def inflight(self):
        """the current depth D: keep up to D device batches in flight (with
        the automatic depth, read it after the pipeline's first enqueue)"""
        return int(self.lib.atg_engine_inflight(self.handle))

    def set_host_chunk_bytes(self, nbytes):
        """PCM bytes per chunk of the host-memory pipeline (encode())"""
        _check(self.lib, self.lib.atg_engine_set_host_chunk_bytes(self.handle, int(nbytes)))

    def copy_device(self, d_dst, d_src, nbytes):
        """device-to-device copy on this engine's device"""
        _check(self.lib, self.lib.atg_copy_device(self.handle, ctypes.c_void_p(d_dst),
                                                  ctypes.c_void_p(d_src), nbytes))

    def copy_to_host(self, dst, d_src):
        """device bytes at d_src -> the numpy array dst (its full size)"""
        _check(self.lib, self.lib.atg_copy_to_host(
            self.handle, dst.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_src),
            dst.nbytes))
        return dst

    def copy_to_device(self, d_dst, src):
        """the numpy array src (its full size) -> device bytes at d_dst"""
        src = np.ascontiguousarray(src)
        _check(self.lib, self.lib.atg_copy_to_device(
            self.handle, ctypes.c_void_p(d_dst), src.ctypes.data_as(ctypes.c_void_p), src.nbytes))

    def device_alloc(self, nbytes):
        """device memory on this engine's device -> pointer (device_free)"""
        p = ctypes.c_void_p()
        _check(self.lib, self.lib.atg_device_alloc(self.handle, max(4, int(nbytes)),
                                                   ctypes.byref(p)))
        return p.value

    def device_free(self, d_ptr):
        _check(self.lib, self.lib.atg_device_free(self.handle, ctypes.c_void_p(d_ptr)))


def stream_header(options, channels, bits_per_sample, sample_rate, total_samples=0,
                  min_frame_bytes=0xFFFFFF, max_frame_bytes=0, md5=b"\0" * 16):
    """fLaC + STREAMINFO + VORBIS_COMMENT + PADDING (atg_flac_stream_header)"""
    lib = load_library()
    cap = 4096 + int(options.padding_size)
    out = ctypes.create_string_buffer(cap)
    m = ctypes.create_string_buffer(bytes(md5), 16)
    n = lib.atg_flac_stream_header(ctypes.byref(options), channels, bits_per_sample,
                                   sample_rate, int(total_samples), int(min_frame_bytes),
                                   int(max_frame_bytes), m, out, cap)
    if not n:
        raise ATGError(ATG_ERR_INVALID, "invalid stream header arguments")
    return out.raw[:n]


def pinned_empty(shape, dtype=np.uint8):
    """a numpy array in page-locked host memory (atg_host_alloc), freed
    when the array is collected"""
    lib = load_library()
    dtype = np.dtype(dtype)
    count = int(np.prod(shape)) if np.ndim(shape) else int(shape)
    nbytes = max(1, count * dtype.itemsize)
    p = ctypes.c_void_p()
    _check(lib, lib.atg_host_alloc(nbytes, ctypes.byref(p)))
    buf = (ctypes.c_uint8 * nbytes).from_address(p.value)
    # not freed by weakref's own atexit hook: that hook runs before
    # close_all (it registers later), and a buffer an unwaited host job still
    # DMAs into must outlive the engine; at exit the process takes it back
    weakref.finalize(buf, lib.atg_host_free, p.value).atexit = False
    return np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)


_staging = {}
_staging_lock = threading.Lock()


def staging(key, nbytes):
    """a page-locked host buffer of at least nbytes, one per key, kept for
    the process's lifetime (grown on demand): uploads from it run at DMA
    rate without a pinning cost per call"""
    with _staging_lock:
        b = _staging.get(key)
        if b is None or b.nbytes < nbytes:
            b = pinned_empty(max(int(nbytes), 1 << 20), np.uint8)
            _staging[key] = b
        return b


_upool = None


def upload_pool():
    """a thread for host-to-device copies beside the host threads' fills"""
    global _upool
    with _staging_lock:
        if _upool is None:
            import concurrent.futures
            _upool = concurrent.futures.ThreadPoolExecutor(4)
        return _upool


def read_metadata(data, sp_cap=4096):
    """flacdec_read_metadata over an in-memory image (host C in libatgpu).
    -> (rc, StreamInfo, [(sample_number, byte_offset, samples)]);
    rc 0 ok, 1 not a FLAC stream, 2 EOF"""
    lib = load_library()
    si = StreamInfo()
    sp = (SeekPoint * max(1, sp_cap))()
    rc = lib.atg_flac_read_metadata(bytes(data), len(data), ctypes.byref(si),
                                    ctypes.cast(sp, ctypes.c_void_p), sp_cap)
    pts = [(sp[i].sample_number, sp[i].byte_offset, sp[i].samples)
           for i in range(min(si.n_seekpoints, sp_cap))]
    return rc, si, pts


def dec_track(offset, nbytes, si):
    """DecTrack for a stream whose first frame is at `offset` of the batch"""
    t = DecTrack()
    t.data_offset = offset
    t.data_bytes = nbytes
    t.total_samples = si.total_samples
    t.sample_rate = si.sample_rate
    t.channels = si.channels
    t.bits_per_sample = si.bits_per_sample
    t.max_block_size = si.max_block_size
    t.md5[:] = bytes(si.md5)
    return t


class Decoder(_DecoderHandle):
    """one libatgpu FLAC decoder (HIP stream + workspace) on one device"""

    _create, _destroy = "atg_decoder_create", "atg_decoder_destroy"
    _last_error, _kernel_times = "atg_decoder_last_error", "atg_decoder_kernel_times"
    _track, _result, _decode_device = DecTrack, DecResult, "atg_flac_decode_device"

    def __init__(self, device=0):
        super().__init__(device)
        self._pending = {}

    def set_inflight(self, n):
        """decode batches decode_device_async keeps in flight (3..16)"""
        self._check(self.lib.atg_decoder_set_inflight(self.handle, int(n)))

    def set_frame_hypothesis(self, mode):
        """the parse's frame-end hypothesis: 0 off (every subframe walked),
        1 on (default), 2 on with every batch redone (self-check)"""
        self._check(self.lib.atg_decoder_set_frame_hypothesis(self.handle, int(mode)))

    def frame_hypothesis_redos(self):
        """batches redone with the full parse after a failed check"""
        return int(self.lib.atg_decoder_frame_hypothesis_redos(self.handle))

    def decode(self, data, tracks, fetch_pcm=True):
        """decode a batch in host memory.  data: bytes-like holding every
        stream; tracks: list of DecTrack.  -> (pcm int32 array, [DecResult],
        frame byte offsets (uint64), frame block sizes (uint32)); pcm is
        None when fetch_pcm is false (results carry the PCM MD5s)"""
        def fetch(res, ns, nf):
            pcm, offs, bss = self._fetch_frames(self.lib.atg_flac_decode_fetch, ns, nf,
                                                fetch_pcm, True)
            return pcm, res, offs, bss

        return self._decode_pair(self.lib.atg_flac_decode_host, DecTrack, DecResult, 2, data,
                                 tracks, fetch)

    def _fetch_frames(self, call, ns, nf, fetch_pcm, fetch_offsets):
        """atg_flac_decode_fetch / atg_oggflac_decode_fetch: the last batch's
        ns samples (or None) and its nf frames' byte offsets (or None) and
        block sizes"""
        pcm = np.empty(max(1, ns), dtype=np.int32) if fetch_pcm else None
        offs = np.empty(max(1, nf), dtype=np.uint64) if fetch_offsets else None
        bss = np.empty(max(1, nf), dtype=np.uint32)
        self._check(call(
            self.handle, pcm.ctypes.data_as(ctypes.c_void_p) if fetch_pcm else None, ns,
            offs.ctypes.data_as(ctypes.c_void_p) if fetch_offsets else None,
            bss.ctypes.data_as(ctypes.c_void_p), nf))
        return (pcm[:ns] if fetch_pcm else None, offs[:nf] if fetch_offsets else None,
                bss[:nf])

    def decode_device_async(self, d_data, nbytes, tracks):
        """enqueue a device-resident batch (three may be in flight) -> ticket;
        d_data must stay valid until decode_wait(ticket)"""
        n = len(tracks)
        arr = (DecTrack * max(1, n))(*tracks)
        ticket = c_u64()
        self._check(self.lib.atg_flac_decode_device_async(
            self.handle, ctypes.c_void_p(d_data), nbytes, arr, n, ctypes.byref(ticket)))
        self._pending[ticket.value] = n
        return ticket.value

    def decode_wait(self, ticket):
        """-> ([DecResult], device pointer of the int32 PCM, interleaved samples)"""
        n = self._pending.pop(ticket, 0)
        res = (DecResult * max(1, n))()
        dp = ctypes.c_void_p()
        ns = c_u64()
        self._check(self.lib.atg_flac_decode_wait(self.handle, ticket, res, ctypes.byref(dp),
                                                  ctypes.byref(ns)))
        return [res[i] for i in range(n)], dp.value, ns.value

    def decode_oggflac(self, data, tracks, fetch_pcm=True):
        """decode a batch of Ogg FLAC images in host memory.  data: bytes-like
        holding every image; tracks: list of OggFlacDecTrack.  -> (pcm int32
        array, [OggFlacDecResult], frame block sizes (uint32))"""
        def fetch(res, ns, nf):
            pcm, _, bss = self._fetch_frames(self.lib.atg_oggflac_decode_fetch, ns, nf,
                                             fetch_pcm, False)
            return pcm, res, bss

        return self._decode_pair(self.lib.atg_oggflac_decode_host, OggFlacDecTrack,
                                 OggFlacDecResult, 2, data, tracks, fetch)

    def decode_oggflac_device(self, d_data, nbytes, tracks):
        """decode a batch of Ogg FLAC images already in device memory ->
        ([OggFlacDecResult], device pointer of the int32 PCM, interleaved samples)"""
        return self._on_device(self.lib.atg_oggflac_decode_device, OggFlacDecTrack,
                               OggFlacDecResult, d_data, nbytes, tracks)


def oggflac_read_info(data):
    """the first packet of an Ogg FLAC image (host C in libatgpu)
    -> (ATG_OGG_* status, OggFlacInfo)"""
    lib = load_library()
    info = OggFlacInfo()
    rc = lib.atg_oggflac_read_info(bytes(data), len(data), ctypes.byref(info))
    return rc, info


def oggflac_dec_track(offset, nbytes):
    t = OggFlacDecTrack()
    t.data_offset = offset
    t.data_bytes = nbytes
    return t


def pack_images(images):
    """whole images -> (batch buffer with every image 4-byte aligned and room
    to read the last word, [(offset, bytes)] of the images in it): what every
    decoder's host-memory batch takes"""
    parts, spans, pos = [], [], 0
    for img in images:
        img = bytes(img)
        spans.append((pos, len(img)))
        pad = (-len(img)) % 4
        parts.append(img + bytes(pad))
        pos += len(img) + pad
    return b"".join(parts), spans


def oggflac_pack(images):
    """pack_images with the images' [OggFlacDecTrack]"""
    data, spans = pack_images(images)
    return data, [oggflac_dec_track(offset, nbytes) for offset, nbytes in spans]


class AlacEncoder(_Handle):
    """one libatgpu ALAC encoder (HIP stream + workspace) on one device"""

    _create, _destroy = "atg_alac_encoder_create", "atg_alac_encoder_destroy"
    _last_error, _kernel_times = "atg_alac_last_error", "atg_alac_encoder_kernel_times"

    @staticmethod
    def options(block_size=4096, initial_history=10, history_multiplier=40, maximum_k=14,
                minimum_interlacing_leftweight=0, maximum_interlacing_leftweight=4):
        return AlacOptions(int(block_size), int(initial_history), int(history_multiplier),
                           int(maximum_k), int(minimum_interlacing_leftweight),
                           int(maximum_interlacing_leftweight))

    def bounds(self, options, tracks, channels, bits_per_sample):
        arr, n, _keep = _track_array(tracks)
        nf, nb = c_u64(), c_u64()
        self._check(self.lib.atg_alac_batch_bounds(self.handle, ctypes.byref(options), arr, n,
                                                   channels, bits_per_sample, ctypes.byref(nf),
                                                   ctypes.byref(nb)))
        return nf.value, nb.value

    def encode(self, options, pcm, tracks, channels, bits_per_sample):
        """host PCM (int16 for 16-bit, int32 otherwise) -> (out bytes array,
        [AlacTrackResult], frameset byte sizes uint32 array)"""
        pcm, fmt = _host_pcm(pcm)
        tracks = list(tracks)
        nf, nb = self.bounds(options, tracks, channels, bits_per_sample)
        arr, n, keep = _track_array(tracks)
        out = np.empty(max(1, nb), dtype=np.uint8)
        res = (AlacTrackResult * max(1, n))()
        fsb = np.zeros(max(1, nf), dtype=np.uint32)
        self._check(self.lib.atg_alac_encode_host(
            self.handle, ctypes.byref(options), pcm.ctypes.data_as(ctypes.c_void_p), fmt, arr,
            n, channels, bits_per_sample, out.ctypes.data_as(ctypes.c_void_p), nb, res,
            fsb.ctypes.data_as(ctypes.c_void_p)))
        return out, [res[i] for i in range(n)], fsb[:nf]

    def encode_device(self, options, d_pcm, fmt, tracks, channels, bits_per_sample, d_out,
                      out_cap, frameset_bytes=None):
        arr, n, keep = _tracks(tracks)
        res = (AlacTrackResult * max(1, n))()
        self._check(self.lib.atg_alac_encode_device(
            self.handle, ctypes.byref(options), ctypes.c_void_p(d_pcm), fmt, arr, n, channels,
            bits_per_sample, ctypes.c_void_p(d_out), out_cap, res,
            frameset_bytes.ctypes.data_as(ctypes.c_void_p) if frameset_bytes is not None
            else None))
        return [res[i] for i in range(n)]


def alac_read_info(data, sp_cap=65536):
    """parse_decoding_parameters + seek_mdat (host C in libatgpu)
    -> (status, AlacInfo, [(pcm_frames_offset, file_offset)], stsz sizes)"""
    lib = load_library()
    data = bytes(data)
    info = AlacInfo()
    sp = (AlacSeekPoint * max(1, sp_cap))()
    nfs = c_u32()
    lib.atg_alac_read_info(data, len(data), ctypes.byref(info), None, 0, None, 0,
                           ctypes.byref(nfs))
    sizes = np.zeros(max(1, nfs.value), dtype=np.uint32)
    st = lib.atg_alac_read_info(data, len(data), ctypes.byref(info),
                                ctypes.cast(sp, ctypes.c_void_p), sp_cap,
                                sizes.ctypes.data_as(ctypes.c_void_p), len(sizes),
                                ctypes.byref(nfs))
    pts = [(sp[i].pcm_frames_offset, sp[i].file_offset)
           for i in range(min(info.n_seekpoints, sp_cap))]
    return st, info, pts, sizes[:nfs.value]


def alac_dec_track(offset, nbytes, info, start=None, remaining=None, frameset_bytes=None):
    """AlacDecTrack for an image at `offset` of the batch buffer; keeps the
    hint array alive on the returned object"""
    t = AlacDecTrack()
    t.data_offset = offset
    t.data_bytes = nbytes
    t.start = info.mdat_offset if start is None else start
    t.remaining = info.total_frames if remaining is None else remaining
    t.max_samples_per_frame = info.max_samples_per_frame
    t.bits_per_sample = info.bits_per_sample
    t.history_multiplier = info.history_multiplier
    t.initial_history = info.initial_history
    t.maximum_k = info.maximum_k
    t.channels = info.channels
    if frameset_bytes is not None and len(frameset_bytes):
        hint = np.ascontiguousarray(frameset_bytes, dtype=np.uint32)
        t._hint = hint
        t.frameset_bytes = hint.ctypes.data_as(ctypes.POINTER(c_u32))
        t.n_frameset_bytes = len(hint)
    else:
        t._hint = None
        t.frameset_bytes = None
        t.n_frameset_bytes = 0
    return t


class AlacDecoder(_DecoderHandle):
    """one libatgpu ALAC decoder (HIP stream + workspace) on one device"""

    _create, _destroy = "atg_alac_decoder_create", "atg_alac_decoder_destroy"
    _last_error, _kernel_times = "atg_alac_decoder_last_error", "atg_alac_decoder_kernel_times"
    _track, _result, _decode_device = AlacDecTrack, AlacDecResult, "atg_alac_decode_device"

    def decode(self, data, tracks):
        """decode a batch in host memory (images 4-byte aligned in data)
        -> (pcm int32, [AlacDecResult], frameset frames, frameset offsets)"""
        def fetch(res, ns, nf):
            pcm = np.empty(max(1, ns), dtype=np.int32)
            ff = np.empty(max(1, nf), dtype=np.uint32)
            fo = np.empty(max(1, nf), dtype=np.uint64)
            self._check(self.lib.atg_alac_decode_fetch(
                self.handle, pcm.ctypes.data_as(ctypes.c_void_p), ns,
                ff.ctypes.data_as(ctypes.c_void_p), fo.ctypes.data_as(ctypes.c_void_p), nf))
            return pcm[:ns], res, ff[:nf], fo[:nf]

        return self._decode_pair(self.lib.atg_alac_decode_host, AlacDecTrack, AlacDecResult, 2,
                                 data, tracks, fetch)


class TtaEncoder(_Handle):
    """one libatgpu True Audio encoder (HIP stream + workspace) on one device"""

    _create, _destroy = "atg_tta_encoder_create", "atg_tta_encoder_destroy"
    _last_error, _kernel_times = "atg_tta_last_error", "atg_tta_encoder_kernel_times"

    @staticmethod
    def frame_count(tracks, sample_rate):
        block = (int(sample_rate) * 256) // 245
        return sum(len(t[2]) if len(t) > 2 and t[2] is not None
                   else (int(t[1]) + block - 1) // block for t in tracks)

    def encode(self, pcm, tracks, channels, bits_per_sample, sample_rate, out_cap=None):
        """host PCM (int16 up to 16 bits, int32 otherwise) -> (out bytes array,
        [TtaTrackResult], frame byte sizes uint32 array).  A TTA frame has no
        size bound, so the first call offers the raw PCM size and a call
        that reports ATG_ERR_CAPACITY is repeated with the size it asks for."""
        pcm, fmt = _host_pcm(pcm)
        tracks = list(tracks)
        arr, n, keep = _track_array(tracks)
        nf = self.frame_count(tracks, sample_rate)
        res = (TtaTrackResult * max(1, n))()
        fsb = np.zeros(max(1, nf), dtype=np.uint32)
        cap = int(out_cap) if out_cap is not None else \
            pcm.size * ((bits_per_sample + 7) // 8) + 64 * nf + 16 * n + 64
        out = self._encode_retry(lambda out, cap, need: self.lib.atg_tta_encode_host(
            self.handle, pcm.ctypes.data_as(ctypes.c_void_p), fmt, arr, n, channels,
            bits_per_sample, sample_rate, out, cap, res, fsb.ctypes.data_as(ctypes.c_void_p),
            len(fsb), need), cap)
        return out, [res[i] for i in range(n)], fsb[:nf]

    def encode_device(self, d_pcm, fmt, tracks, channels, bits_per_sample, sample_rate, d_out,
                      out_cap, frame_bytes=None):
        """-> ([TtaTrackResult], bytes needed); raises ATGError with status
        ATG_ERR_CAPACITY (and .needed) when out_cap is too small"""
        arr, n, keep = _tracks(tracks)
        res = (TtaTrackResult * max(1, n))()
        need = c_u64()
        st = self.lib.atg_tta_encode_device(
            self.handle, ctypes.c_void_p(d_pcm), fmt, arr, n, channels, bits_per_sample,
            sample_rate, ctypes.c_void_p(d_out), out_cap, res,
            frame_bytes.ctypes.data_as(ctypes.c_void_p) if frame_bytes is not None else None,
            len(frame_bytes) if frame_bytes is not None else 0, ctypes.byref(need))
        self._check(st, need)
        return [res[i] for i in range(n)], need.value


def tta_read_info(data):
    """header + seektable of a .tta image (host C in libatgpu), an ID3v2
    prefix skipped -> (ATG_TD_* status, TtaInfo, frame sizes uint32 array)"""
    lib = load_library()
    data = bytes(data)
    info = TtaInfo()
    nf = c_u32()
    lib.atg_tta_read_info(data, len(data), ctypes.byref(info), None, 0, ctypes.byref(nf))
    sizes = np.zeros(max(1, nf.value), dtype=np.uint32)
    st = lib.atg_tta_read_info(data, len(data), ctypes.byref(info),
                               sizes.ctypes.data_as(ctypes.c_void_p), len(sizes),
                               ctypes.byref(nf))
    return st, info, sizes[:nf.value]


def tta_dec_track(offset, nbytes, info, frame_bytes, first_frame=0):
    """TtaDecTrack for an image at `offset` of the batch buffer, reading from
    its frame `first_frame`; keeps the size array alive on the returned object"""
    t = TtaDecTrack()
    sizes = np.ascontiguousarray(frame_bytes, dtype=np.uint32)
    t.data_offset = offset
    t.data_bytes = nbytes
    t.start = int(info.frames_offset) + int(sizes[:first_frame].astype(np.uint64).sum())
    t.remaining = max(0, int(info.total_pcm_frames) - first_frame * int(info.block_size))
    t.channels = info.channels
    t.bits_per_sample = info.bits_per_sample
    t.block_size = info.block_size
    rest = np.ascontiguousarray(sizes[first_frame:])
    t._sizes = rest
    t.frame_bytes = rest.ctypes.data_as(ctypes.POINTER(c_u32)) if len(rest) else None
    t.n_frame_bytes = len(rest)
    return t


class TtaDecoder(_DecoderHandle):
    """one libatgpu True Audio decoder (HIP stream + workspace) on one device"""

    _create, _destroy = "atg_tta_decoder_create", "atg_tta_decoder_destroy"
    _last_error, _kernel_times = "atg_tta_decoder_last_error", "atg_tta_decoder_kernel_times"
    _track, _result = TtaDecTrack, TtaDecResult
    _decode_device, _decode_fetch = "atg_tta_decode_device", "atg_tta_decode_fetch"

    def decode(self, data, tracks):
        """decode a batch in host memory (images 4-byte aligned in data)
        -> (pcm int32, [TtaDecResult])"""
        return self._decode_pair(self.lib.atg_tta_decode_host, TtaDecTrack, TtaDecResult, 1,
                                 data, tracks, lambda res, ns: (self.fetch(ns), res))


def wv_read_info(data):
    """WavPackDecoder_init and the block table of a .wv image (host C in
    libatgpu) -> (ATG_WVD_* status, WvInfo, WvBlock array)"""
    lib = load_library()
    data = bytes(data)
    info = WvInfo()
    nb = c_u32()
    st = lib.atg_wv_read_info(data, len(data), ctypes.byref(info), None, 0, ctypes.byref(nb))
    blocks = (WvBlock * max(1, nb.value))()
    if st == 0 and nb.value:
        st = lib.atg_wv_read_info(data, len(data), ctypes.byref(info), blocks, nb.value,
                                  ctypes.byref(nb))
    return st, info, blocks


def wv_dec_track(offset, nbytes, info, blocks, first_set=0, check_md5=None):
    """WvDecTrack for an image at `offset` of the batch buffer, decoding from
    its set `first_set`; keeps the table alive on the returned object.  The
    MD5 is checked when the whole stream is decoded, unless told otherwise
    (check_md5: 0 no, 1 signed bytes at every width, 2 8-bit unsigned)."""
    t = WvDecTrack()
    skip = 0
    while skip < info.n_blocks - info.tail_blocks and blocks[skip].set < first_set:
        skip += 1
    n = info.n_blocks - skip
    rest = (WvBlock * max(1, n))(*[blocks[skip + k] for k in range(n)])
    t._blocks = rest
    t.data_offset = offset
    t.data_bytes = nbytes
    t.blocks = rest if n else None
    t.n_blocks = n
    t.tail_blocks = info.tail_blocks
    t.channels = info.channels
    t.bits_per_sample = info.bits_per_sample
    t.end_status = info.end_status
    if check_md5 is None:
        check_md5 = 1 if first_set == 0 else 0
    t.check_md5 = int(check_md5) if info.has_md5 else 0
    ctypes.memmove(t.md5, info.md5, 16)
    return t


class WvDecoder(_DecoderHandle):
    """one libatgpu WavPack decoder (HIP stream + workspace) on one device"""

    _create, _destroy = "atg_wv_decoder_create", "atg_wv_decoder_destroy"
    _last_error, _kernel_times = "atg_wv_decoder_last_error", "atg_wv_decoder_kernel_times"
    _track, _result = WvDecTrack, WvDecResult
    _decode_device, _decode_fetch = "atg_wv_decode_device", "atg_wv_decode_fetch"

    def decode(self, data, tracks, pcm_out=None):
        """decode a batch in host memory (images 4-byte aligned in data)
        -> (pcm int32, [WvDecResult]); pcm_out: an int32 array to fetch into"""
        return self._decode_pair(self.lib.atg_wv_decode_host, WvDecTrack, WvDecResult, 1, data,
                                 tracks, lambda res, ns: (self.fetch(ns, pcm_out), res))


class WvEncoder(_Handle):
    """one libatgpu WavPack encoder (HIP stream + workspace) on one device"""

    _create, _destroy = "atg_wv_encoder_create", "atg_wv_encoder_destroy"
    _last_error, _kernel_times = "atg_wv_encoder_last_error", "atg_wv_encoder_kernel_times"

    @staticmethod
    def options(block_size, correlation_passes=0, false_stereo=False, wasted_bits=False,
                joint_stereo=False):
        return WvEncOptions(int(block_size), int(correlation_passes), int(bool(false_stereo)),
                            int(bool(wasted_bits)), int(bool(joint_stereo)))

    @staticmethod
    def block_count(tracks, channels, channel_mask, block_size):
        """blocks of a batch: ceil(frames / block_size) sets of one block per
        channel group"""
        if channels <= 2:
            per = 1
        else:
            per = {0x7: 2, 0x33: 2, 0x107: 3, 0x37: 3, 0x3F: 4}.get(channel_mask, channels)
        block_size = max(1, int(block_size))
        return sum((int(t[1]) + block_size - 1) // block_size for t in tracks) * per

    def encode(self, opts, pcm, tracks, channels, channel_mask, bits_per_sample, sample_rate,
               out=None):
        """host PCM (int16 up to 16 bits, int32 otherwise) -> (out bytes array,
        [WvTrackResult], block byte sizes uint32 array): complete .wv images.
        A block has no size bound, so the first call offers the raw PCM size
        and a call that reports ATG_ERR_CAPACITY is repeated with the size
        it asks for.  With `out` (a uint8 array) given there is one call into
        it; an ATGError carries .needed."""
        pcm, fmt = _host_pcm(pcm)
        tracks = list(tracks)
        arr, n, keep = _track_array(tracks)
        nb = self.block_count(tracks, channels, channel_mask, opts.block_size)
        res = (WvTrackResult * max(1, n))()
        bsb = np.zeros(max(1, nb), dtype=np.uint32)
        cap = len(out) if out is not None else \
            pcm.size * ((bits_per_sample + 7) // 8) + 320 * nb + 128 * n + 64
        out = self._encode_retry(lambda out, cap, need: self.lib.atg_wv_encode_host(
            self.handle, pcm.ctypes.data_as(ctypes.c_void_p), fmt, arr, n, channels,
            channel_mask, bits_per_sample, sample_rate, ctypes.byref(opts), out, cap, res,
            bsb.ctypes.data_as(ctypes.c_void_p), len(bsb), need), cap, out=out)
        return out, [res[i] for i in range(n)], bsb[:nb]

    def encode_device(self, opts, d_pcm, fmt, tracks, channels, channel_mask, bits_per_sample,
                      sample_rate, d_out, out_cap, block_bytes=None):
        """-> ([WvTrackResult], bytes needed); raises ATGError with status
        ATG_ERR_CAPACITY (and .needed) when out_cap is too small"""
        arr, n, keep = _tracks(tracks)
        res = (WvTrackResult * max(1, n))()
        need = c_u64()
        st = self.lib.atg_wv_encode_device(
            self.handle, ctypes.c_void_p(d_pcm), fmt, arr, n, channels, channel_mask,
            bits_per_sample, sample_rate, ctypes.byref(opts), ctypes.c_void_p(d_out), out_cap,
            res, block_bytes.ctypes.data_as(ctypes.c_void_p) if block_bytes is not None else None,
            len(block_bytes) if block_bytes is not None else 0, ctypes.byref(need))
        self._check(st, need)
        return [res[i] for i in range(n)], need.value


_engine_lock = threading.Lock()
_shared = {}  # handle class -> the process-wide instance (engine() ... wv_encoder())


# Shorten decoder status (include/atgpu.h ATG_SHN_*) and the exceptions the
# reference raises for them (src/decoders/shn.c SHNDecoder_init, SHNDecoder_read)
(SHN_OK, SHN_END_OF_STREAM, SHN_IOERROR, SHN_UNKNOWN_COMMAND, SHN_INVALID_MAGIC_NUMBER,
 SHN_INVALID_SHORTEN_VERSION, SHN_UNSUPPORTED_FILE_TYPE, SHN_UNSUPPORTED) = range(8)
SHN_HEADER_ERRORS = {2: (IOError, "I/O error reading Shorten header"),
                     4: (ValueError, "invalid magic number"),
                     5: (ValueError, "invalid Shorten version"),
                     6: (ValueError, "unsupported Shorten file type"),
                     7: (ValueError, "unsupported Shorten stream")}
SHN_READ_ERRORS = {2: (IOError, "I/O error reading Shorten file"),
                   3: (ValueError, "unknown command in Shorten stream"),
                   7: (ValueError, "unsupported Shorten stream")}


def _shn_extra(n, headers, footers):
    """the atg_shn_track_data array of a batch (None where no track has
    header or footer bytes); the bytes objects are kept alive in the list"""
    if headers is None and footers is None:
        return None, []
    arr = (ShnTrackData * max(1, n))()
    keep = []
    for i in range(n):
        h = bytes(headers[i]) if headers is not None and headers[i] else b""
        f = bytes(footers[i]) if footers is not None and footers[i] else b""
        keep += [h, f]
        arr[i].header, arr[i].header_bytes = (h or None), len(h)
        arr[i].footer, arr[i].footer_bytes = (f or None), len(f)
    return arr, keep


class ShnEncoder(_Handle):
    """one libatgpu Shorten encoder (HIP stream + workspace) on one device"""

    _create, _destroy = "atg_shn_encoder_create", "atg_shn_encoder_destroy"
    _last_error, _kernel_times = "atg_shn_encoder_last_error", "atg_shn_encoder_kernel_times"

    def encode(self, pcm, tracks, channels, bits_per_sample, block_size=256,
               is_big_endian=False, signed_samples=True, headers=None, footers=None,
               out_cap=None):
        """host PCM (int16 or int32) -> (out bytes array, [ShnTrackResult]).
        Sizes are known only after the length pass, so the first call offers
        the raw PCM size and a call that reports ATG_ERR_CAPACITY is repeated
        with the size it asks for."""
        pcm, fmt = _host_pcm(pcm)
        arr, n, keep = _track_array(tracks)
        extra, keep2 = _shn_extra(n, headers, footers)
        opts = ShnOptions(int(block_size), int(bool(is_big_endian)), int(bool(signed_samples)), 0)
        res = (ShnTrackResult * max(1, n))()
        cap = int(out_cap) if out_cap is not None else pcm.size * 2 + 64 * n + 64
        out = self._encode_retry(lambda out, cap, need: self.lib.atg_shn_encode_host(
            self.handle, pcm.ctypes.data_as(ctypes.c_void_p), fmt, arr, extra, n, channels,
            bits_per_sample, ctypes.byref(opts), out, cap, res, need), cap,
            retry=out_cap is None)
        return out, [res[i] for i in range(n)]

    def encode_device(self, d_pcm, fmt, tracks, channels, bits_per_sample, d_out, out_cap,
                      block_size=256, is_big_endian=False, signed_samples=True, headers=None,
                      footers=None):
        """-> ([ShnTrackResult], bytes needed); raises ATGError with status
        ATG_ERR_CAPACITY (and .needed) when out_cap is too small"""
        arr, n, keep = _tracks(tracks)
        extra, keep2 = _shn_extra(n, headers, footers)
        opts = ShnOptions(int(block_size), int(bool(is_big_endian)), int(bool(signed_samples)), 0)
        res = (ShnTrackResult * max(1, n))()
        need = c_u64()
        st = self.lib.atg_shn_encode_device(
            self.handle, ctypes.c_void_p(d_pcm), fmt, arr, extra, n, channels, bits_per_sample,
            ctypes.byref(opts), ctypes.c_void_p(d_out), out_cap, res, ctypes.byref(need))
        self._check(st, need)
        return [res[i] for i in range(n)], need.value


def shn_read_info(data):
    """read_shn_header of a .shn image (host C in libatgpu)
    -> (ATG_SHN_* status, ShnInfo)"""
    lib = load_library()
    data = bytes(data)
    info = ShnInfo()
    st = lib.atg_shn_read_info(data, len(data), ctypes.byref(info))
    return st, info


def shn_dec_track(offset, nbytes, info):
    """ShnDecTrack for an image at `offset` of the batch buffer"""
    return ShnDecTrack(offset, nbytes, info.first_command_bit, info.file_type, info.channels,
                       info.block_length, info.max_lpc, info.mean_count, 0)


class ShnDecoder(_DecoderHandle):
    """one libatgpu Shorten decoder (HIP stream + workspace) on one device"""

    _create, _destroy = "atg_shn_decoder_create", "atg_shn_decoder_destroy"
    _last_error, _kernel_times = "atg_shn_decoder_last_error", "atg_shn_decoder_kernel_times"
    _track, _result = ShnDecTrack, ShnDecResult
    _decode_device, _decode_fetch = "atg_shn_decode_device", "atg_shn_decode_fetch"

    def set_index_walk(self, cooperative):
        """the index pass: the wave-cooperative code walk (default) or the
        lane-serial one"""
        self._check(self.lib.atg_shn_decoder_set_index_walk(self.handle, int(bool(cooperative))))

    def decode(self, data, tracks, blocks=False):
        """decode a batch in host memory (images 4-byte aligned in data)
        -> (pcm int32, [ShnDecResult], VERBATIM bytes); with blocks, also the
        list of every stream's fetch_blocks(), read before another thread's
        decode can replace them"""
        def fetch(res, ns):
            out = (self.fetch(ns), res, self.fetch_verbatim(res))
            if blocks:
                out += ([self.fetch_blocks(k) for k in range(len(res))],)
            return out

        return self._decode_pair(self.lib.atg_shn_decode_host, ShnDecTrack, ShnDecResult, 1,
                                 data, tracks, fetch)

    def fetch_blocks(self, track):
        """the frame counts of the sets of channels stream `track` of the
        last decode gave, in order"""
        n = c_u64()
        st = self.lib.atg_shn_decode_fetch_blocks(self.handle, track, None, 0, ctypes.byref(n))
        if st not in (ATG_OK, ATG_ERR_CAPACITY):
            self._check(st)
        out = np.zeros(max(1, n.value), dtype=np.uint32)
        self._check(self.lib.atg_shn_decode_fetch_blocks(
            self.handle, track, out.ctypes.data_as(ctypes.c_void_p), len(out), ctypes.byref(n)))
        return out[:n.value]

    def fetch_verbatim(self, results):
        """the last decode's VERBATIM bytes (header then footer per stream)"""
        nb = sum(r.header_bytes + r.footer_bytes for r in results)
        out = np.empty(max(1, nb), dtype=np.uint8)
        self._check(self.lib.atg_shn_decode_fetch_verbatim(
            self.handle, out.ctypes.data_as(ctypes.c_void_p), nb))
        return out[:nb]


def default_device():
    """ATG_DEVICE, else LOCAL_RANK, else this process's turn of a node-wide
    round robin over the visible GPUs (atg_pick_device, csrc/devices.hip):
    one process per track under track2track -j N lands on N GPUs"""
    return int(load_library().atg_pick_device())


def visible_devices():
    """GPUs this process may use (atg_visible_devices; no HIP call)"""
    return int(load_library().atg_visible_devices())


def _shared_handle(cls):
    """the process-wide instance of a handle class, made on first use"""
    with _engine_lock:
        obj = _shared.get(cls)
        if obj is None:
            obj = _shared[cls] = cls(default_device())
        return obj


def engine():
    """process-wide engine on ATG_DEVICE / LOCAL_RANK / device 0"""
    return _shared_handle(Engine)


def decoder():
    """process-wide FLAC decoder on ATG_DEVICE / LOCAL_RANK / device 0"""
    return _shared_handle(Decoder)


def alac_decoder():
    """process-wide ALAC decoder on ATG_DEVICE / LOCAL_RANK / device 0"""
    return _shared_handle(AlacDecoder)


def alac_encoder():
    """process-wide ALAC encoder on ATG_DEVICE / LOCAL_RANK / device 0"""
    return _shared_handle(AlacEncoder)


def tta_encoder():
    """process-wide True Audio encoder on ATG_DEVICE / LOCAL_RANK / device 0"""
    return _shared_handle(TtaEncoder)


def tta_decoder():
    """process-wide True Audio decoder on ATG_DEVICE / LOCAL_RANK / device 0"""
    return _shared_handle(TtaDecoder)


def shn_encoder():
    """the process-wide Shorten encoder on the default device"""
    return _shared_handle(ShnEncoder)


def shn_decoder():
    """the process-wide Shorten decoder on the default device"""
    return _shared_handle(ShnDecoder)


def wv_decoder():
    """process-wide WavPack decoder on ATG_DEVICE / LOCAL_RANK / device 0"""
    return _shared_handle(WvDecoder)


def wv_encoder():
    """process-wide WavPack encoder on ATG_DEVICE / LOCAL_RANK / device 0"""
    return _shared_handle(WvEncoder)


# ---- batches sharded over the node's GPUs ---------------------
# A batch entry point (encode_flac_batch, decode_flac_batch,
# calculate_replay_gain) splits its tracks into contiguous groups, one per
# device, balanced by PCM frames, and runs every group on its device's
# engine in a thread of its own (the C calls release the GIL); results are
# merged in track order.  No collective: the groups are independent, except
# ReplayGain's album histogram / peak, reduced by the caller (replaygain.py).
_shard_objs = {}


def batch_devices():
    """devices a batch call shards over: the one ATG_DEVICE / LOCAL_RANK
    names (a process bound to a GPU), else every visible GPU.
    ATG_SHARD_DEVICES="0,0" lists them explicitly (tests: two shards on one
    GPU take the multi-device path)"""
    v = os.environ.get("ATG_SHARD_DEVICES", "")
    if v.strip():
        return [int(x) for x in v.split(",") if x.strip()]
    for var in ("ATG_DEVICE", "LOCAL_RANK"):
        if os.environ.get(var, "").strip():
            return [int(os.environ[var])]
    return list(range(visible_devices()))


def shard_ranges(weights, n):
    """contiguous [t0, t1) ranges of len(weights) tracks over at most n
    shards, each ending where the running weight first reaches its share
    of the total; empty ranges dropped"""
    weights = [max(0, int(w)) for w in weights]
    t, n = len(weights), max(1, min(n, len(weights)))
    if t == 0:
        return []
    total = float(sum(weights)) or float(t)
    w = weights if sum(weights) else [1] * t
    out, t0, run = [], 0, 0
    for k in range(1, n + 1):
        goal = total * k / n
        t1 = t0
        while t1 < t and (run + w[t1] <= goal or t1 == t0) and (t - t1) > (n - k):
            run += w[t1]
            t1 += 1
        if k == n:
            t1 = t
        if t1 > t0:
            out.append((t0, t1))
        t0 = t1
    return out


def shard_object(kind, i, device):
    """the engine / decoder of shard i on `device` (one per shard, kept for
    the process's lifetime like engine())"""
    key = (kind, i, device)
    with _engine_lock:
        obj = _shard_objs.get(key)
        if obj is None:
            obj = {"engine": Engine, "decoder": Decoder, "alac_decoder": AlacDecoder}[kind](
                device)
            _shard_objs[key] = obj
        return obj


def run_shards(fn, n):
    """fn(i) for i in range(n) on n threads (one per device); results in
    order; the first exception is raised"""
    if n == 1:
        return [fn(0)]
    out, err = [None] * n, []

    def one(i):
        try:
            out[i] = fn(i)
        except BaseException as e:  # noqa: B902 -- re-raised below
            err.append(e)

    th = [threading.Thread(target=one, args=(i,)) for i in range(n)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    if err:
        raise err[0]
    return out


def pcm_convert(kind, pcm, channels, in_bps, out_bps=None, channel_mask=0,
                dither=b"", dither_bit0=0, device=None):
    """one GPU conversion of interleaved int32 PCM held in host memory
    (atg_pcm_convert_host) -> int32 numpy array"""
    lib = load_library()
    a = np.ascontiguousarray(pcm, dtype=np.int32)
    frames = len(a) // channels
    oc = lib.atg_pcm_convert_out_channels(kind, channels)
    out = np.empty(max(1, frames * oc), dtype=np.int32)
    d = np.frombuffer(bytes(dither), dtype=np.uint8) if dither else None
    st = lib.atg_pcm_convert_host(
        default_device() if device is None else device, kind,
        a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), frames,
        channels, channel_mask, in_bps, in_bps if out_bps is None else out_bps,
        d.ctypes.data_as(ctypes.c_void_p) if d is not None else None,
        0 if d is None else len(d), dither_bit0)
    _check(lib, st, "pcm_convert")
    return out[:frames * oc]


def replaygain_device(d_pcm, tracks, n_albums=0, d_album_hist=None):
    """ReplayGain of a batch whose int32 PCM is in device memory.
    tracks: list of RgTrack.  -> ([RgResult], [album peak])"""
    lib = load_library()
    n = len(tracks)
    arr = (RgTrack * max(1, n))(*tracks)
    res = (RgResult * max(1, n))()
    peaks = (ctypes.c_double * max(1, n_albums))()
    _check(lib, lib.atg_replaygain_device(
        ctypes.c_void_p(d_pcm), arr, n, n_albums, res,
        ctypes.c_void_p(d_album_hist) if d_album_hist else None, peaks, None), "replaygain")
    return [res[i] for i in range(n)], [peaks[i] for i in range(n_albums)]


def replaygain_hist_gain(d_hist, n):
    """analyzeResult of n device histograms -> list of gains (NaN = none)"""
    lib = load_library()
    g = (ctypes.c_double * max(1, n))()
    _check(lib, lib.atg_replaygain_hist_gain(ctypes.c_void_p(d_hist), n, g, None), "replaygain")
    return [g[i] for i in range(n)]


def replaygain_host(pcm, tracks, n_albums=0, return_hist=False, eng=None):
    """same as replaygain_device for int32 PCM in host memory, on `eng`'s
    device (the process-wide engine's by default)
    -> (results, album_peaks, album_gains[, album histograms uint32])"""
    lib = load_library()
    eng = eng or engine()
    a = np.ascontiguousarray(pcm, dtype=np.int32)
    d_pcm, d_hist = ctypes.c_void_p(), ctypes.c_void_p()
    _check(lib, lib.atg_device_alloc(eng.handle, max(4, a.nbytes), ctypes.byref(d_pcm)))
    _check(lib, lib.atg_device_alloc(eng.handle, max(4, 48000 * n_albums),
                                     ctypes.byref(d_hist)))
    try:
        if a.nbytes:
            _check(lib, lib.atg_copy_to_device(eng.handle, d_pcm,
                                               a.ctypes.data_as(ctypes.c_void_p), a.nbytes))
        res, peaks = replaygain_device(d_pcm.value, tracks, n_albums, d_hist.value)
        gains = replaygain_hist_gain(d_hist.value, n_albums) if n_albums else []
        hist = None
        if return_hist:
            hist = np.zeros((max(1, n_albums), 12000), dtype=np.uint32)
            if n_albums:
                _check(lib, lib.atg_copy_to_host(eng.handle, hist.ctypes.data_as(ctypes.c_void_p),
                                                 d_hist, hist.nbytes))
    finally:
        lib.atg_device_free(eng.handle, d_pcm)
        lib.atg_device_free(eng.handle, d_hist)
    if return_hist:
        return res, peaks, gains, hist[:n_albums]
    return res, peaks, gains


def replaygain_hist_gain_host(hists):
    """analyzeResult of host uint32[n][12000] histograms on the GPU
    -> list of gains (NaN = not enough samples)"""
    lib = load_library()
    eng = engine()
    h = np.ascontiguousarray(np.atleast_2d(hists), dtype=np.uint32)
    n = h.shape[0]
    d = ctypes.c_void_p()
    _check(lib, lib.atg_device_alloc(eng.handle, max(4, h.nbytes), ctypes.byref(d)))
    try:
        _check(lib, lib.atg_copy_to_device(eng.handle, d, h.ctypes.data_as(ctypes.c_void_p),
                                           h.nbytes))
        return replaygain_hist_gain(d.value, n)
    finally:
        lib.atg_device_free(eng.handle, d)


def ar_track(pcm_offset, pcm_frames, sample_rate=44100, is_first=False, is_last=False,
             lo_frame=None, hi_frame=None, index0=0, total_pcm_frames=None):
    """ArTrack of pcm_frames frames at frame position pcm_offset of the batch
    buffer; the readable region defaults to the track itself"""
    lo = max(0, pcm_offset) if lo_frame is None else lo_frame
    hi = max(lo, pcm_offset + pcm_frames) if hi_frame is None else hi_frame
    return ArTrack(pcm_offset, pcm_frames, lo, hi, index0,
                   pcm_frames if total_pcm_frames is None else total_pcm_frames, sample_rate,
                   (AR_FIRST if is_first else 0) | (AR_LAST if is_last else 0))


def _ar_call(call, tracks, max_offset):
    lib = load_library()
    n = len(tracks)
    arr = (ArTrack * max(1, n))(*tracks)
    res = (ArResult * max(1, n))()
    table = np.zeros((n, 2 * max_offset + 1), dtype=np.uint32)
    st = call(lib, arr, n, res, table.ctypes.data_as(ctypes.c_void_p))
    _check(lib, st, "accuraterip")
    return [res[i] for i in range(n)], table


def accuraterip_device(d_pcm, fmt, tracks, max_offset=0):
    """AccurateRip checksums of a batch whose PCM (PCM_S16 / PCM_S32) is in
    device memory (on the device that holds it).  tracks: list of ArTrack.
    -> ([ArResult], uint32 array [track][k + max_offset] of v1 at offset k)"""
    return _ar_call(lambda lib, arr, n, res, table: lib.atg_accuraterip_device(
        ctypes.c_void_p(d_pcm), fmt, arr, n, max_offset, res, table, None), tracks, max_offset)


def accuraterip_host(pcm, fmt, tracks, max_offset=0, device=None):
    """the same for interleaved stereo PCM in host memory (int16 for PCM_S16,
    int32 for PCM_S32), staged through `device`"""
    a = np.ascontiguousarray(pcm, dtype=np.int16 if fmt == PCM_S16 else np.int32)
    return _ar_call(lambda lib, arr, n, res, table: lib.atg_accuraterip_host(
        default_device() if device is None else device, a.ctypes.data_as(ctypes.c_void_p), fmt,
        len(a) // 2, arr, n, max_offset, res, table), tracks, max_offset)


def accuraterip_tile_frames():
    """PCM frames per tile of the checksum's streaming pass"""
    return int(load_library().atg_accuraterip_tile_frames())


# ------------------------------------------------- packed PCM bytes (pcm_bytes.hip)
def pcm_layout(bytes_per_sample, big_endian, is_signed):
    return PcmLayout(bytes_per_sample, 1 if big_endian else 0, 1 if is_signed else 0, 0)


def pcm_runs(runs):
    """[(byte_offset, samples, sample_offset)] -> (PcmRun array, count)"""
    runs = list(runs)
    arr = (PcmRun * max(1, len(runs)))()
    for i, (b, n, s) in enumerate(runs):
        arr[i].byte_offset, arr[i].samples, arr[i].sample_offset = b, n, s
    return arr, len(runs)


def pcm_unpack_device(d_bytes, bytes_cap, layout, runs, d_pcm, fmt, pcm_cap_samples):
    """packed bytes in device memory -> interleaved int16 (PCM_S16) or int32
    (PCM_S32) in device memory, one launch for all runs (atg_pcm_unpack_device);
    runs: [(byte_offset, samples, sample_offset)] or a pcm_runs() pair"""
    lib = load_library()
    arr, n = runs if isinstance(runs, tuple) else pcm_runs(runs)
    _check(lib, lib.atg_pcm_unpack_device(
        ctypes.c_void_p(d_bytes), bytes_cap, layout, arr, n, ctypes.c_void_p(d_pcm), fmt,
        pcm_cap_samples, None), "pcm_bytes")


def pcm_pack_device(d_pcm, fmt, pcm_cap_samples, layout, runs, d_bytes, bytes_cap):
    """the inverse (atg_pcm_pack_device): only the runs' packed bytes are written"""
    lib = load_library()
    arr, n = runs if isinstance(runs, tuple) else pcm_runs(runs)
    _check(lib, lib.atg_pcm_pack_device(
        ctypes.c_void_p(d_pcm), fmt, pcm_cap_samples, layout, arr, n, ctypes.c_void_p(d_bytes),
        bytes_cap, None), "pcm_bytes")


def pcm_unpack_host(data, layout, runs, out, device=None):
    """packed bytes in host memory (bytes or uint8 array) -> the runs' sample
    ranges of `out` (int16 or int32 numpy array), staged through `device`"""
    lib = load_library()
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    arr, n = runs if isinstance(runs, tuple) else pcm_runs(runs)
    fmt = PCM_S16 if out.dtype == np.int16 else PCM_S32
    _check(lib, lib.atg_pcm_unpack_host(
        default_device() if device is None else device, a.ctypes.data_as(ctypes.c_void_p),
        a.nbytes, layout, arr, n, out.ctypes.data_as(ctypes.c_void_p), fmt, len(out)), "pcm_bytes")
    return out


def pcm_pack_host(pcm, layout, runs, out, device=None):
    """int16 / int32 samples in host memory -> the runs' byte ranges of the
    uint8 array `out`, staged through `device`"""
    lib = load_library()
    a = np.ascontiguousarray(pcm)
    arr, n = runs if isinstance(runs, tuple) else pcm_runs(runs)
    fmt = PCM_S16 if a.dtype == np.int16 else PCM_S32
    _check(lib, lib.atg_pcm_pack_host(
        default_device() if device is None else device, a.ctypes.data_as(ctypes.c_void_p), fmt,
        len(a), layout, arr, n, out.ctypes.data_as(ctypes.c_void_p), out.nbytes), "pcm_bytes")
    return out


def pcm_bytes_tile_samples():
    """samples per tile of the pack / unpack kernels"""
    return int(load_library().atg_pcm_bytes_tile_samples())


def pcm_bytes_kernel_times():
    """{"unpack" or "pack": ms} of this thread's last launch"""
    return _thread_times(load_library().atg_pcm_bytes_kernel_times, 1)


# ------------------------------------------------- DVD-Audio AOB (aob_decode.hip)
def aob_titles(titles):
    """[(byte_offset, n_sectors)] -> (AobTitle array, count)"""
    titles = list(titles)
    arr = (AobTitle * max(1, len(titles)))()
    for i, (off, n) in enumerate(titles):
        arr[i].byte_offset, arr[i].n_sectors = off, n
    return arr, len(titles)


def aob_scan_device(d_bytes, bytes_cap, titles, fmt=PCM_S32, want_sectors=False):
    """sector and layout passes over AOB bytes in device memory
    (atg_aob_scan_device): ([AobResult], total_samples) with sample_offset
    laid out for `fmt`, and the AobSector table of all titles' sectors in
    order as a third item when want_sectors"""
    lib = load_library()
    arr, n = titles if isinstance(titles, tuple) else aob_titles(titles)
    res = (AobResult * max(1, n))()
    total = ctypes.c_uint64()
    n_sec = sum(arr[i].n_sectors for i in range(n))
    sec = (AobSector * max(1, n_sec))() if want_sectors else None
    _check(lib, lib.atg_aob_scan_device(ctypes.c_void_p(d_bytes), bytes_cap, arr, n, fmt, res,
                                        ctypes.byref(total), sec, n_sec, None), "aob")
    out = (list(res[:n]), total.value)
    return out + (list(sec[:n_sec]),) if want_sectors else out


def aob_decode_device(d_bytes, bytes_cap, titles, d_pcm, fmt, pcm_cap_samples):
    """all three passes into d_pcm (atg_aob_decode_device): [AobResult]; raises
    ATGError(ATG_ERR_CAPACITY) when pcm_cap_samples is too small"""
    lib = load_library()
    arr, n = titles if isinstance(titles, tuple) else aob_titles(titles)
    res = (AobResult * max(1, n))()
    _check(lib, lib.atg_aob_decode_device(ctypes.c_void_p(d_bytes), bytes_cap, arr, n,
                                          ctypes.c_void_p(d_pcm), fmt, pcm_cap_samples, res,
                                          None), "aob")
    return list(res[:n])


def aob_decode_host(data, titles, fmt=PCM_S32, device=None):
    """AOB bytes in host memory -> ([AobResult], int16 / int32 numpy array),
    staged through `device`.  The array is sized from the sectors' byte count,
    which bounds the samples of any layout."""
    lib = load_library()
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    arr, n = titles if isinstance(titles, tuple) else aob_titles(titles)
    res = (AobResult * max(1, n))()
    cap = sum(arr[i].n_sectors for i in range(n)) * (AOB_SECTOR_BYTES // 2) + 8 * n
    out = np.zeros(cap, dtype=np.int16 if fmt == PCM_S16 else np.int32)
    _check(lib, lib.atg_aob_decode_host(
        default_device() if device is None else device, a.ctypes.data_as(ctypes.c_void_p),
        a.nbytes, arr, n, out.ctypes.data_as(ctypes.c_void_p), fmt, cap, res), "aob")
    return list(res[:n]), out


def aob_tile_frames():
    """PCM frames per tile of the PCM pass"""
    return int(load_library().atg_aob_tile_frames())


def aob_kernel_times():
    """{"sectors", "layout", "pcm": ms} of this thread's last call"""
    return _thread_times(load_library().atg_aob_kernel_times, 3)


# ------------------------------------------------- MLP titles (mlp_decode.hip)
def mlp_scan_device(d_bytes, bytes_cap, titles, fmt=PCM_S32, want_units=False):
    """every pass that writes no PCM over AOB bytes in device memory
    (atg_mlp_scan_device): ([MlpResult], total_samples) with sample_offset
    laid out for `fmt`, and the MlpUnit table of all titles' access units in
    order as a third item when want_units (a sizing call comes first)"""
    lib = load_library()
    arr, n = titles if isinstance(titles, tuple) else aob_titles(titles)
    res = (MlpResult * max(1, n))()
    total = ctypes.c_uint64()
    _check(lib, lib.atg_mlp_scan_device(ctypes.c_void_p(d_bytes), bytes_cap, arr, n, fmt, res,
                                        ctypes.byref(total), None, 0, None), "mlp")
    if not want_units:
        return list(res[:n]), total.value
    n_units = sum(res[i].access_units for i in range(n))
    units = (MlpUnit * max(1, n_units))()
    _check(lib, lib.atg_mlp_scan_device(ctypes.c_void_p(d_bytes), bytes_cap, arr, n, fmt, res,
                                        ctypes.byref(total), units, n_units, None), "mlp")
    return list(res[:n]), total.value, list(units[:n_units])


def mlp_decode_device(d_bytes, bytes_cap, titles, d_pcm, fmt, pcm_cap_samples):
    """all passes into d_pcm (atg_mlp_decode_device): [MlpResult]; raises
    ATGError(ATG_ERR_CAPACITY) when pcm_cap_samples is too small"""
    lib = load_library()
    arr, n = titles if isinstance(titles, tuple) else aob_titles(titles)
    res = (MlpResult * max(1, n))()
    _check(lib, lib.atg_mlp_decode_device(ctypes.c_void_p(d_bytes), bytes_cap, arr, n,
                                          ctypes.c_void_p(d_pcm), fmt, pcm_cap_samples, res,
                                          None), "mlp")
    return list(res[:n])


def mlp_decode_host(data, titles, cap_samples, fmt=PCM_S32, device=None):
    """AOB bytes in host memory -> ([MlpResult], int16 / int32 numpy array of
    cap_samples samples), staged through `device`"""
    lib = load_library()
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    arr, n = titles if isinstance(titles, tuple) else aob_titles(titles)
    res = (MlpResult * max(1, n))()
    out = np.zeros(max(1, cap_samples), dtype=np.int16 if fmt == PCM_S16 else np.int32)
    _check(lib, lib.atg_mlp_decode_host(
        default_device() if device is None else device, a.ctypes.data_as(ctypes.c_void_p),
        a.nbytes, arr, n, out.ctypes.data_as(ctypes.c_void_p), fmt, cap_samples, res), "mlp")
    return list(res[:n]), out


def mlp_kernel_times():
    """{pass name: ms} of this thread's last MLP call"""
    return _thread_times(load_library().atg_mlp_kernel_times, 10)


# ------------------------------------------------- PCM comparison (pcm_compare.hip)
def pcm_view(d_pcm, fmt, src_frames, sample_offset=0, window_offset=0):
    """PcmView over the src_frames frames whose first sample is
    d_pcm[sample_offset] (PCM_S16 / PCM_S32); view frame 0 is source frame
    window_offset"""
    return PcmView(d_pcm, sample_offset, src_frames, window_offset, fmt, 0)


def pcm_pair(a, b, frames, channels):
    return PcmPair(a, b, frames, channels, 0)


def _pc_call(call, pairs):
    lib = load_library()
    n = len(pairs)
    arr = (PcmPair * max(1, n))(*pairs)
    res = (PcmCmpResult * max(1, n))()
    st = call(lib, arr, n, res)
    _check(lib, st, "pcm_compare")
    return [res[i] for i in range(n)]


def pcm_compare_device(pairs):
    """first differing frame of every PcmPair, one launch for the batch
    (atg_pcm_compare_device) -> [first_mismatch or None]"""
    res = _pc_call(lambda lib, arr, n, res: lib.atg_pcm_compare_device(arr, n, res, None), pairs)
    return [None if r.first_mismatch == PCM_NO_MISMATCH else int(r.first_mismatch) for r in res]


def pcm_offset_search_device(pairs, max_offset):
    """the shift k of smallest |k| in [-max_offset, max_offset] with
    a(i) == b(i + k) over every PcmPair (atg_pcm_offset_search_device)
    -> [(offset or None, first_mismatch at shift 0 or None)]"""
    res = _pc_call(lambda lib, arr, n, res: lib.atg_pcm_offset_search_device(
        arr, n, max_offset, res, None), pairs)
    return [(int(r.offset) if r.offset_found else None,
             None if r.first_mismatch == PCM_NO_MISMATCH else int(r.first_mismatch))
            for r in res]


def pcm_compare_tile_frames():
    """PCM frames per tile of the compare pass"""
    return int(load_library().atg_pcm_compare_tile_frames())


def pcm_compare_kernel_times():
    """{"compare": ms, "probe": ms} of this thread's last compare or search"""
    return _thread_times(load_library().atg_pcm_compare_kernel_times, 2)


# ------------------------------------------------- converter chain (pcm_chain.hip)
def pcm_chain_row(src, in_channels, out_channels, in_bps, out_bps, out_offset,
                  channel_op=CHAIN_MAP, channel_map=None, channel_mask=0, dither_bit0=0):
    """PcmChainRow over the PcmView `src`; channel_map (MAP): per output
    channel an input channel or None for silence, default the identity"""
    r = PcmChainRow()
    r.src = src
    r.in_channels, r.out_channels = in_channels, out_channels
    r.channel_op, r.channel_mask = channel_op, channel_mask
    if channel_map is None:
        channel_map = list(range(out_channels))
    for k in range(8):
        m = channel_map[k] if k < len(channel_map) else None
        r.map[k] = CHAIN_SILENT if m is None else m
    r.in_bps, r.out_bps = in_bps, out_bps
    r.out_offset, r.dither_bit0 = out_offset, dither_bit0
    return r


def pcm_chain_device(rows, d_out, out_fmt, out_cap_samples, d_dither=None, dither_bytes=0):
    """every PcmChainRow converted in one launch, device memory in and out
    (atg_pcm_chain_device)"""
    lib = load_library()
    arr = (PcmChainRow * max(1, len(rows)))(*rows)
    _check(lib, lib.atg_pcm_chain_device(
        arr, len(rows), ctypes.c_void_p(d_out), out_fmt, out_cap_samples,
        ctypes.c_void_p(d_dither) if d_dither else None, dither_bytes, None), "pcm_chain")


def pcm_chain_host(rows, out, dither=b"", device=None):
    """the same for host memory (atg_pcm_chain_host): the rows' src.d_pcm are
    host addresses (of arrays the caller keeps alive), `out` an int16 or
    int32 numpy array of which only the rows' ranges change"""
    lib = load_library()
    arr = (PcmChainRow * max(1, len(rows)))(*rows)
    d = np.frombuffer(bytes(dither), dtype=np.uint8) if len(dither) else None
    _check(lib, lib.atg_pcm_chain_host(
        default_device() if device is None else device, arr, len(rows),
        out.ctypes.data_as(ctypes.c_void_p), PCM_S16 if out.dtype == np.int16 else PCM_S32,
        len(out), d.ctypes.data_as(ctypes.c_void_p) if d is not None else None,
        0 if d is None else len(d)), "pcm_chain")
    return out


def pcm_chain_tile_samples():
    """samples per tile of the chain kernel, on a row's wider side"""
    return int(load_library().atg_pcm_chain_tile_samples())


def pcm_chain_tile_frames(in_channels, out_channels):
    """PCM frames per tile of a row with these channel counts"""
    return 8 * (pcm_chain_tile_samples() // (8 * max(in_channels, out_channels)))


def pcm_chain_kernel_times():
    """{"chain": ms} of this thread's last launch"""
    return _thread_times(load_library().atg_pcm_chain_kernel_times, 1)


# --------------------------------------------------- device-side dither (dither.hip)
def dither_fill_device(runs, seed, d_out, out_cap, stream=None):
    """runs: [(stream, first_block, blocks, byte_offset)]; the 16-byte blocks
    of those streams under `seed` written to d_out in one launch
    (atg_dither_fill_device)"""
    lib = load_library()
    arr = (DitherRun * max(1, len(runs)))(*[DitherRun(*[int(v) for v in r]) for r in runs])
    _check(lib, lib.atg_dither_fill_device(
        arr, len(runs), int(seed), ctypes.c_void_p(d_out) if d_out else None, out_cap,
        ctypes.c_void_p(stream) if stream else None), "dither")


def flac_index_range(offset, nbytes, si):
    """FlacIndexRange over `nbytes` of frame data at `offset` of the buffer,
    for a stream with the StreamInfo `si`"""
    return FlacIndexRange(offset, nbytes, si.sample_rate, si.channels, si.bits_per_sample,
                          si.max_block_size, si.min_block_size, 0)


def _flac_index_call(call, ranges, cap):
    """atg_flac_index_device / _host through `call(lib, ranges, n, entries,
    cap, count)` -> [(range, byte_offset, first_sample, block_size)] sorted;
    a capacity that proves too small is answered by one call with the
    count the first reported"""
    lib = load_library()
    n = len(ranges)
    arr = (FlacIndexRange * max(1, n))(*ranges)
    count = c_u64()
    while True:
        ents = (FlacIndexEntry * max(1, cap))()
        st = call(lib, arr, n, ents, cap, ctypes.byref(count))
        if st != ATG_ERR_CAPACITY:
            break
        cap = count.value
    _check(lib, st, "flac_index")
    rows = np.frombuffer(ents, dtype=FLAC_INDEX_ENTRY_DTYPE, count=count.value)
    return [(int(r), int(o), int(s), int(b)) for o, s, b, r in rows.tolist()]


FLAC_INDEX_ENTRY_DTYPE = np.dtype([("byte_offset", "<u8"), ("first_sample", "<u8"),
                                   ("block_size", "<u4"), ("range", "<u4")])


def flac_index_device(d_data, nbytes, ranges, cap=None):
    """the frame starts inside `ranges` (FlacIndexRange) of a device buffer
    -> [(range, byte_offset from the range's start, first_sample, block_size)]"""
    cap = sum(r.data_bytes for r in ranges) // 1024 + 64 if cap is None else cap
    return _flac_index_call(lambda lib, arr, n, ents, cap, count: lib.atg_flac_index_device(
        ctypes.c_void_p(d_data), nbytes, arr, n, ents, cap, count, None), ranges, cap)


def flac_index_host(data, ranges, cap=None, device=None):
    """flac_index_device over bytes in host memory, staged for the call"""
    data = bytes(data)
    cap = sum(r.data_bytes for r in ranges) // 1024 + 64 if cap is None else cap
    dev = default_device() if device is None else device
    return _flac_index_call(lambda lib, arr, n, ents, cap, count: lib.atg_flac_index_host(
        dev, data, len(data), arr, n, ents, cap, count), ranges, cap)


def flac_index_kernel_times():
    """{stage: ms} of this thread's last frame index call"""
    return _thread_times(load_library().atg_flac_index_kernel_times, 3)


def dither_tile_blocks():
    """16-byte blocks one workgroup of the fill kernel writes"""
    return int(load_library().atg_dither_tile_blocks())


def dither_kernel_times():
    """{"fill": ms} of this thread's last fill"""
    return _thread_times(load_library().atg_dither_kernel_times, 1)


# ------------------------------------------------------ tensors (pcm_tensor.hip)
def pcm_to_tensor_row(src, channels, bits_per_sample, pad_frames, out_offset, channel_stride):
    """PcmToTensorRow over the PcmView `src` (its src_frames is the row's
    length)"""
    return PcmToTensorRow(src, channels, bits_per_sample, pad_frames, out_offset, channel_stride)


def pcm_from_tensor_row(in_offset, channel_stride, frames, channels, bits_per_sample,
                        out_offset):
    return PcmFromTensorRow(in_offset, channel_stride, frames, channels, bits_per_sample,
                            out_offset)


def pcm_to_tensor_device(rows, d_out, dtype, out_cap_elems, stream=None):
    """rows: [PcmToTensorRow] -> the planar runs in device memory
    (atg_pcm_to_tensor_device); stream: a hipStream_t as an integer"""
    lib = load_library()
    arr = (PcmToTensorRow * max(len(rows), 1))(*rows)
    _check(lib, lib.atg_pcm_to_tensor_device(
        arr, len(rows), ctypes.c_void_p(d_out), dtype, out_cap_elems,
        ctypes.c_void_p(stream) if stream else None), "pcm_tensor")


def pcm_from_tensor_device(rows, d_in, dtype, in_cap_elems, d_out, out_fmt, out_cap_samples,
                           stream=None):
    """rows: [PcmFromTensorRow] -> interleaved PCM in device memory
    (atg_pcm_from_tensor_device)"""
    lib = load_library()
    arr = (PcmFromTensorRow * max(len(rows), 1))(*rows)
    _check(lib, lib.atg_pcm_from_tensor_device(
        arr, len(rows), ctypes.c_void_p(d_in), dtype, in_cap_elems, ctypes.c_void_p(d_out),
        out_fmt, out_cap_samples, ctypes.c_void_p(stream) if stream else None), "pcm_tensor")


def pcm_tensor_tile_frames():
    """frames per tile of both tensor kernels"""
    return int(load_library().atg_pcm_tensor_tile_frames())


def pcm_tensor_kernel_times():
    """{"to_tensor" or "from_tensor": ms} of this thread's last tensor call"""
    return _thread_times(load_library().atg_pcm_tensor_kernel_times, 2)


def aiff_read_info(data):
    """(status, AiffInfo) of a whole AIFF file image (atg_aiff_read_info)"""
    info = AiffInfo()
    data = bytes(data)
    return int(load_library().atg_aiff_read_info(data, len(data), ctypes.byref(info))), info


def au_read_info(data):
    """(status, AuInfo) of a whole Sun AU file image (atg_au_read_info)"""
    info = AuInfo()
    data = bytes(data)
    return int(load_library().atg_au_read_info(data, len(data), ctypes.byref(info))), info


def apply_gain(pcm, channels, bits_per_sample, multiplier, chunk_frames, dither,
               dither_bit0=0, device=None):
    """ReplayGainReader sample transform on the GPU (atg_pcm_apply_gain_host)"""
    lib = load_library()
    a = np.ascontiguousarray(pcm, dtype=np.int32)
    out = np.empty(max(1, len(a)), dtype=np.int32)
    d = np.frombuffer(bytes(dither) or b"\0", dtype=np.uint8)
    st = lib.atg_pcm_apply_gain_host(
        default_device() if device is None else device, a.ctypes.data_as(ctypes.c_void_p),
        out.ctypes.data_as(ctypes.c_void_p), len(a) // channels, channels, bits_per_sample,
        multiplier, chunk_frames, d.ctypes.data_as(ctypes.c_void_p), len(d), dither_bit0)
    _check(lib, st, "pcm_convert")
    return out[:len(a)]


# ------------------------------------------------------------------ resampler
def resample_output_frames(in_frames, channels, in_rate, out_rate):
    return int(load_library().atg_resample_output_frames(in_frames, channels, in_rate, out_rate))


def resample_tracks(tracks, channels):
    """[(pcm_offset, pcm_frames, in_rate, out_rate[, reads])] -> RsTrack
    array (reads: the upstream read() frame counts, None = 4096-frame
    reads); the read arrays are kept alive on the returned object"""
    arr = (RsTrack * max(1, len(tracks)))()
    keep = []
    for i, t in enumerate(tracks):
        off, n, a, b = t[:4]
        arr[i].pcm_offset, arr[i].pcm_frames = off, n
        arr[i].in_rate, arr[i].out_rate = a, b
        reads = t[4] if len(t) > 4 else None
        if reads is not None:
            r = np.ascontiguousarray(reads, dtype=np.uint32)
            keep.append(r)
            arr[i].reads = r.ctypes.data_as(ctypes.POINTER(c_u32))
            arr[i].n_reads = len(r)
    arr._keep = keep
    return arr


def resample_device(d_in, d_out, out_cap_samples, tracks, channels, bits_per_sample,
                    stream=None):
    """resample a batch whose int32 PCM is in device memory
    -> (out frame offsets, out frame counts) numpy uint64"""
    lib = load_library()
    n = len(tracks)
    arr = resample_tracks(tracks, channels)
    offs = np.zeros(max(1, n), dtype=np.uint64)
    cnt = np.zeros(max(1, n), dtype=np.uint64)
    _check(lib, lib.atg_resample_device(
        arr, n, channels, bits_per_sample, ctypes.c_void_p(d_in), ctypes.c_void_p(d_out),
        out_cap_samples, offs.ctypes.data_as(ctypes.c_void_p),
        cnt.ctypes.data_as(ctypes.c_void_p), stream), "resample")
    return offs[:n], cnt[:n]


def resample_host(pcm, tracks, channels, bits_per_sample, device=None):
    """resample int32 interleaved PCM held in host memory (atg_resample_host)
    -> (int32 output, out frame offsets, out frame counts)"""
    lib = load_library()
    a = np.ascontiguousarray(pcm, dtype=np.int32)
    n = len(tracks)
    total = 0
    for t in tracks:
        if len(t) > 4 and t[4] is not None:
            total += sum(resample_read_sizes(t[1], channels, t[2], t[3], t[4]))
        else:
            total += resample_output_frames(t[1], channels, t[2], t[3])
    out = np.empty(max(1, total * channels), dtype=np.int32)
    offs = np.zeros(max(1, n), dtype=np.uint64)
    cnt = np.zeros(max(1, n), dtype=np.uint64)
    _check(lib, lib.atg_resample_host(
        default_device() if device is None else device, resample_tracks(tracks, channels), n,
        channels, bits_per_sample, a.ctypes.data_as(ctypes.c_void_p), len(a),
        out.ctypes.data_as(ctypes.c_void_p), total * channels,
        offs.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p)), "resample")
    return out[:total * channels], offs[:n], cnt[:n]


def resample_read_sizes(in_frames, channels, in_rate, out_rate, reads):
    """frame counts of successive Resampler.read() calls (the last is 0)"""
    lib = load_library()
    r = np.ascontiguousarray(reads, dtype=np.uint32)
    cap = len(r) + 16
    while True:
        sizes = np.zeros(cap, dtype=np.uint32)
        k = lib.atg_resample_read_sizes(in_frames, channels, in_rate, out_rate,
                                        r.ctypes.data_as(ctypes.c_void_p), len(r),
                                        sizes.ctypes.data_as(ctypes.c_void_p), cap)
        if k < 0:
            raise ValueError("invalid sample rate")
        if k <= cap:
            return [int(x) for x in sizes[:k]]
        cap = int(k)


def resample_kernel_times():
    """{"rs_positions", "rs_filter": ms} of this thread's last resample"""
    return _thread_times(load_library().atg_resample_kernel_times, 4)
