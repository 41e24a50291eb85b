"""audiotools.pcmconverter — the integer PCM converters on the MI355X.

Same names and reader contract as the reference's C types
(src/pcmconverter.c, used by audiotools/__init__.py:2729-2802 when
track2track changes bits per sample or channel count):

  BPSConverter(pcmreader, bits_per_sample)   BPSConverter_read :667-747
  Downmixer(pcmreader)   -> 2 channels       Downmixer_read    :220-342
  Averager(pcmreader)    -> 1 channel        Averager_read     :64-97
  Resampler(pcmreader, sample_rate)          Resampler_read    :439-495

Each read() pulls 4096 PCM frames from the wrapped reader, as the reference
does, and converts them with pcm_convert.hip (atg_pcm_convert_host).  Dither
bits come from os.urandom like the reference's (src/dither.c), consumed
MSB first, one per sample, channel by channel within each read; pass
`dither=` (a callable n -> bytes) to make a conversion reproducible.
No CPU path: a missing library raises ImportError.

convert_pcm_batch is the same chain for a whole batch of tracks without the
readers: PCMConverter's stack planned per track (plan_chain), then run over
device memory by csrc/pcm_chain.hip (atg_pcm_chain_device) -- one launch
for tracks whose rate stays, two with atg_resample_device between them for
the others -- instead of an upload, a launch and a download per 4096 frames
per stage.  audiotools.convert_files_batch runs it between the decoders
and the FLAC encoder.

Resampler drains the wrapped reader on its first read() (recording what each
read(4096) returned), resamples the whole track in one GPU batch
(resample.hip, atg_resample_host) and then hands out the frames in the
chunks the reference's src_process loop would have produced
(atg_resample_read_sizes).
"""

import os
from collections import OrderedDict, namedtuple

import numpy as np

from . import _atgpu
from . import pcm


class _Converter(object):
    kind = None

    def __init__(self, pcmreader):
        self.pcmreader = pcmreader
        self.sample_rate = pcmreader.sample_rate
        self._closed = False

    def close(self):
        """closes the wrapped reader; later reads raise ValueError"""
        self._closed = True
        self.pcmreader.close()

    def _input(self):
        if self._closed:
            raise ValueError("cannot read closed stream")
        fl = self.pcmreader.read(4096)
        if not isinstance(fl, pcm.FrameList):
            raise TypeError("pcmreader.read() must return a FrameList")
        return fl


class BPSConverter(_Converter):
    kind = _atgpu.CONV_BPS

    def __init__(self, pcmreader, bits_per_sample, dither=None):
        _Converter.__init__(self, pcmreader)
        self.channels = pcmreader.channels
        self.channel_mask = pcmreader.channel_mask
        self.bits_per_sample = bits_per_sample
        self._rand = dither if dither is not None else os.urandom
        self._bits = b""
        self._bitpos = 0

    def _dither_bits(self, n):
        """bytes holding the next n dither bits at offset self._bitpos"""
        have = len(self._bits) * 8 - self._bitpos
        if have < n:
            need = (n - have + 7) // 8
            self._bits = self._bits[self._bitpos // 8:] + self._rand(max(need, 4096))
            self._bitpos %= 8
        start = self._bitpos
        self._bitpos += n
        return self._bits, start

    def read(self, pcm_frames):
        fl = self._input()
        ib, ob = self.pcmreader.bits_per_sample, self.bits_per_sample
        if ib == ob or fl.frames == 0:
            return pcm.FrameList._wrap(fl.samples, self.channels, ob)
        kw = {}
        if ob < ib:
            bits, bit0 = self._dither_bits(len(fl))
            kw = dict(dither=bits, dither_bit0=bit0)
        out = _atgpu.pcm_convert(self.kind, fl.samples, self.channels, ib, ob, **kw)
        return pcm.FrameList._wrap(out, self.channels, ob)


class Downmixer(_Converter):
    kind = _atgpu.CONV_DOWNMIX

    def __init__(self, pcmreader):
        _Converter.__init__(self, pcmreader)
        self.channels = 2
        self.channel_mask = 0x3
        self.bits_per_sample = pcmreader.bits_per_sample

    def read(self, pcm_frames):
        fl = self._input()
        if fl.frames == 0:
            return pcm.empty_framelist(2, self.bits_per_sample)
        out = _atgpu.pcm_convert(self.kind, fl.samples, self.pcmreader.channels,
                                 self.bits_per_sample,
                                 channel_mask=self.pcmreader.channel_mask)
        return pcm.FrameList._wrap(out, 2, self.bits_per_sample)


class Averager(_Converter):
    kind = _atgpu.CONV_AVERAGE

    def __init__(self, pcmreader):
        _Converter.__init__(self, pcmreader)
        self.channels = 1
        self.channel_mask = 0x4
        self.bits_per_sample = pcmreader.bits_per_sample

    def read(self, pcm_frames):
        fl = self._input()
        if fl.frames == 0:
            return pcm.empty_framelist(1, self.bits_per_sample)
        out = _atgpu.pcm_convert(self.kind, fl.samples, self.pcmreader.channels,
                                 self.bits_per_sample)
        return pcm.FrameList._wrap(out, 1, self.bits_per_sample)


class Resampler(object):
    """reference pcmconverter.Resampler (src/pcmconverter.c:370-495):
    libsamplerate sinc interpolation to `sample_rate`, bits per sample and
    channels unchanged; read() returns what one src_process round yields
    and an empty FrameList at the end"""

    def __init__(self, pcmreader, sample_rate):
        sample_rate = int(sample_rate)
        if sample_rate <= 0:
            raise ValueError("new sample rate must be positive")
        self.pcmreader = pcmreader
        self.sample_rate = sample_rate
        self.channels = pcmreader.channels
        self.channel_mask = pcmreader.channel_mask
        self.bits_per_sample = pcmreader.bits_per_sample
        self._chunks = None
        self._closed = False

    def _run(self):
        ratio = float(self.sample_rate) / float(self.pcmreader.sample_rate)
        if ratio > 256 or ratio < 1.0 / 256:
            raise ValueError("SRC ratio outside [1/256, 256] range.")
        parts, reads = [], []
        while True:
            fl = self.pcmreader.read(4096)
            if not isinstance(fl, pcm.FrameList):
                raise TypeError("pcmreader.read() must return a FrameList")
            if fl.frames == 0:
                break
            parts.append(fl.samples)
            reads.append(fl.frames)
        data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
        frames = len(data) // self.channels
        out, _, counts = _atgpu.resample_host(
            data, [(0, frames, self.pcmreader.sample_rate, self.sample_rate, reads)],
            self.channels, self.bits_per_sample)
        sizes = _atgpu.resample_read_sizes(frames, self.channels,
                                           self.pcmreader.sample_rate, self.sample_rate, reads)
        if sum(sizes) != int(counts[0]):
            raise RuntimeError("resampler frame count disagrees with its read sizes")
        self._out = out
        self._chunks = sizes
        self._next = 0
        self._pos = 0

    def read(self, pcm_frames):
        if self._closed:
            raise ValueError("cannot read closed stream")
        if self._chunks is None:
            self._run()
        if self._next >= len(self._chunks):
            return pcm.empty_framelist(self.channels, self.bits_per_sample)
        n = self._chunks[self._next]
        self._next += 1
        a = self._pos * self.channels
        self._pos += n
        return pcm.FrameList._wrap(self._out[a:a + n * self.channels].copy(), self.channels,
                                   self.bits_per_sample)

    def close(self):
        self._closed = True
        self.pcmreader.close()


# ------------------------------------------------------------ the batch chain
# what PCMConverter builds for one track, as the chain kernel takes it
ChainPlan = namedtuple("ChainPlan", "op channel_map downmix_mask in_channels in_bits in_rate "
                       "channels channel_mask bits_per_sample sample_rate")


def plan_chain(src_channels, src_mask, src_bits, src_rate, sample_rate, channels, channel_mask,
               bits_per_sample):
    """PCMConverter(reader, sample_rate, channels, channel_mask,
    bits_per_sample) for a reader of the src_* parameters, as a ChainPlan;
    the ValueErrors PCMConverter, RemaskedPCMReader and Resampler raise are
    raised here, with their messages.  `channel_mask` of the plan is the
    mask the converted stream reports."""
    from . import ChannelMask, _check_mask
    if sample_rate <= 0:
        raise ValueError("invalid sample rate")
    if channels <= 0:
        raise ValueError("invalid channel count")
    if bits_per_sample not in (8, 16, 24):
        raise ValueError("invalid bits-per-sample")
    _check_mask(channel_mask, channels)
    op, cmap, out_mask = _atgpu.CHAIN_MAP, list(range(channels)), src_mask
    if src_channels > channels:
        if channels == 1 and channel_mask in (0, 0x4):
            op = _atgpu.CHAIN_DOWNMIX_AVERAGE if src_channels > 2 else _atgpu.CHAIN_AVERAGE
            out_mask = 0x4
        elif channels == 2 and channel_mask in (0, 0x3):
            op, out_mask = _atgpu.CHAIN_DOWNMIX, 0x3
        else:
            # RemaskedPCMReader: matching speakers forwarded, others silent
            out_mask = channel_mask
            if src_mask != 0 and channel_mask != 0:
                mask = ChannelMask(channel_mask)
                if len(mask) != channels:
                    raise ValueError("channel count and channel mask mismatch")
                have = ChannelMask(src_mask).channels()
                cmap = [have.index(c) if c in have else None for c in mask.channels()]
    elif src_channels < channels:
        # ReorderedPCMReader: the first channel duplicated
        cmap = list(range(src_channels)) + [0] * (channels - src_channels)
        out_mask = channel_mask
    if src_rate != sample_rate:
        ratio = float(sample_rate) / float(src_rate)
        if ratio > 256 or ratio < 1.0 / 256:
            raise ValueError("SRC ratio outside [1/256, 256] range.")
    return ChainPlan(op, cmap, src_mask, src_channels, src_bits, src_rate, channels, out_mask,
                     bits_per_sample, sample_rate)


def plan_target(params, sample_rate=None, channels=None, channel_mask=None,
                bits_per_sample=None):
    """ChainPlan of a track of params (channels, channel_mask,
    bits_per_sample, sample_rate) for a target in which None keeps the
    track's own value; a channel mask left open is the track's when its
    channel count stays, else 0"""
    ch, mask, bits, rate = [int(p) for p in params]
    t_ch = ch if channels is None else channels
    if channel_mask is None:
        channel_mask = mask if t_ch == ch else 0
    return plan_chain(ch, mask, bits, rate, rate if sample_rate is None else sample_rate, t_ch,
                      int(channel_mask), bits if bits_per_sample is None else bits_per_sample)


# a track's PCM in device memory, before and after the chain
DevicePcm = namedtuple("DevicePcm", "d_pcm fmt sample_offset frames")


def _round_up(x, m):
    return (x + m - 1) // m * m


class DeviceDither(object):
    """The dither source of the batch paths that stays on the device: pass
    one as `dither=` to run_chain_device, convert_pcm_batch,
    convert_files_batch or load_batch and the bits are made in device memory
    by csrc/dither.hip (atg_dither_fill_device) instead of being drawn and
    uploaded by the host.  Track k of a call's sources reads stream k of a
    counter-based generator (Philox4x32-10, include/atgpu_dither.h) under
    the 64-bit `seed`, from the stream's bit 0 on, so a seed fixes a call's
    result and tests/dither_port.py reproduces it.  seed=None takes 8 bytes
    of os.urandom once, here, and keeps them in .seed."""

    def __init__(self, seed=None):
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError("seed must fit 64 bits")
        self.seed = seed


def run_chain_device(sources, plans, dither=None, int16_out=True, streams=None):
    """The chain over device memory.  sources: [DevicePcm]; plans:
    [ChainPlan].  -> ([DevicePcm] of the converted tracks, device pointers
    to free once they are used).  Tracks of at most 16 output bits land in
    an int16 buffer when int16_out is set, the others in an int32 one; every
    track starts on a 16-byte boundary, whole frames from its buffer's start.  The dither bytes are drawn from
    `dither` (n -> bytes, default os.urandom) track by track in order, one
    draw of ceil(bits / 8) bytes per track that reduces.  With a
    DeviceDither nothing is drawn here: track i's bits are stream
    streams[i] (default i) of its generator, written by one fill launch into
    the dither buffer, every track's on a 16-byte boundary."""
    on_device = isinstance(dither, DeviceDither)
    rand = os.urandom if dither is None else dither
    if streams is None:
        streams = range(len(sources))
    eng = _atgpu.engine()
    free = []

    def alloc(nbytes):
        free.append(eng.device_alloc(max(16, nbytes)))
        return free[-1]

    try:
        n = len(sources)
        stage = list(sources)  # what the last pass reads
        resampled = [i for i in range(n)
                     if plans[i].in_rate != plans[i].sample_rate and sources[i].frames]
        if resampled:
            # pass 1: the channel stage alone, into one int32 buffer in which
            # the tracks of a (channels, bits) group lie whole frames apart
            groups = OrderedDict()
            for i in resampled:
                groups.setdefault((plans[i].channels, plans[i].in_bits), []).append(i)
            pos, base, start = 0, {}, {}
            for key, members in groups.items():
                pos = base[key] = _round_up(pos, 4)
                for i in members:
                    pos = start[i] = base[key] + _round_up(pos - base[key], 4 * key[0])
                    pos += sources[i].frames * key[0]
            d_mid = alloc(4 * pos)
            rows = []
            for i in resampled:
                p, s = plans[i], sources[i]
                rows.append(_atgpu.pcm_chain_row(
                    _atgpu.pcm_view(s.d_pcm, s.fmt, s.frames, s.sample_offset), p.in_channels,
                    p.channels, p.in_bits, p.in_bits, start[i], p.op, p.channel_map,
                    p.downmix_mask))
            _atgpu.pcm_chain_device(rows, d_mid, _atgpu.PCM_S32, pos)
            for (ch, bits), members in groups.items():
                tracks = [((start[i] - base[(ch, bits)]) // ch, sources[i].frames,
                           plans[i].in_rate, plans[i].sample_rate) for i in members]
                cap = sum(_atgpu.resample_output_frames(t[1], ch, t[2], t[3])
                          for t in tracks) * ch
                d_rs = alloc(4 * cap)
                offs, counts = _atgpu.resample_device(d_mid + 4 * base[(ch, bits)], d_rs, cap,
                                                      tracks, ch, bits)
                for i, o, c in zip(members, offs, counts):
                    stage[i] = DevicePcm(d_rs, _atgpu.PCM_S32, int(o) * ch, int(c))
        # the last pass: channel stage and bits for the tracks whose rate
        # stays, bits alone behind the resampler
        fmts = [_atgpu.PCM_S16 if int16_out and p.bits_per_sample <= 16 else _atgpu.PCM_S32
                for p in plans]
        sizes, starts = {_atgpu.PCM_S16: 0, _atgpu.PCM_S32: 0}, []
        for s, p, f in zip(stage, plans, fmts):
            # on a 16-byte boundary and whole frames from the buffer's start
            starts.append(_round_up(sizes[f], 8 * p.channels))
            sizes[f] = starts[-1] + s.frames * p.channels
        bits_at, parts, runs, nbytes = [], [], [], 0
        for s, p, stream in zip(stage, plans, streams):
            bits_at.append(8 * nbytes)
            if p.bits_per_sample < p.in_bits and s.frames:
                want = (s.frames * p.channels + 7) // 8
                if on_device:
                    blocks = (want + 15) // 16
                    runs.append((stream, 0, blocks, nbytes))
                    nbytes += 16 * blocks
                    continue
                parts.append(bytes(rand(want)))
                if len(parts[-1]) != want:
                    raise ValueError("dither callable returned the wrong number of bytes")
                nbytes += want
        d_dither = None
        if nbytes:
            d_dither = alloc(nbytes)
            if on_device:
                _atgpu.dither_fill_device(runs, dither.seed, d_dither, nbytes)
            else:
                eng.copy_to_device(d_dither, np.frombuffer(b"".join(parts), dtype=np.uint8))
        out = [None] * n
        for fmt in (_atgpu.PCM_S16, _atgpu.PCM_S32):
            members = [i for i in range(n) if fmts[i] == fmt]
            if not members:
                continue
            d_out = alloc((2 if fmt == _atgpu.PCM_S16 else 4) * sizes[fmt])
            rows = []
            for i in members:
                p, s = plans[i], stage[i]
                out[i] = DevicePcm(d_out, fmt, starts[i], s.frames)
                if not s.frames:
                    continue
                view = _atgpu.pcm_view(s.d_pcm, s.fmt, s.frames, s.sample_offset)
                if s is sources[i]:
                    rows.append(_atgpu.pcm_chain_row(
                        view, p.in_channels, p.channels, p.in_bits, p.bits_per_sample,
                        starts[i], p.op, p.channel_map, p.downmix_mask, bits_at[i]))
                else:
                    rows.append(_atgpu.pcm_chain_row(
                        view, p.channels, p.channels, p.in_bits, p.bits_per_sample, starts[i],
                        dither_bit0=bits_at[i]))
            _atgpu.pcm_chain_device(rows, d_out, fmt, sizes[fmt], d_dither, nbytes)
        return out, free
    except Exception:
        for d in free:
            eng.device_free(d)
        raise


def convert_pcm_batch(arrays, params, sample_rate=None, channels=None, channel_mask=None,
                      bits_per_sample=None, dither=None):
    """PCMConverter for a batch of tracks held as numpy arrays.  arrays:
    interleaved int16 or int32 PCM, one array per track; params: per track
    (channels, channel_mask, bits_per_sample, sample_rate); the target is
    shared, None keeping each track's own value.  -> one int32 array per
    track: what reading PCMConverter(reader of the track, ...) to its end
    gives (under a resampler the dither bits fall on other samples, see
    DESIGN section 4o).  ValueError, before any GPU work, for what
    PCMConverter refuses.  dither: n -> bytes, default os.urandom; the
    tracks that lose bits draw in order."""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    params = list(params)
    if len(arrays) != len(params):
        raise ValueError("arrays and params differ in length")
    plans = [plan_target(p, sample_rate, channels, channel_mask, bits_per_sample)
             for p in params]
    for a, p in zip(arrays, plans):
        if a.dtype not in (np.int16, np.int32):
            raise ValueError("PCM arrays must be int16 or int32")
        if a.ndim != 1 or len(a) % p.in_channels:
            raise ValueError("PCM arrays must hold whole interleaved frames")
    if not arrays:
        return []
    # every array on a 16-byte boundary of one buffer
    at, pos = [], 0
    for a in arrays:
        at.append(pos)
        pos += _round_up(a.nbytes, 16)
    host = np.zeros(max(pos, 16), dtype=np.uint8)
    for a, s in zip(arrays, at):
        host[s:s + a.nbytes] = a.view(np.uint8)
    eng = _atgpu.engine()
    d_in = eng.device_alloc(len(host))
    free = [d_in]
    try:
        eng.copy_to_device(d_in, host)
        sources = [DevicePcm(d_in + s, _atgpu.PCM_S16 if a.dtype == np.int16 else _atgpu.PCM_S32,
                             0, len(a) // p.in_channels)
                   for a, s, p in zip(arrays, at, plans)]
        done, more = run_chain_device(sources, plans, dither)
        free += more
        held, out = {}, []
        for d, p in zip(done, plans):
            if d.d_pcm not in held:
                n = max([x.sample_offset + x.frames * q.channels
                         for x, q in zip(done, plans) if x.d_pcm == d.d_pcm] + [1])
                held[d.d_pcm] = eng.copy_to_host(
                    np.empty(n, dtype=np.int16 if d.fmt == _atgpu.PCM_S16 else np.int32),
                    d.d_pcm)
            out.append(held[d.d_pcm][d.sample_offset:d.sample_offset + d.frames * p.channels]
                       .astype(np.int32))
        return out
    finally:
        for d in free:
            eng.device_free(d)
