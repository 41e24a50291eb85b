"""The Shorten test inputs, shared by tests/golden/make_shn_golden.py (which
records what the reference's shnenc and shndec make of them) and the Shorten
tests (which hold shn_port and the GPU codec to the record)."""
import numpy as np

import shn_port
import signals

FIXTURES = ("shorten-frames.shn", "shorten-lpc.shn")
BLOCKS = (3, 4, 255, 256, 4096)


def lengths(block):
    return (0, 1, block - 1, block, block + 1, 3 * block + 5)


def constant(n, ch, value=1234):
    return np.full(n * ch, value, dtype=np.int32)


def square(n, ch, bps):
    hi, lo = (1 << (bps - 1)) - 1, -(1 << (bps - 1))
    x = np.where((np.arange(n) // 7) % 2 == 0, hi, lo)
    return np.repeat(x[:, None], ch, 1).reshape(-1).astype(np.int32)


def stepped_shifts(n, ch, block, seed):
    """samples that are multiples of 4 or 16, the multiple changing per
    block and per channel"""
    rng = np.random.RandomState(seed)
    x = rng.randint(-1500, 1500, size=(n, ch)).astype(np.int64)
    for b in range(0, n, block):
        for c in range(ch):
            x[b:b + block, c] *= (4, 16, 1)[(b // block + c) % 3]
    return x.reshape(-1).astype(np.int32)


def silent_beside_shifted(n, block, seed):
    """channel 0 silent in every other block, channel 1 multiples of 8: a
    ZERO command must leave the shift state alone"""
    rng = np.random.RandomState(seed)
    x = np.zeros((n, 2), dtype=np.int64)
    x[:, 1] = rng.randint(-900, 900, size=n) * 8
    x[:, 0] = rng.randint(-900, 900, size=n)
    for b in range(0, n, 2 * block):
        x[b:b + block, 0] = 0
    return x.reshape(-1).astype(np.int32)


def impulse(n, at):
    x = np.zeros(n, dtype=np.int32)
    x[at] = 32767
    return x


def wave_header(n_bytes, extra=0):
    import struct
    return (b"RIFF" + struct.pack("<I", 36 + n_bytes + extra) + b"WAVEfmt " +
            struct.pack("<IHHIIHH", 16, 1, 2, 44100, 176400, 4, 16) + b"data" +
            struct.pack("<I", n_bytes))


def encoder_cases():
    """what shnenc can make: [(name, channels, bps, block, samples, header, footer)]"""
    out = []
    for block in BLOCKS:
        for n in lengths(block):
            out.append(("tone_c2_b16_B%d_n%d" % (block, n), 2, 16, block,
                        signals.make("tone", n, 2, 16, seed=block + n), b"", b""))
    n = 3 * 256 + 5
    for ch in (1, 3, 8):
        for bps in (8, 16):
            out.append(("noise_c%d_b%d" % (ch, bps), ch, bps, 256,
                        signals.make("noise", n, ch, bps, seed=ch * 10 + bps), b"", b""))
    out.append(("tone_c2_b8", 2, 8, 256, signals.make("tone", n, 2, 8, seed=5), b"", b""))
    out.append(("silence_c2", 2, 16, 256, signals.make("silence", n, 2, 16), b"", b""))
    out.append(("constant_c2", 2, 16, 256, constant(n, 2), b"", b""))
    out.append(("square_c2_b16", 2, 16, 256, square(n, 2, 16), b"", b""))
    out.append(("square_c1_b8", 1, 8, 4, square(23, 1, 8), b"", b""))
    out.append(("stepped_c3", 3, 16, 256, stepped_shifts(4 * 256 + 9, 3, 256, 7), b"", b""))
    out.append(("stepped_c2_B4", 2, 16, 4, stepped_shifts(41, 2, 4, 8), b"", b""))
    out.append(("silent_beside_shifted", 2, 16, 256, silent_beside_shifted(6 * 256 + 3, 256, 9),
                b"", b""))
    out.append(("impulse_B4096", 1, 16, 4096, impulse(4096, 2000), b"", b""))
    tone = signals.make("tone", 700, 2, 16, seed=3)
    out.append(("head44_foot1", 2, 16, 256, tone, wave_header(2800, 1), b"\x00"))
    out.append(("head300_foot9", 2, 16, 256, tone,
                bytes(bytearray((i * 7 + 1) & 0xFF for i in range(300))), b"LISTabcde"))
    return out


def port_cases():
    """what shnenc cannot make (unsigned and big-endian types, explicit frame
    sizes), checked through shndec:
    [(name, channels, bps, block, samples, header, footer, big_endian, signed, sizes)]"""
    out = []
    n = 2 * 256 + 77
    for bps in (8, 16):
        x = signals.make("tone", n, 2, bps, seed=bps)
        out.append(("unsigned_b%d" % bps, 2, bps, 256, x, b"", b"", False, False, None))
    x = signals.make("noise", n, 2, 16, seed=21)
    out.append(("big_endian_signed", 2, 16, 256, x, b"", b"", True, True, None))
    out.append(("big_endian_unsigned", 2, 16, 256, x, b"hd", b"ft", True, False, None))
    out.append(("unsigned_silence", 1, 16, 256, np.zeros(300, np.int32), b"", b"", False, False,
                None))
    sizes = [256, 100, 100, 7, 256, 3, 4096, 50]
    x = stepped_shifts(sum(sizes), 2, 100, 31)
    out.append(("sizes_mid_stream", 2, 16, 256, x, b"", b"", False, True, sizes))
    sizes = [4, 4, 3, 5, 4, 1]
    out.append(("sizes_small", 3, 16, 4, signals.make("noise", sum(sizes), 3, 16, seed=2), b"", b"",
                False, True, sizes))
    return out


def mixed_batch():
    """tracks of unequal length for one encode call"""
    return [signals.make(k, n, 2, 16, seed=n) for k, n in
            (("tone", 1000), ("noise", 1), ("silence", 513), ("tone", 0), ("chirp", 2049),
             ("noise", 255), ("tone", 256 * 3))] + [silent_beside_shifted(700, 256, 4)]


def builder_streams():
    """{name: image} of streams only the builder can write"""
    B = shn_port.Builder
    rng = np.random.RandomState(77)
    out = {}

    def res(n, amp):
        return rng.randint(-amp, amp + 1, size=n)

    for mc in (1, 4):
        b = B(5, 2, 40, 0, mc)
        for k in range(5):
            for c in range(2):
                b.diff(0 if (k + c) % 2 else 1 + (k % 3), 4, res(40, 60))
        out["diff0_means%d" % mc] = b.quit()
    b = B(5, 1, 50, 8, 2)
    for order in (0, 1, 3, 8, 8, 3):
        b.qlpc(3, res(order, 15), res(50, 20))
    b.diff(3, 3, res(50, 20))
    out["qlpc_orders"] = b.quit()
    b = B(3, 2, 64, 8, 1)
    for k in range(3):
        b.qlpc(2, res(8, 12), res(64, 9)).diff(2, 2, res(64, 9))
    out["qlpc_stereo_big_endian"] = b.quit()
    b = B(5, 1, 30, 0, 0).diff(3, 5, res(30, 100))
    b.blocksize(1).diff(1, 5, res(1, 100)).blocksize(30).diff(3, 5, res(30, 100))
    b.blocksize(2).diff(2, 5, res(2, 100)).blocksize(30).diff(3, 5, res(30, 100))
    b.blocksize(2).diff(2, 5, res(2, 100)).blocksize(1).diff(1, 2, res(1, 9))
    b.blocksize(70).diff(3, 5, res(70, 100)).diff(2, 5, res(70, 100))
    out["short_history"] = b.quit()
    b = B(6, 2, 33, 0, 0)
    for k, s in enumerate((0, 3, 3, 1, 9, 0)):
        b.bitshift(s)
        b.diff(1 + k % 3, 3, res(33, 30))
        if k % 2:
            b.verbatim(b"mid%d" % k)
        b.zero() if k == 2 else b.diff(2, 3, res(33, 30))
    out["shifts_verbatim_unsigned"] = b.verbatim(b"tail").quit()
    b = B(2, 1, 100, 0, 0).verbatim(b"eight").diff(1, 0, res(100, 2)).diff(2, 1, res(100, 3))
    out["unsigned8_energy0"] = b.quit()
    # 40000 at energy 2 is a zero run of 10000 bits
    b = B(5, 1, 300, 0, 0).diff(1, 2, [0] * 16 + [40000] + [0] * 283)
    b.diff(1, 20, res(300, 400000))
    out["zero_run_energy20"] = b.quit()
    b = B(5, 2, 200, 0, 0)
    for k in range(6):
        b.diff(1 + k % 3, 1 + k, res(200, 3 << k))
        b.zero() if k == 3 else b.diff(3, 2 + k, res(200, 6 << k))
    out["long_runs_stereo"] = b.quit()
    # the ends a stream can come to
    out["no_quit"] = B(5, 1, 10).diff(1, 2, res(10, 5)).unfinished()
    out["unknown_command"] = B(5, 1, 10).diff(1, 2, res(10, 5)).command(11).quit()
    out["incomplete_set"] = B(5, 2, 10).diff(1, 2, res(10, 5)).diff(1, 2, res(10, 5)) \
        .diff(1, 2, res(10, 5)).quit()
    out["incomplete_set_then_verbatim"] = B(5, 2, 10).verbatim(b"front") \
        .diff(1, 2, res(10, 5)).diff(2, 2, res(10, 5)).diff(1, 2, res(10, 5)) \
        .verbatim(b"late").quit()
    return out


def unsupported_streams():
    """{name: image} of streams only the limits of include/atgpu.h refuse"""
    B = shn_port.Builder
    r = [1, -1, 2, 0]
    return {
        "channels_0": B(5, 0, 4).diff(1, 1, r).quit(),
        "channels_257": B(5, 257, 4).diff(1, 1, r).quit(),
        "block_length_0": B(5, 1, 0).diff(1, 1, []).quit(),
        "diff0_no_means": B(5, 1, 4).diff(1, 1, r).diff(0, 1, r).quit(),
        "qlpc_no_means": B(5, 1, 4).qlpc(1, [1], r).quit(),
        "shift_32": B(5, 1, 4).diff(1, 1, r).bitshift(32).diff(1, 1, r).quit(),
        "energy_32": B(5, 1, 4).diff(1, 1, r).diff(1, 32, r).quit(),
        "lpc_count_33": B(5, 1, 4, 33, 1).qlpc(1, [1] * 33, r).quit(),
        "zero_2_32": B(5, 1, 4).diff(1, 1, r).blocksize(0xFFFFFFFF).zero().quit(),
        "length_changes_in_set": B(5, 2, 4).diff(1, 1, r).blocksize(3).diff(1, 1, r[:3]).quit(),
        "means_65": B(5, 1, 4, 0, 65).diff(1, 1, r).quit(),
    }


def pcm_bytes(samples, bps):
    """little-endian signed PCM, as the reference's tools read and write it
    (shndec's converter clamps a sample that does not fit)"""
    a = np.clip(np.asarray(samples, dtype=np.int64), -(1 << (bps - 1)), (1 << (bps - 1)) - 1)
    return a.astype(np.int8).tobytes() if bps == 8 else a.astype("<i2").tobytes()
