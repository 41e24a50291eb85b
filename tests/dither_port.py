"""numpy port of the device-side dither source (include/atgpu_dither.h):
Philox4x32-10, one 16-byte block per counter value.  Byte j of stream s
under the 64-bit seed is byte j % 16 of the four little-endian output words
of Philox(counter = (lo32(j / 16), hi32(j / 16), lo32(s), hi32(s)),
key = (lo32(seed), hi32(seed)))."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox(counter, key):
    """counter: four uint32 arrays (or ints) of one shape; key: two ints.
    -> the four output words as uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in counter]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    lo, sh = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]   # < 2^64: no wrap
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> sh) ^ c[3] ^ np.uint64(k1),
             p0 & lo]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [x.astype(np.uint32) for x in c]


def blocks(seed, stream, first_block, n):
    """blocks first_block .. first_block + n - 1 of a stream -> 16 n bytes
    (a uint8 array)"""
    b = (np.arange(n, dtype=np.uint64) + np.uint64(first_block)) if n else np.zeros(0, np.uint64)
    ctr = (b & np.uint64(MASK), b >> np.uint64(32),
           np.full(n, stream & MASK, dtype=np.uint64), np.full(n, (stream >> 32) & MASK,
                                                               dtype=np.uint64))
    words = philox(ctr, (seed & MASK, (seed >> 32) & MASK))
    return np.stack(words, axis=1).astype("<u4").view(np.uint8).reshape(-1)


def stream_bytes(seed, stream, n, first_byte=0):
    """bytes first_byte .. first_byte + n - 1 of a stream, as bytes"""
    if n <= 0:
        return b""
    b0, b1 = first_byte // 16, (first_byte + n - 1) // 16
    data = blocks(seed, stream, b0, b1 - b0 + 1)
    at = first_byte - 16 * b0
    return data[at:at + n].tobytes()
