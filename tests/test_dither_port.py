"""CPU: tests/dither_port.py, the numpy port the GPU dither tests compare
with, against the known answers of Philox4x32-10 and against its own stream
definition (include/atgpu_dither.h)."""
import numpy as np
import pytest

import dither_port as port

KNOWN = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KNOWN, ids=["zeros", "ones", "pi"])
def test_known_answers(counter, key, want):
    got = port.philox(counter, key)
    assert " ".join("%08x" % int(w) for w in got) == want


@pytest.mark.parametrize("counter,key,want", KNOWN, ids=["zeros", "ones", "pi"])
def test_a_block_is_the_words_little_endian(counter, key, want):
    seed = key[0] | key[1] << 32
    stream = counter[2] | counter[3] << 32
    block = counter[0] | counter[1] << 32
    words = np.array([int(w, 16) for w in want.split()], dtype="<u4")
    assert port.blocks(seed, stream, block, 1).tobytes() == words.tobytes()
    assert port.stream_bytes(seed, stream, 16, 16 * block) == words.tobytes()


def test_a_byte_alone_is_the_byte_of_a_long_draw():
    seed, stream = 0x0123456789ABCDEF, 7
    whole = port.stream_bytes(seed, stream, 16 * 300 + 5)
    assert len(whole) == 16 * 300 + 5
    for j in (0, 1, 15, 16, 17, 31, 32, 255, 256, 4095, 4096, 4799, 4804):
        assert port.stream_bytes(seed, stream, 1, j) == whole[j:j + 1], j
    # any slice, and the vectorised draw against one block at a time
    assert port.stream_bytes(seed, stream, 100, 1000) == whole[1000:1100]
    assert b"".join(port.blocks(seed, stream, b, 1).tobytes() for b in range(20)) == whole[:320]


def test_streams_and_seeds_differ():
    a = port.stream_bytes(1, 0, 64)
    assert a != port.stream_bytes(1, 1, 64)
    assert a != port.stream_bytes(2, 0, 64)
    assert a != port.stream_bytes(1 << 32, 0, 64)
    assert port.stream_bytes(1, 1, 64) != port.stream_bytes(1, 1 << 32, 64)


def test_the_counter_carries_at_block_2_32():
    seed, stream = 99, 3
    got = port.blocks(seed, stream, (1 << 32) - 1, 3)
    key = (seed, 0)
    for k, ctr in enumerate([(0xFFFFFFFF, 0, 3, 0), (0, 1, 3, 0), (1, 1, 3, 0)]):
        words = np.array([int(w) for w in port.philox(ctr, key)], dtype="<u4")
        assert got[16 * k:16 * k + 16].tobytes() == words.tobytes(), k
    # byte addressing across the carry
    j = 16 << 32
    assert port.stream_bytes(seed, stream, 20, j - 10) == got[6:26].tobytes()


def test_the_stream_index_carries_into_the_fourth_word():
    words = np.array([int(w) for w in port.philox((5, 0, 0, 1), (7, 9))], dtype="<u4")
    assert port.blocks(7 | 9 << 32, 1 << 32, 5, 1).tobytes() == words.tobytes()
