"""CPU-only test of the numpy Philox-4x32-10 (``philox_ref.py``) that the GPU tests of the device deviates compare against:
the known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10)."""

import numpy as np
import pytest

import philox_ref

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_known_answer_vectors(counter, key, want):
    got = philox_ref.philox4x32(np.array(counter, dtype=np.uint64), *key)
    assert [int(w) for w in got] == list(want)


def test_blocks_broadcast_and_take_the_seed_as_the_key():
    """an array of counters gives the blocks of its rows; the 64-bit seed is (key0, key1) = (low, high) half"""
    counter, key, want = KAT[2]
    seed = key[0] | (key[1] << 32)
    got = philox_ref.block(seed, np.array([counter[0], 0]), np.array([counter[1], 0]), counter[2], counter[3])
    assert got.shape == (2, 4) and [int(w) for w in got[0]] == list(want)
    assert [int(w) for w in got[1]] == [int(w) for w in philox_ref.philox4x32(np.array((0, 0) + counter[2:], dtype=np.uint64), *key)]
