"""Inputs and expected values shared by the one-minimizer tests (tests/test_one_minimizer_cpu.py,
tests/test_gpu_one_minimizer.py).  Expected values come from the oracle (packed) or from tests/text_checker.py (text),
never from the code under test:

    expect(r) = argmin(hash_kmers(record r) & 0xffff0000)    np.argmin takes the first = the leftmost
                NO_MINIMIZER when len_r < k
"""
from __future__ import annotations

import numpy as np

import text_checker

NO_MINIMIZER = 0xFFFFFFFF
KS = (1, 5, 21, 31, 32, 33, 64, 65, 200)
TEXT_KS = (1, 7, 21, 33)


def shape_lengths(T: int, k: int, tail: int = 500) -> list:
    """Records that end exactly on a tile edge, k-mers that straddle one, runs of empty and too-short records inside a
    tile and at the start of one, then ``tail`` reads of 150."""
    return [T - 1, T, T + 1, T + k - 1, T + k, k - 1, k, 0, 0, 0, 1, 2 * T] + [150] * tail


def packed_records(lengths, seed: int, base_offset: int = 0, first_start: int = 0):
    """(packed bytes, starts[n + 1], codes): random bases, ``first_start`` junk bases in front of record 0 and
    ``base_offset`` in front of those, a few junk bases behind the last record."""
    rng = np.random.default_rng(seed)
    total = int(np.sum(lengths))
    codes = rng.integers(0, 4, size=base_offset + first_start + total + 5, dtype=np.uint8)
    starts = np.zeros(len(lengths) + 1, dtype=np.uint64)
    starts[0] = first_start
    starts[1:] = first_start + np.cumsum(np.asarray(lengths, dtype=np.uint64), dtype=np.uint64)
    return text_checker.pack_codes(codes), starts, codes


def expect_packed(oracle, packed, starts, k: int, hasher, base_offset: int = 0, lens=None) -> np.ndarray:
    """``lens``: the records' lengths when they are not ``starts[r + 1] - starts[r]`` (fixed-stride layouts)."""
    n = len(starts) - 1 if lens is None else len(lens)
    out = np.full(n, NO_MINIMIZER, dtype=np.uint32)
    for r in range(n):
        ln = int(starts[r + 1] - starts[r]) if lens is None else int(lens[r])
        if ln >= k:
            h = oracle.hash_kmers(packed, ln, k, hasher, base_offset=base_offset + int(starts[r]))[: ln - k + 1]
            out[r] = int(np.argmin(h & np.uint32(0xFFFF0000)))
    return out


def expect_windows(oracle, packed, starts, k: int, hasher, base_offset: int = 0) -> np.ndarray:
    """The second, independent route: a minimizer run with the single window w = len - k + 1."""
    n = len(starts) - 1
    out = np.full(n, NO_MINIMIZER, dtype=np.uint32)
    for r in range(n):
        ln = int(starts[r + 1] - starts[r])
        if ln >= k:
            p = oracle.window_positions(packed, ln, k, ln - k + 1, hasher, False, base_offset=base_offset + int(starts[r]))
            assert len(p) == 1
            out[r] = int(p[0])
    return out


def text_records(lengths, seed: int, first_start: int = 0, alphabet: int = 256):
    """(text bytes, starts[n + 1]): bytes over ``alphabet`` values, junk in front of record 0 and behind the last."""
    rng = np.random.default_rng(seed)
    total = int(np.sum(lengths))
    text = rng.integers(0, alphabet, size=first_start + total + 3, dtype=np.uint8)
    starts = np.zeros(len(lengths) + 1, dtype=np.uint64)
    starts[0] = first_start
    starts[1:] = first_start + np.cumsum(np.asarray(lengths, dtype=np.uint64), dtype=np.uint64)
    return text, starts


def expect_text(text, starts, k: int, hasher) -> np.ndarray:
    n = len(starts) - 1
    out = np.full(n, NO_MINIMIZER, dtype=np.uint32)
    for r in range(n):
        b, e = int(starts[r]), int(starts[r + 1])
        if e - b >= k:
            h = text_checker.hashes(text[b:e], k, hasher)
            out[r] = int(np.argmin(h & np.uint32(0xFFFF0000)))
    return out
