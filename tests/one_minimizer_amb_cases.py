"""Inputs and expected values shared by the skip-ambiguous one-minimizer tests (tests/test_one_minimizer_amb_cpu.py,
tests/test_gpu_one_minimizer_amb.py, tests/test_gpu_fastx_one_minimizer.py).  Expected values come from the oracle's
hashes, never from the code under test:

    a k-mer start p of record r is CLEAN when none of the record's bases p .. p + k - 1 has its ambiguity bit set
    expect(r) = the smallest clean p whose hash_kmers(record r)[p] & 0xffff0000 is minimal over the clean p
                NO_MINIMIZER when record r has no clean p

Bit numbering: symbol i (counted from base_offset, as the starts count) is bit amb_offset + i, bit b = bit b % 8 of byte
b / 8.
"""
from __future__ import annotations

import numpy as np

import one_minimizer_cases as oc

NO_MINIMIZER = oc.NO_MINIMIZER
MASK = np.uint32(0xFFFF0000)
KS = (1, 5, 21, 32, 33, 65)
# (base_offset, amb_offset): base_offset % 4 != amb_offset % 8 in five of the six
OFFSETS = tuple((bo, ao) for bo in (0, 3) for ao in (0, 5, 37))


def pack_bits(mask, amb_offset: int) -> np.ndarray:
    """``mask[i]`` = symbol i is ambiguous -> the bytes of the bits; the ``amb_offset`` bits in front and the bits behind
    the last symbol up to the end of the last byte are SET (junk that must never count)."""
    bits = np.ones((amb_offset + len(mask) + 7) // 8 * 8, dtype=np.uint8)
    bits[amb_offset:amb_offset + len(mask)] = np.asarray(mask, dtype=np.uint8)
    return np.packbits(bits, bitorder="little")


def record_bits(amb, amb_offset: int, start: int, length: int) -> np.ndarray:
    """The record's OWN bits, nothing outside them."""
    b0 = amb_offset + start
    lo, hi = b0 // 8, (b0 + length + 7) // 8
    return np.unpackbits(np.asarray(amb[lo:hi], dtype=np.uint8), bitorder="little")[b0 - 8 * lo:b0 - 8 * lo + length]


def expect_packed_amb(oracle, packed, starts, k: int, hasher, amb, base_offset: int = 0, amb_offset: int = 0, lens=None):
    n = len(starts) - 1 if lens is None else len(lens)
    out = np.full(n, NO_MINIMIZER, dtype=np.uint32)
    for r in range(n):
        s = int(starts[r])
        ln = int(starts[r + 1]) - s if lens is None else int(lens[r])
        if ln < k:
            continue
        h = oracle.hash_kmers(packed, ln, k, hasher, base_offset=base_offset + s)[: ln - k + 1] & MASK
        c = np.concatenate([[0], np.cumsum(record_bits(amb, amb_offset, s, ln), dtype=np.int64)])
        clean = np.nonzero(c[k:] - c[:-k] == 0)[0]  # (p is clean: no set bit among p .. p + k - 1)
        if len(clean):
            out[r] = int(clean[np.argmin(h[clean])])
    return out


def expect_runs(oracle, packed, starts, k: int, hasher, amb, base_offset: int = 0, amb_offset: int = 0, lens=None):
    """The second, independent route: every record cut at its set bits into maximal clean runs, the plain expectation
    (one_minimizer_cases.expect_packed) of each run as a record of its own, the minimum of (masked hash, position)."""
    n = len(starts) - 1 if lens is None else len(lens)
    out = np.full(n, NO_MINIMIZER, dtype=np.uint32)
    for r in range(n):
        s = int(starts[r])
        ln = int(starts[r + 1]) - s if lens is None else int(lens[r])
        bits = record_bits(amb, amb_offset, s, ln)
        edges = np.concatenate([[-1], np.nonzero(bits)[0], [ln]])
        best = None
        for a, b in zip(edges[:-1] + 1, edges[1:]):
            if b - a < k:
                continue
            p = int(oc.expect_packed(oracle, packed, np.array([s + a, s + b], dtype=np.uint64), k, hasher, base_offset)[0])
            h = int(oracle.hash_kmers(packed, k, k, hasher, base_offset=base_offset + s + int(a) + p)[0]) & int(MASK)
            if best is None or (h, int(a) + p) < best:
                best = (h, int(a) + p)
        if best is not None:
            out[r] = best[1]
    return out


def shape_case(oracle, T: int, k: int, hasher, seed: int, base_offset: int, amb_offset: int, tail: int = 40, first_start: int = 7):
    """Records of one_minimizer_cases.shape_lengths(T, k, tail) with ambiguity bits placed BY RULE (T: the tile the
    run will use), plus random bits at density 1 / 200.  Returns (packed, starts, amb, knocked, plain): ``plain`` = the
    plain call's expectation, ``knocked`` = the records whose plain answer had its first base set, so that the result must
    differ from the plain call's."""
    lens = oc.shape_lengths(T, k, tail)
    packed, starts, codes = oc.packed_records(lens, seed, base_offset, first_start)
    n_sym = len(codes) - base_offset
    s = [int(x) for x in starts]
    rng = np.random.default_rng(seed + 1)
    mask = rng.random(n_sym) < 1.0 / 200
    # the tile's seams and a lane's: the bases at global position T - 1, T, T + k - 2 and at 15, 16, 17 of a lane
    for g in (T - 1, T, T + k - 2, 16 * 5 + 15, 16 * 5 + 16, 16 * 5 + 17):
        mask[s[0] + g] = True
    first150 = 12  # (shape_lengths: twelve shaped records, then reads of 150)
    mask[s[first150 + 1] - 1] = True               # the last base of one record
    mask[s[6]] = True                              # the first base of the record after a too-short one (k - 1, then k)
    mask[s[first150 + 1]:s[first150 + 2]] = True   # one record all N
    run_at = 40 if k <= 100 else 0
    for r, run in ((first150 + 2, k), (first150 + 3, k - 1)):  # the only clean run has exactly k bases / k - 1 bases
        mask[s[r]:s[r + 1]] = True
        mask[s[r] + run_at:s[r] + run_at + run] = False
    # the plain call's answer knocked out (from the oracle's plain expectation, not from the code under test)
    plain = oc.expect_packed(oracle, packed, starts, k, hasher, base_offset)
    knocked = [r for r in (0, 3, 11, first150 + 5, first150 + 6) if plain[r] != NO_MINIMIZER]
    for r in knocked:
        mask[s[r] + int(plain[r])] = True
    mask[:s[0]] = True    # every bit in front of record 0 ...
    mask[s[-1]:] = True   # ... and behind the last record
    return packed, starts, pack_bits(mask, amb_offset), knocked, plain
