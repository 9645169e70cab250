"""Hasher tables for the tests of custom hashers (tests/test_hashers_cpu.py, tests/test_gpu_hashers.py and the text
twin tests/test_gpu_text_hashers.py): named table families from a seed, and a case as both the product's
``sm.Hasher`` / ``sm.TextHasher`` and the oracle's ``Hasher`` with ``kind = 0``.

  random   independent 32-bit values; rc is not derived from fw
  paired   rc[c] = fw[c ^ 2], NtHasher's shape
  const    all fw equal and all rc equal: every key ties, every window emits
  two      fw = [a, a, b, b], rc = [c, d, c, d]: frequent ties
  low16    entries differ only in their low 16 bits: with rot 0 or 16 every masked forward key ties, otherwise the
           keys depend on how far bits rotate into the upper half
  zero_rc  rc all zero (with a canonical hasher the sum is the forward hash alone)

The rot values include 0 and 16 (the two-step warm-up rotates by 2 * rot), 15 / 17 around it, and 39, which the
product and the oracle both reduce modulo 32 to 7.
"""
from __future__ import annotations

import numpy as np

FAMILIES = ("random", "paired", "const", "two", "low16", "zero_rc")
ROTS = (0, 1, 7, 15, 16, 17, 31, 39)
TEXT_FAMILIES = ("const", "two", "low16", "random")
TEXT_ROTS = (0, 16, 17, 31)


def tables(family: str, seed: int, size: int = 4) -> tuple[list, list]:
    """(fw[size], rc[size]) of a family; ``size`` is 4 (2-bit codes) or 256 (byte text)."""
    rng = np.random.default_rng([seed, FAMILIES.index(family), size])
    r32 = lambda n: [int(x) for x in rng.integers(0, 1 << 32, size=n, dtype=np.uint64)]
    idx = range(size)
    if family == "random":
        return r32(size), r32(size)
    if family == "paired":
        fw = r32(size)
        return fw, [fw[c ^ 2] for c in idx]
    if family == "const":
        a, b = r32(2)
        return [a] * size, [b] * size
    if family == "two":
        a, b, c_, d = r32(4)
        return [b if (c >> 1) & 1 else a for c in idx], [d if c & 1 else c_ for c in idx]
    if family == "low16":
        hf, hr = (x & 0xFFFF0000 for x in r32(2))
        return [hf | (x & 0xFFFF) for x in r32(size)], [hr | (x & 0xFFFF) for x in r32(size)]
    if family == "zero_rc":
        return r32(size), [0] * size
    raise KeyError(family)


def const_emits_every_window(w: int, canonical_windows: bool) -> bool:
    """With a ``const`` table every key ties: forward window i selects i (leftmost), a canonical window i selects i or
    i + w - 1 by its strand vote.  Neighbouring windows then select different positions - one output per window, which
    overflows lists sized for a random hasher's density - except at canonical w = 2, where window i's rightmost k-mer
    IS window i + 1's leftmost one and the two may select the same position."""
    return not (canonical_windows and w == 2)


class Case:
    """One hasher: tables of a family, rot, strand, xor terms."""

    def __init__(self, family, rot, canonical, seed=1, xor=False, size=4):
        self.family, self.rot, self.canonical, self.seed, self.size = family, int(rot), bool(canonical), seed, size
        self.fw, self.rc = tables(family, seed, size)
        self.fw_xor = self.rc_xor = 0
        if xor:
            rng = np.random.default_rng([seed, 99, FAMILIES.index(family), self.rot])
            self.fw_xor, self.rc_xor = (int(x) for x in rng.integers(1, 1 << 32, size=2, dtype=np.uint64))

    def __repr__(self):
        return (f"Case({self.family}, rot={self.rot}, canonical={self.canonical}, seed={self.seed}, "
                f"xor=({self.fw_xor:#x}, {self.rc_xor:#x}), size={self.size})")

    def with_rot(self, rot) -> "Case":
        c = Case(self.family, rot, self.canonical, self.seed, False, self.size)
        c.fw_xor, c.rc_xor = self.fw_xor, self.rc_xor
        return c

    def product(self, sm):
        """``sm.Hasher`` (4 entries) or ``sm.TextHasher`` (256)."""
        cls = sm.Hasher if self.size == 4 else sm.TextHasher
        return cls.from_tables(self.fw, self.rc, self.rot, self.canonical, fw_xor=self.fw_xor, rc_xor=self.rc_xor)

    def oracle(self, oracle):
        """``oracle.Hasher`` with ``kind = 0`` (4-entry cases only)."""
        assert self.size == 4
        h = oracle.Hasher()
        for i in range(4):
            h.fw[i], h.rc[i] = self.fw[i], self.rc[i]
        h.rot, h.canonical, h.fw_xor, h.rc_xor, h.kind = self.rot, int(self.canonical), self.fw_xor, self.rc_xor, 0
        return h


def nth(i: int, canonical, seed=1, size=4, families=FAMILIES, rots=ROTS) -> Case:
    """Case ``i`` of the rotation the GPU tests draw their hashers from: family and rot advance together, and the rot
    shifts by one after every common period, so that ``len(rots)`` consecutive cases within a period hold every family
    and every rot, and a long run every (family, rot) pair.  The xor terms are non-zero in every second pair of cases.
    ``canonical``: the hasher's strand (None: alternate)."""
    nf, nr = len(families), len(rots)
    period = int(np.lcm(nf, nr))
    canon = bool(i & 1) if canonical is None else canonical
    return Case(families[i % nf], rots[(i + i // period) % nr], canon, seed + i // period, xor=bool((i // 2) & 1),
                size=size)


def rotation(canonical, seed=1, size=4, families=FAMILIES, rots=ROTS):
    """``nth(0), nth(1), ...`` without end."""
    i = 0
    while True:
        yield nth(i, canonical, seed, size, families, rots)
        i += 1


class Draw:
    """A counter over ``nth``: ``draw(canonical)`` is the next case of the rotation with the strand the plan needs."""

    def __init__(self, seed=1, size=4, families=FAMILIES, rots=ROTS, start=0):
        self.i, self.kw = start, dict(seed=seed, size=size, families=families, rots=rots)

    def __call__(self, canonical) -> Case:
        c = nth(self.i, canonical, **self.kw)
        self.i += 1
        return c


class Tally:
    """Which families and rot values a test function actually ran through the path it is about."""

    def __init__(self, families=FAMILIES, rots=ROTS):
        self.families, self.rots = set(families), set(rots)
        self.seen_f, self.seen_r = set(), set()
        self.cases = self.bases = self.positions = 0

    def add(self, case: Case, bases: int, positions: int):
        self.seen_f.add(case.family)
        self.seen_r.add(case.rot)
        self.cases += 1
        self.bases += int(bases)
        self.positions += int(positions)

    def check(self, what: str):
        print(f"hasher tally [{what}]: {self.cases} cases, {self.bases} bases, {self.positions} positions")
        assert self.seen_f == self.families, (what, "families never run", self.families - self.seen_f)
        assert self.seen_r == self.rots, (what, "rot values never run", self.rots - self.seen_r)
