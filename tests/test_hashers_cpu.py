"""The reference side of the custom-hasher tests (tests/hasher_cases.py): on every table family, rot value and strand
the oracle's definition-level flavour equals its streaming restatement, rot is reduced modulo 32, a constant table
selects one position per window, and the skip-ambiguous walk equals the canonical run on input without ``N`` - so
that a failure of tests/test_gpu_hashers.py points at the GPU."""
import numpy as np
import pytest

import hasher_cases as hc

N = 6000
PLANS = [(1, 1), (5, 7), (21, 11), (31, 19), (32, 5), (33, 4), (64, 2), (65, 3), (100, 12)]


def _flavours(case):
    """(k, w, canonical windows, mode) a hasher can run: canonical windows need a canonical hasher and an odd l."""
    for k, w in PLANS:
        for canon_w in ((False, True) if case.canonical else (False,)):
            if canon_w and (k + w - 1) % 2 == 0:
                continue
            for mode in (0, 1, 2):
                if mode == 2 and w % 2 == 0:
                    continue
                yield k, w, canon_w, mode


@pytest.mark.parametrize("family", hc.FAMILIES)
def test_naive_equals_streaming_on_every_table(oracle, family):
    data = oracle.gen_packed(41, N)
    cases = 0
    for canonical in (False, True):
        by_rot = {}
        for rot in hc.ROTS:
            case = hc.Case(family, rot, canonical, seed=3, xor=rot in (1, 16, 31))
            h = case.oracle(oracle)
            for k, w, canon_w, mode in _flavours(case):
                tag = (case, k, w, canon_w, mode)
                want = oracle.run(data, N, k, w, hasher=h, canonical=canon_w, mode=mode, flavour=oracle.NAIVE)
                got = oracle.run(data, N, k, w, hasher=h, canonical=canon_w, mode=mode, flavour=oracle.STREAMING)
                assert np.array_equal(got, want), tag
                if family == "const" and mode == 0 and hc.const_emits_every_window(w, canon_w):
                    assert len(want) == N - (k + w - 1) + 1, tag
                by_rot[(rot, k, w, canon_w, mode)] = want
                cases += 1
        # rot is reduced modulo 32 (the xor terms of rot 7 and 39 are both zero here)
        for (rot, *rest), want in by_rot.items():
            if rot == 39:
                assert np.array_equal(want, by_rot[(7, *rest)]), (family, canonical, rest)
    assert cases == len(hc.ROTS) * (24 + 24 + 19)


def test_skip_ambiguous_equals_canonical_run_without_n(oracle):
    rng = np.random.default_rng(5)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=N)]
    packed, amb = oracle.pack_ascii_n(a.tobytes())
    assert not amb.any()
    cases = 0
    for family in hc.FAMILIES:
        for rot in hc.ROTS:
            case = hc.Case(family, rot, True, seed=4, xor=rot in (0, 15, 17))
            h = case.oracle(oracle)
            for mode in (0, 1, 2):
                want = oracle.run(packed, N, 21, 11, hasher=h, canonical=True, mode=mode, flavour=oracle.NAIVE)
                got = oracle.run_skip_ambiguous(packed, amb, N, 21, 11, hasher=h, canonical=True, mode=mode)
                assert np.array_equal(got, want), (case, mode)
                cases += 1
    assert cases == 144


def test_rotation_reaches_every_family_and_rot():
    """The rotation the GPU tests draw from: 8 cases hold every family and rot, 48 every pair."""
    it = hc.rotation(None)
    cases = [next(it) for _ in range(48)]
    assert {(c.family, c.rot) for c in cases} == {(f, r) for f in hc.FAMILIES for r in hc.ROTS}
    assert {c.family for c in cases[:8]} == set(hc.FAMILIES) and {c.rot for c in cases[:8]} == set(hc.ROTS)
    assert {bool(c.fw_xor) for c in cases[:8]} == {False, True}
    t = hc.Tally()
    for c in cases[:5]:
        t.add(c, 1, 1)
    with pytest.raises(AssertionError):
        t.check("too few")


def test_from_tables_carries_the_xor_terms(sm, oracle):
    """``Hasher.from_tables(fw_xor=, rc_xor=)``: the product's struct equals the oracle's, field by field."""
    case = hc.Case("random", 39, True, seed=2, xor=True)
    hp, ho = case.product(sm), case.oracle(oracle)
    assert case.fw_xor and case.rc_xor
    assert list(hp.fw) == list(ho.fw) and list(hp.rc) == list(ho.rc)
    assert (hp.rot, hp.canonical, hp.fw_xor, hp.rc_xor, hp.kind) == (39, 1, case.fw_xor, case.rc_xor, 0)
    assert (ho.rot, ho.canonical, ho.fw_xor, ho.rc_xor, ho.kind) == (39, 1, case.fw_xor, case.rc_xor, 0)
    plain = sm.Hasher.from_tables(case.fw, case.rc, 7, False)
    assert (plain.fw_xor, plain.rc_xor, plain.kind) == (0, 0, 0)
    th = hc.Case("two", 16, False, xor=True, size=256).product(sm)
    assert isinstance(th, sm.TextHasher) and th.fw_xor and th.fw[0] == th.fw[1] != th.fw[2]
