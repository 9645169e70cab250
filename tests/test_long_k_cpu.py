"""k above 64 on the CPU: the references that judge the GPU paths at long k (tests/test_gpu_long_k.py,
tests/test_gpu_text_long_k.py) are pinned here first.  The oracle's streaming flavour against its naive one, the numpy
text checker against the oracle's naive flavour, the checker's hash against a per-k-mer loop written out below, and the
plans' acceptance of k = 1024, 1025 and 4097.  The reference's own grid reaches k = 65 and random k up to 99
(src/test.rs:29-33); the values beyond are the limits of this engine's kernels (1024 / 1025) and a k above a tile."""
import numpy as np
import pytest

import text_checker as tc

K_LIST = [64, 65, 96, 97, 99, 128, 255, 1000, 1024, 1025, 4097]
W_LIST = [1, 5, 16, 33]


def _codes(n, seed):
    """Random 2-bit codes with a low-complexity stretch (ties everywhere) and a period-2 one, as in
    tests/test_text_cpu.py::test_checker_equals_oracle_on_code_bytes, scaled to n."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, n, dtype=np.uint8)
    codes[n // 4: n // 4 + n // 8] = 1
    codes[n // 2: n // 2 + n // 8: 2] = 2
    return codes


def _plans(canonical, mode, ks):
    """(k, w) of the sweep: canonical takes k or k + 1 so that l = k + w - 1 is odd (the list holds neighbours, so both
    parities of k stay covered); open syncmers have odd w only."""
    out = []
    for k in ks:
        for w in W_LIST:
            if mode == 2 and w % 2 == 0:
                continue
            kk = k + 1 if canonical and (k + w - 1) % 2 == 0 else k
            out.append((kk, w))
    return out


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_oracle_streaming_equals_naive_at_long_k(oracle, canonical, mode):
    """Positions (and super-k-mer indices of minimizers) of the streaming flavour - the one every GPU test compares
    with - equal the naive flavour's."""
    h = oracle.default_hasher(canonical)
    seen = set()
    for k, w in _plans(canonical, mode, K_LIST):
        n = 10_000 if k >= 4097 else 6_000
        packed = tc.pack_codes(_codes(n, 3 + mode + 10 * canonical + k))
        want = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.NAIVE)
        got = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.STREAMING)
        assert len(want) > 0 and np.array_equal(got, want), (k, w)
        if mode == 0:
            wp, wsk = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.NAIVE, super_kmers=True)
            gp, gsk = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.STREAMING, super_kmers=True)
            assert np.array_equal(gp, wp) and np.array_equal(gsk, wsk), (k, w)
            assert np.array_equal(wp, want), (k, w)
        seen.add(k)
    # (canonical open syncmers: w odd and l odd leave odd k only)
    assert {k % 2 for k in seen} == ({1} if canonical and mode == 2 else {0, 1}) and max(seen) >= 4097


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_checker_equals_oracle_at_long_k(sm, oracle, canonical, mode):
    """text_checker.run on the code bytes 0..3 with fw[c] = nt.fw[c & 3] equals the oracle's naive flavour on the same
    codes packed, k up to 1025 (the first k of the generic text family)."""
    h = oracle.default_hasher(canonical)
    fw, rc = tc.text_tables_from_dna(h)
    th = sm.TextHasher.from_tables(fw, rc, rot=7, canonical=canonical)
    n = 6_000
    for k, w in _plans(canonical, mode, [k for k in K_LIST if k <= 1025]):
        codes = _codes(n, 5 + mode + 10 * canonical + k)
        packed = tc.pack_codes(codes)
        if mode == 0:
            wp, wsk = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.NAIVE, super_kmers=True)
            gp, gsk = tc.run(codes, k, w, th, canonical, mode, super_kmers=True)
            assert len(wp) > 0 and np.array_equal(gp, wp) and np.array_equal(gsk, wsk), (k, w)
        else:
            want = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.NAIVE)
            assert len(want) > 0 and np.array_equal(tc.run(codes, k, w, th, canonical, mode), want), (k, w)


def _rotl(x, r):
    r %= 32
    return ((x << r) | (x >> (32 - r))) & 0xFFFFFFFF


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("rot", [1, 8, 16, 31])
def test_checker_hash_equals_its_definition(sm, rot, canonical):
    """text_checker.hashes with random 256-entry tables and non-zero xor constants against the definition, one k-mer at
    a time in Python integers: the only independent statement of the rot-xor hash at long k for 256-symbol tables.
    k = 100 on 300 bytes; k = 1024 on 1024 + 299 bytes (300 k-mers: 300 bytes would hold none)."""
    rng = np.random.default_rng(40 + rot + canonical)
    fw = [int(v) for v in rng.integers(0, 1 << 32, 256, dtype=np.uint64)]
    rc = [int(v) for v in rng.integers(0, 1 << 32, 256, dtype=np.uint64)]
    fx, rx = int(rng.integers(1, 1 << 32)), int(rng.integers(1, 1 << 32))
    th = sm.TextHasher.from_tables(fw, rc, rot=rot, canonical=canonical, fw_xor=fx, rc_xor=rx)
    for k, n in [(100, 300), (1024, 1024 + 299)]:
        s = [int(c) for c in rng.integers(0, 256, n, dtype=np.uint8)]
        want = []
        for i in range(n - k + 1):
            h_fw, h_rc = fx, rx
            for j in range(k):
                h_fw ^= _rotl(fw[s[i + j]], rot * (k - 1 - j))
                h_rc ^= _rotl(rc[s[i + j]], rot * j)
            want.append((h_fw + h_rc) & 0xFFFFFFFF if canonical else h_fw)
        got = tc.hashes(np.array(s, dtype=np.uint8), k, th)
        assert len(want) == n - k + 1 >= 201 and [int(v) for v in got] == want, (k, rot)


@pytest.mark.parametrize("text", [False, True])
def test_plans_accept_long_k(sm, text):
    """mm_plan_create and mm_plan_create_text have no upper bound on k: every mode and both strands at k = 1024, 1025
    and 4097.  Canonical plans take w = 6 where k is even (l odd); canonical open syncmers of even k do not exist (w odd
    makes l even)."""
    made = 0
    for k in (1024, 1025, 4097):
        for canonical in (False, True):
            for mode in (0, 1, 2):
                w = 6 if canonical and k % 2 == 0 and mode != 2 else 5
                if canonical and (k + w - 1) % 2 == 0:
                    with pytest.raises(sm.MinimizerError) as e:
                        sm.Plan(k, w, canonical, mode, None, text=text)
                    assert e.value.code == sm.ERR["EVEN_L"]
                    continue
                p = sm.Plan(k, w, canonical, mode, None, text=text)
                assert p.h and p.value_len() == (k if mode == 0 else k + w - 1)
                made += 1
    assert made == 17
