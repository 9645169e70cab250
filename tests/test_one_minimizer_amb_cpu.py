"""One minimizer per read that skips ambiguous bases (mm_one_minimizer_reads_skip_ambiguous_*): what needs no GPU - the
exports, the return codes, the kernel's per-tile function run on the host (mm_debug_one_minimizer_reads_skip_ambiguous
and its counts form) against two independent expectations built from the oracle's hashes, and the kernel's header under
AddressSanitizer + UBSan in a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import one_minimizer_amb_cases as ac
import one_minimizer_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mm_one_minimizer_reads_skip_ambiguous_device_async", "mm_one_minimizer_reads_skip_ambiguous_counts_device_async",
           "mm_one_minimizer_reads_skip_ambiguous_host")
DEBUG = ("mm_debug_one_minimizer_reads_skip_ambiguous", "mm_debug_one_minimizer_reads_skip_ambiguous_counts")
EXTRA = 37  # max_records = n + EXTRA
SMALL = 64  # the tile override: a record spans many tiles


def test_entry_points_exported_and_wrapped(sm):
    L = sm.lib()
    for name in ENTRIES + DEBUG:
        assert hasattr(L, name), name
        assert name in sm.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name


def both_routes(oracle, packed, starts, k, hasher, amb, bo, ao, lens=None):
    want = ac.expect_packed_amb(oracle, packed, starts, k, hasher, amb, bo, ao, lens)
    second = ac.expect_runs(oracle, packed, starts, k, hasher, amb, bo, ao, lens)
    assert np.array_equal(want, second), np.nonzero(want != second)[0][:8]
    return want


@pytest.mark.parametrize("k", ac.KS)
def test_debug_reads_equal_both_expectations(sm, oracle, k):
    """Bits placed by rule (one_minimizer_amb_cases.shape_case) for the small tile and for the kernel's own, base and bit
    offsets out of step, junk bits set in front of record 0 and behind the last record."""
    T = sm.one_minimizer_tile()
    for i, (bo, ao) in enumerate(ac.OFFSETS):
        canonical = bool(i & 1)
        ho, hp = oracle.default_hasher(canonical), sm.NtHasher(k, canonical)
        for tile in (SMALL, T):
            packed, starts, amb, knocked, plain = ac.shape_case(oracle, tile, k, ho, 900 * k + i, bo, ao)
            n = len(starts) - 1
            want = both_routes(oracle, packed, starts, k, ho, amb, bo, ao)
            got = sm.debug_one_minimizer_reads(hp, k, packed, n, starts, base_offset=bo, tile=tile, amb=amb, amb_offset=ao)
            bad = np.nonzero(got != want)[0]
            assert not len(bad), (k, bo, ao, tile, bad[:8], got[bad[:8]], want[bad[:8]])
            # the rules did what they are for
            assert len(knocked) >= 1 and all(want[r] != plain[r] for r in knocked), (knocked, want[knocked], plain[knocked])
            assert want[13] == oc.NO_MINIMIZER                      # all N
            assert want[14] == (40 if k <= 100 else 0)              # the only clean run has exactly k bases
            assert want[15] == oc.NO_MINIMIZER                      # ... k - 1 bases
            assert want[6] == oc.NO_MINIMIZER                       # k bases, the first one N
            # the counts form at the bounds and with records to spare, junk starts past n
            padded = np.concatenate([starts, np.full(EXTRA, (1 << 64) - 1, dtype=np.uint64)])
            got = sm.debug_one_minimizer_reads_counts(hp, k, packed, padded, (int(starts[-1]), n), base_offset=bo, tile=tile,
                                                      amb=amb, amb_offset=ao)
            assert np.array_equal(got[:n], want) and (got[n:] == oc.NO_MINIMIZER).all()


def test_all_zero_bits_equal_the_plain_call(sm, oracle):
    T = sm.one_minimizer_tile()
    for k in (1, 21, 33):
        lens = oc.shape_lengths(T, k, 40)
        packed, starts, codes = oc.packed_records(lens, 31 + k, 2, 7)
        amb = np.zeros((5 + len(codes)) // 8 + 2, dtype=np.uint8)
        for canonical in (False, True):
            hp = sm.NtHasher(k, canonical)
            plain = sm.debug_one_minimizer_reads(hp, k, packed, len(lens), starts, base_offset=2, tile=SMALL)
            assert np.array_equal(plain, oc.expect_packed(oracle, packed, starts, k, oracle.default_hasher(canonical), 2))
            got = sm.debug_one_minimizer_reads(hp, k, packed, len(lens), starts, base_offset=2, tile=SMALL, amb=amb, amb_offset=5)
            assert np.array_equal(got, plain), (k, canonical)


def test_k_above_the_tile(sm, oracle):
    """k = 200 with tiles of 64 positions: every k-mer spans tiles, a lane's warm-up crosses several."""
    k, bo, ao = 200, 3, 37
    lens = [700, 199, 200, 201, 1000, 0, 450]
    packed, starts, codes = oc.packed_records(lens, 77, bo, 7)
    rng = np.random.default_rng(78)
    mask = rng.random(len(codes) - bo) < 1.0 / 200
    s = [int(x) for x in starts]
    mask[s[2]:s[3]] = False      # 200 clean bases: one k-mer
    mask[s[3] + 100] = True      # 201 bases with an N in the middle: none
    mask[:s[0]] = True
    mask[s[-1]:] = True
    amb = ac.pack_bits(mask, ao)
    for canonical in (False, True):
        ho = oracle.default_hasher(canonical)
        want = both_routes(oracle, packed, starts, k, ho, amb, bo, ao)
        assert want[1] == oc.NO_MINIMIZER and want[2] == 0 and want[3] == oc.NO_MINIMIZER
        got = sm.debug_one_minimizer_reads(sm.NtHasher(k, canonical), k, packed, len(lens), starts, base_offset=bo, tile=SMALL,
                                           amb=amb, amb_offset=ao)
        assert np.array_equal(got, want), np.nonzero(got != want)[0]


def test_more_records_in_a_tile_than_slots(sm, oracle):
    """1500 records of length 2 with k = 2 in one tile: the records past the LDS slots."""
    k, n, T = 2, 1500, sm.one_minimizer_tile()
    assert 2 * n <= T
    packed, starts, codes = oc.packed_records([2] * n, 5, 1, 7)
    rng = np.random.default_rng(6)
    mask = rng.random(len(codes) - 1) < 1.0 / 50
    mask[:7] = True
    mask[int(starts[-1]):] = True
    amb = ac.pack_bits(mask, 5)
    ho = oracle.default_hasher(True)
    want = both_routes(oracle, packed, starts, k, ho, amb, 1, 5)
    assert (want == oc.NO_MINIMIZER).sum() > 10 and (want[1100:] == 0).sum() > 300
    got = sm.debug_one_minimizer_reads(sm.NtHasher(k, True), k, packed, n, starts, base_offset=1, tile=0, amb=amb, amb_offset=5)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


def test_fixed_stride_layouts(sm, oracle):
    n = 300
    for length, stride in ((100, 128), (150, 150)):
        packed, _, codes = oc.packed_records([stride] * n, length, 1, 0)
        fixed = np.arange(n + 1, dtype=np.uint64) * np.uint64(stride)
        rng = np.random.default_rng(length)
        mask = rng.random(len(codes) - 1) < 1.0 / 200
        for r in range(0, n, 7):   # the gap between two reads (or the neighbour's first base) is N: it must not count
            mask[r * stride + length:(r + 1) * stride + 1] = True
        mask[5 * stride:5 * stride + length] = True  # one read all N
        amb = ac.pack_bits(mask, 37)
        for k in (21, length, length + 1):
            for canonical in (False, True):
                ho = oracle.default_hasher(canonical)
                want = both_routes(oracle, packed, fixed, k, ho, amb, 1, 37, lens=[length] * n)
                assert want[5] == oc.NO_MINIMIZER
                got = sm.debug_one_minimizer_reads(sm.NtHasher(k, canonical), k, packed, n, None, stride, length, base_offset=1,
                                                   tile=SMALL, amb=amb, amb_offset=37)
                assert np.array_equal(got, want), (length, stride, k, np.nonzero(got != want)[0][:8])


def test_counts_form(sm, oracle):
    k, bo, ao = 21, 3, 5
    T = sm.one_minimizer_tile()
    ho, hp = oracle.default_hasher(True), sm.NtHasher(k, True)
    packed, starts, amb, _, _ = ac.shape_case(oracle, SMALL, k, ho, 4242, bo, ao)
    n = len(starts) - 1
    want = both_routes(oracle, packed, starts, k, ho, amb, bo, ao)
    for junk in (0, (1 << 64) - 1):
        padded = np.concatenate([starts, np.full(EXTRA, junk, dtype=np.uint64)])
        # counts below the bounds: the first m records, NO_MINIMIZER at and past m
        for m in (9, 20, n):
            got = sm.debug_one_minimizer_reads_counts(hp, k, packed, padded, (int(starts[-1]), m), base_offset=bo, tile=SMALL,
                                                      amb=amb, amb_offset=ao)
            assert len(got) == n + EXTRA
            assert np.array_equal(got[:m], want[:m]) and (got[m:] == oc.NO_MINIMIZER).all(), m
    # counts at the bounds
    max_bases = min(4 * len(packed) - bo, 8 * len(amb) - ao)
    got = sm.debug_one_minimizer_reads_counts(hp, k, packed, starts, (int(starts[-1]), n), max_bases=max_bases, base_offset=bo,
                                              tile=T, amb=amb, amb_offset=ao)
    assert np.array_equal(got, want)
    # counts beyond the bounds: "none" everywhere and MM_ERR_CAPACITY
    padded = np.concatenate([starts, np.zeros(EXTRA, dtype=np.uint64)])
    for counts in ((max_bases + 1, n), (int(starts[-1]), n + EXTRA + 1)):
        got = sm.debug_one_minimizer_reads_counts(hp, k, packed, padded, counts, max_bases=max_bases, base_offset=bo, tile=SMALL,
                                                  refused_ok=True, amb=amb, amb_offset=ao)
        assert (got == oc.NO_MINIMIZER).all(), counts
        with pytest.raises(sm.MinimizerError) as e:
            sm.debug_one_minimizer_reads_counts(hp, k, packed, padded, counts, max_bases=max_bases, base_offset=bo, tile=SMALL,
                                                amb=amb, amb_offset=ao)
        assert e.value.code == sm.ERR["CAPACITY"]


def test_return_codes_need_no_device(sm):
    L, E = sm.lib(), sm.ERR
    fake = C.c_void_p(4096)  # (never dereferenced: the refusals come first)
    hp = sm.NtHasher(21, False)
    packed, amb = np.zeros(16, dtype=np.uint8), np.zeros(8, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint32)
    ok = np.array([0, 30, 64], dtype=np.uint64)
    cn = np.array([64, 2], dtype=np.uint64)
    p8, pa, p32, ps, pc = (C.c_void_p(a.ctypes.data) for a in (packed, amb, out, ok, cn))
    # a NULL workspace first
    assert L.mm_one_minimizer_reads_skip_ambiguous_device_async(None, C.byref(hp), 0, fake, 16, 999, fake, 8, 999, 1, fake, 0, 0,
                                                                fake) == E["NULL"]
    assert L.mm_one_minimizer_reads_skip_ambiguous_host(None, C.byref(hp), 0, fake, 16, 999, fake, 8, 999, 1, fake, 0, 0,
                                                        fake) == E["NULL"]
    reads = lambda k, pk, bo, am, ab, ao, n, st, o: L.mm_debug_one_minimizer_reads_skip_ambiguous(
        C.byref(hp), k, pk, 16, bo, am, ab, ao, n, st, 0, 0, 0, o)
    # NULL amb where a NULL packed buffer is refused: before K_ZERO and the layout
    assert reads(0, p8, 65, None, 8, 65, 2, ps, p32) == E["NULL"]
    assert reads(0, None, 65, pa, 8, 65, 2, ps, p32) == E["NULL"]
    assert reads(0, p8, 65, pa, 8, 65, 2, ps, p32) == E["K_ZERO"]
    assert reads(0, p8, 0, pa, 8, 0, 0, None, None) == E["K_ZERO"]
    assert reads(21, p8, 65, pa, 8, 65, 2, ps, p32) == E["CAPACITY"]  # (base_offset past the buffer)
    assert reads(21, p8, 0, pa, 8, 65, 2, ps, p32) == E["CAPACITY"]   # (amb_offset past the 64 bits)
    assert reads(21, p8, 0, pa, 8, 64, 2, ps, p32) == 0               # (at the end: no bit, no k-mer)
    assert (out[:2] == oc.NO_MINIMIZER).all()
    assert reads(21, p8, 0, None, 8, 0, 0, None, None) == 0           # (n_reads == 0: nothing to do)
    assert reads(21, p8, 0, pa, 8, 0, 2, ps, p32) == 0
    # the counts form: device entry with a fake workspace, and the debug entry
    dev = lambda k, pk, bo, am, ab, ao, mb, mr, st, c, o: L.mm_one_minimizer_reads_skip_ambiguous_counts_device_async(
        fake, C.byref(hp), k, pk, 16, bo, am, ab, ao, mb, mr, st, c, o)
    dbg = lambda k, pk, bo, am, ab, ao, mb, mr, st, c, o: L.mm_debug_one_minimizer_reads_skip_ambiguous_counts(
        C.byref(hp), k, pk, 16, bo, am, ab, ao, mb, mr, st, c, 0, o)
    for f, a, b in ((dev, fake, fake), (dbg, p8, pa)):
        assert f(0, a, 65, None, 8, 65, 64, 2, ps, pc, p32) == E["NULL"]
        assert f(0, a, 65, b, 8, 65, 64, 2, ps, None, p32) == E["NULL"]
        assert f(0, a, 65, b, 8, 65, 64, 2, ps, pc, p32) == E["K_ZERO"]
        assert f(21, a, 65, b, 8, 65, 1 << 32, 2, ps, pc, p32) == E["LEN_TOO_LARGE"]
        assert f(21, a, 65, b, 8, 65, 64, 2, ps, pc, p32) == E["CAPACITY"]
        assert f(21, a, 0, b, 8, 65, 64, 2, ps, pc, p32) == E["CAPACITY"]  # (amb_offset past the bits)
        assert f(21, a, 0, b, 8, 1, 64, 2, ps, pc, p32) == E["CAPACITY"]   # (amb_offset + max_bases = 65 > 64 bits)
        assert f(21, a, 0, b, 8, 1, 64, 0, None, pc, None) == 0            # (no records can come)
    assert dbg(21, p8, 0, pa, 8, 1, 63, 2, ps, np.array([63, 2], np.uint64).ctypes.data_as(C.c_void_p), p32) == 0


def test_amb_header_under_sanitizers(tmp_path):
    """tests/cxx/one_minimizer_amb_check.cpp: mm_one_min.h's ambiguity-aware lane in a stand-alone host program (its own
    main) built with -fsanitize=address,undefined and run directly; nothing is preloaded and nothing is loaded into
    Python."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: the header cannot be checked"
    exe = tmp_path / "one_minimizer_amb_check"
    inc = os.path.join(ROOT, "simd-minimizers_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc,
                    "-o", str(exe), os.path.join(ROOT, "tests", "cxx", "one_minimizer_amb_check.cpp")], check=True,
                   capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "records ok" in r.stdout
