"""One minimizer per record: what needs no GPU - the exports, the refusals in their stated order, the kernel's per-tile
function run on the host (mm_debug_one_minimizer_*) against the oracle, and the kernel's header under AddressSanitizer +
UBSan in a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hasher_cases
import one_minimizer_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mm_one_minimizer_reads_device_async", "mm_one_minimizer_text_batch_device_async", "mm_one_minimizer_reads_host",
           "mm_one_minimizer_text_batch_host")
DEBUG = ("mm_debug_one_minimizer_reads", "mm_debug_one_minimizer_text_batch", "mm_one_minimizer_tile")


def test_entry_points_exported_and_wrapped(sm):
    L = sm.lib()
    for name in ENTRIES + DEBUG:
        assert hasattr(L, name), name
        assert name in sm.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    for name in ("one_minimizer", "one_minimizer_reads_host", "one_minimizer_reads_device", "one_minimizer_text_batch_host",
                 "one_minimizer_text_batch_device", "one_minimizer_tile", "debug_one_minimizer_reads",
                 "debug_one_minimizer_text_batch"):
        assert callable(getattr(sm, name)), name
    assert sm.NO_MINIMIZER == 0xFFFFFFFF
    T = sm.one_minimizer_tile()
    assert T >= 64 and T % 64 == 0  # (whole wavefronts)


def test_refusals_in_their_order_need_no_device(sm):
    """MM_ERR_NULL, then MM_ERR_K_ZERO, then the layout.  The entry points proper refuse a NULL workspace first; the debug
    entry points run the same checks without one."""
    L, E = sm.lib(), sm.ERR
    fake = C.c_void_p(4096)  # (never dereferenced: the refusals come first)
    hp, th = sm.NtHasher(21, False), sm.TextMulHasher(21, False)
    # a NULL workspace: MM_ERR_NULL whatever else is wrong
    assert L.mm_one_minimizer_reads_device_async(None, C.byref(hp), 0, fake, 16, 999, 1, fake, 0, 0, fake) == E["NULL"]
    assert L.mm_one_minimizer_reads_host(None, C.byref(hp), 0, fake, 16, 999, 1, fake, 0, 0, fake) == E["NULL"]
    assert L.mm_one_minimizer_text_batch_device_async(None, C.byref(th), 0, fake, 16, 1, fake, fake) == E["NULL"]
    assert L.mm_one_minimizer_text_batch_host(None, C.byref(th), 0, fake, 16, 1, fake, fake) == E["NULL"]
    packed = np.zeros(16, dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint32)
    p8, p32 = C.c_void_p(packed.ctypes.data), C.c_void_p(out.ctypes.data)
    s64 = lambda *v: np.array(v, dtype=np.uint64)
    reads = lambda h, k, pk, nb, bo, n, st, stride, ln, o: L.mm_debug_one_minimizer_reads(
        C.byref(h) if h is not None else None, k, pk, nb, bo, n, C.c_void_p(st.ctypes.data) if st is not None else None,
        stride, ln, 0, o)
    ok = s64(0, 30, 64)
    # NULL before K_ZERO before the layout
    assert reads(None, 0, p8, 16, 65, 2, ok, 0, 0, p32) == E["NULL"]
    assert reads(hp, 0, p8, 16, 65, 2, ok, 0, 0, None) == E["NULL"]
    assert reads(hp, 0, None, 16, 65, 2, ok, 0, 0, p32) == E["NULL"]
    assert reads(hp, 0, p8, 16, 65, 2, ok, 0, 0, p32) == E["K_ZERO"]
    assert reads(hp, 0, p8, 16, 0, 2, s64(5, 3, 9), 0, 0, p32) == E["K_ZERO"]
    assert reads(hp, 0, p8, 16, 0, 0, None, 0, 0, None) == E["K_ZERO"]
    # the layout
    assert reads(hp, 21, p8, 16, 65, 2, ok, 0, 0, p32) == E["CAPACITY"]  # (base_offset past the buffer)
    assert reads(hp, 21, p8, 16, 1, 2, ok, 0, 0, p32) == E["CAPACITY"]  # (starts[n] = 64 > 63)
    assert reads(hp, 21, p8, 16, 0, 2, s64(5, 3, 9), 0, 0, p32) == E["UNSORTED"]
    assert reads(hp, 21, p8, 16, 0, 2, s64(0, 1, 1 << 32), 0, 0, p32) == E["LEN_TOO_LARGE"]  # (a record of 2^32 - 1)
    assert reads(hp, 21, p8, 16, 0, 1 << 32, ok, 0, 0, p32) == E["LEN_TOO_LARGE"]
    assert reads(hp, 21, p8, 16, 0, 3, None, 22, 22, p32) == E["CAPACITY"]  # (fixed stride: the last read ends at 66)
    assert reads(hp, 21, p8, 16, 0, 3, None, 20, 21, p32) == E["BAD_MODE"]  # (read_len > read_stride)
    assert reads(hp, 21, p8, 16, 0, 0, None, 0, 0, None) == 0  # (no reads: nothing to do)
    assert reads(hp, 21, p8, 16, 0, 2, ok, 0, 0, p32) == 0
    text = lambda h, k, tx, nb, n, st, o: L.mm_debug_one_minimizer_text_batch(
        C.byref(h) if h is not None else None, k, tx, nb, n, C.c_void_p(st.ctypes.data) if st is not None else None, 0, o)
    assert text(None, 0, p8, 16, 2, ok, p32) == E["NULL"]
    assert text(th, 0, p8, 16, 2, None, p32) == E["NULL"]
    assert text(th, 0, p8, 16, 2, ok, p32) == E["K_ZERO"]
    assert text(th, 7, p8, 16, 2, ok, p32) == E["CAPACITY"]  # (starts[n] = 64 > 16 bytes)
    assert text(th, 7, p8, 16, 2, s64(5, 3, 9), p32) == E["UNSORTED"]
    assert text(th, 7, p8, 16, 0, None, None) == 0
    assert text(th, 7, p8, 16, 2, s64(0, 7, 16), p32) == 0


@pytest.mark.parametrize("k", oc.KS)
def test_debug_reads_equal_the_oracle(sm, oracle, k):
    """The kernel's per-tile function on the host for tile overrides 8, 64 and T, base offsets 0-3, starts[0] > 0."""
    T = sm.one_minimizer_tile()
    lens = oc.shape_lengths(T, k, 60)
    for bo in range(4):
        packed, starts, _ = oc.packed_records(lens, 100 * k + bo, bo, 5 + bo)
        for canonical in (False, True):
            want = oc.expect_packed(oracle, packed, starts, k, oracle.default_hasher(canonical), bo)
            for tile in (8, 64, T):
                got = sm.debug_one_minimizer_reads(sm.NtHasher(k, canonical), k, packed, len(lens), starts, base_offset=bo,
                                                   tile=tile)
                bad = np.nonzero(got != want)[0]
                assert not len(bad), (k, bo, canonical, tile, bad[:8], got[bad[:8]], want[bad[:8]])


def test_debug_reads_second_route_and_fixed_stride(sm, oracle):
    lens = [150, 40, 31, 500, 700, 129, 3, 0, 33]
    packed, starts, _ = oc.packed_records(lens, 3, 2, 5)
    for k in (21, 5, 31, 32, 33, 1):
        for canonical in (False, True):
            want = oc.expect_windows(oracle, packed, starts, k, oracle.default_hasher(canonical), 2)
            got = sm.debug_one_minimizer_reads(sm.NtHasher(k, canonical), k, packed, len(lens), starts, base_offset=2, tile=8)
            assert np.array_equal(got, want), (k, canonical)
    n = 300
    for length, stride in ((100, 128), (150, 150)):
        packed, _, _ = oc.packed_records([stride] * n, length, 1, 0)
        fixed = np.arange(n + 1, dtype=np.uint64) * np.uint64(stride)
        for k in (21, length, length + 1):
            want = oc.expect_packed(oracle, packed, fixed, k, oracle.default_hasher(True), 1, lens=[length] * n)
            got = sm.debug_one_minimizer_reads(sm.NtHasher(k, True), k, packed, n, None, stride, length, base_offset=1, tile=64)
            assert np.array_equal(got, want), (length, stride, k)


def test_debug_reads_every_hasher_family(sm, oracle):
    """const and low16 included: where every key ties the answer is position 0."""
    T, k = sm.one_minimizer_tile(), 21
    draw, tally = hasher_cases.Draw(seed=3), hasher_cases.Tally()
    lens = oc.shape_lengths(T, k, 40)
    for i in range(24):
        case = draw(None)
        packed, starts, _ = oc.packed_records(lens, 60 + i, i % 4, i)
        want = oc.expect_packed(oracle, packed, starts, k, case.oracle(oracle), i % 4)
        if case.family == "const" or (case.family == "low16" and case.rot % 32 == 0 and not case.canonical):
            assert (want[np.asarray(lens) >= k] == 0).all(), case
        for tile in (8, 64, T):
            got = sm.debug_one_minimizer_reads(case.product(sm), k, packed, len(lens), starts, base_offset=i % 4, tile=tile)
            assert np.array_equal(got, want), (case, tile)
        tally.add(case, int(starts[-1]), len(lens))
    tally.check("debug_one_minimizer_reads")


@pytest.mark.parametrize("k", oc.TEXT_KS)
def test_debug_text_equals_the_checker(sm, k):
    T = sm.one_minimizer_tile()
    draw = hasher_cases.Draw(seed=2, size=256, families=hasher_cases.TEXT_FAMILIES, rots=hasher_cases.TEXT_ROTS)
    tally = hasher_cases.Tally(hasher_cases.TEXT_FAMILIES, hasher_cases.TEXT_ROTS)
    lens = oc.shape_lengths(T, k, 30)
    text, starts = oc.text_records(lens, 50 + k, 3)
    assert len(np.unique(text)) == 256
    cases = [draw(None) for _ in range(4)]
    for case in cases:
        tally.add(case, int(starts[-1]), len(lens))
    for hp, hc in [(c.product(sm), c) for c in cases] + [(sm.TextMulHasher(k, c),) * 2 for c in (False, True)]:
        want = oc.expect_text(text, starts, k, hc)
        for tile in (8, 64, T):
            got = sm.debug_one_minimizer_text_batch(hp, k, text, starts, tile=tile)
            assert np.array_equal(got, want), (k, tile)
    tally.check("debug_one_minimizer_text_batch")


def test_kernel_header_under_sanitizers(tmp_path):
    """tests/cxx/one_minimizer_check.cpp: mm_one_min.h in a stand-alone host program (its own main) built with
    -fsanitize=address,undefined and run directly; nothing is preloaded and nothing is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "one_minimizer_check"
    inc = os.path.join(ROOT, "simd-minimizers_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc,
                    "-o", str(exe), os.path.join(ROOT, "tests", "cxx", "one_minimizer_check.cpp")], check=True,
                   capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "records ok" in r.stdout
