"""One minimizer per record with the counts read on the device (mm_one_minimizer_*_counts_device_async): what needs no
GPU - the exports, the refusals in their stated order, the function that turns {counts, bounds} into (n, limit, refused)
(mm_debug_one_minimizer_counts_view), the per-tile function run on the host with that view against the oracle, and the
header under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import one_minimizer_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mm_one_minimizer_text_batch_counts_device_async", "mm_one_minimizer_reads_counts_device_async")
DEBUG = ("mm_debug_one_minimizer_counts_view", "mm_debug_one_minimizer_text_batch_counts",
         "mm_debug_one_minimizer_reads_counts")
EXTRA = 37  # max_records = n + EXTRA


def test_entry_points_exported_and_wrapped(sm):
    L = sm.lib()
    for name in ENTRIES + DEBUG:
        assert hasattr(L, name), name
        assert name in sm.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    for name in ("one_minimizer_text_batch_counts_device", "one_minimizer_reads_counts_device",
                 "debug_one_minimizer_counts_view", "debug_one_minimizer_text_batch_counts",
                 "debug_one_minimizer_reads_counts"):
        assert callable(getattr(sm, name)), name


def test_refusals_in_their_order_need_no_device(sm):
    """MM_ERR_NULL (d_counts included), MM_ERR_K_ZERO, [max_records == 0: MM_OK], MM_ERR_LEN_TOO_LARGE, MM_ERR_CAPACITY:
    every argument wrong at once, one fix at a time.  The workspace is a fake pointer: no refusal dereferences it."""
    L, E = sm.lib(), sm.ERR
    fake = C.c_void_p(4096)  # (never dereferenced: the refusals come first)
    th, hp = sm.TextMulHasher(7, False), sm.NtHasher(21, False)
    big, rec_big = 1 << 32, 1 << 31

    def text(ws, h, k, tx, nb, mc, mr, st, cn, o):
        return L.mm_one_minimizer_text_batch_counts_device_async(ws, C.byref(h) if h is not None else None, k, tx, nb, mc, mr,
                                                                 st, cn, o)

    assert text(None, None, 0, None, 16, big, rec_big, None, None, None) == E["NULL"]
    assert text(fake, None, 0, None, 16, big, rec_big, None, None, None) == E["NULL"]
    assert text(fake, th, 0, None, 16, big, rec_big, None, None, None) == E["NULL"]  # (d_counts)
    assert text(fake, th, 0, None, 16, big, rec_big, None, fake, None) == E["NULL"]  # (the starts)
    assert text(fake, th, 0, None, 16, big, rec_big, fake, fake, None) == E["NULL"]  # (the output)
    assert text(fake, th, 0, None, 16, big, rec_big, fake, fake, fake) == E["NULL"]  # (the text, max_chars > 0)
    assert text(fake, th, 0, fake, 16, big, rec_big, fake, fake, fake) == E["K_ZERO"]
    assert text(fake, th, 7, fake, 16, big, rec_big, fake, fake, fake) == E["LEN_TOO_LARGE"]
    assert text(fake, th, 7, fake, 16, big - 1, rec_big, fake, fake, fake) == E["LEN_TOO_LARGE"]  # (max_records alone)
    assert text(fake, th, 7, fake, 16, big - 1, rec_big - 1, fake, fake, fake) == E["CAPACITY"]  # (max_chars > text_bytes)
    assert text(fake, th, 7, fake, 16, 17, 4, fake, fake, fake) == E["CAPACITY"]
    # no records can come: MM_OK with nothing launched (d_counts is still required)
    assert text(fake, th, 7, fake, 16, 17, 0, None, fake, None) == 0
    assert text(fake, th, 7, fake, 16, 17, 0, None, None, None) == E["NULL"]
    assert text(fake, th, 0, fake, 16, 17, 0, None, fake, None) == E["K_ZERO"]

    def reads(ws, h, k, pk, nb, bo, mb, mr, st, cn, o):
        return L.mm_one_minimizer_reads_counts_device_async(ws, C.byref(h) if h is not None else None, k, pk, nb, bo, mb, mr,
                                                            st, cn, o)

    assert reads(None, None, 0, None, 16, 65, big, rec_big, None, None, None) == E["NULL"]
    assert reads(fake, None, 0, None, 16, 65, big, rec_big, None, None, None) == E["NULL"]
    assert reads(fake, hp, 0, None, 16, 65, big, rec_big, None, None, None) == E["NULL"]  # (d_counts)
    assert reads(fake, hp, 0, None, 16, 65, big, rec_big, None, fake, None) == E["NULL"]
    assert reads(fake, hp, 0, None, 16, 65, big, rec_big, fake, fake, None) == E["NULL"]
    assert reads(fake, hp, 0, None, 16, 65, big, rec_big, fake, fake, fake) == E["NULL"]
    assert reads(fake, hp, 0, fake, 16, 65, big, rec_big, fake, fake, fake) == E["K_ZERO"]
    assert reads(fake, hp, 21, fake, 16, 65, big, rec_big, fake, fake, fake) == E["LEN_TOO_LARGE"]
    assert reads(fake, hp, 21, fake, 16, 65, 64, rec_big, fake, fake, fake) == E["LEN_TOO_LARGE"]
    assert reads(fake, hp, 21, fake, 16, 65, 64, 4, fake, fake, fake) == E["CAPACITY"]  # (base_offset past the buffer)
    assert reads(fake, hp, 21, fake, 16, 1, 64, 4, fake, fake, fake) == E["CAPACITY"]  # (1 + 64 > 64 bases)
    assert reads(fake, hp, 21, fake, 16, 1, 64, 0, None, fake, None) == 0
    # the host-side entries: the same checks minus the workspace
    packed = np.zeros(16, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint32)
    st = np.array([0, 7, 16, 16, 16], dtype=np.uint64)
    cn = np.array([16, 2], dtype=np.uint64)
    p8, p32, ps, pc = (C.c_void_p(a.ctypes.data) for a in (packed, out, st, cn))
    dtext = lambda h, k, tx, nb, mc, mr, s, c, o: L.mm_debug_one_minimizer_text_batch_counts(
        C.byref(h) if h is not None else None, k, tx, nb, mc, mr, s, c, 0, o)
    assert dtext(None, 0, None, 16, big, rec_big, None, None, None) == E["NULL"]
    assert dtext(th, 0, None, 16, big, rec_big, None, None, None) == E["NULL"]
    assert dtext(th, 0, None, 16, big, rec_big, ps, pc, p32) == E["NULL"]
    assert dtext(th, 0, p8, 16, big, rec_big, ps, pc, p32) == E["K_ZERO"]
    assert dtext(th, 7, p8, 16, big, rec_big, ps, pc, p32) == E["LEN_TOO_LARGE"]
    assert dtext(th, 7, p8, 16, 17, 4, ps, pc, p32) == E["CAPACITY"]
    assert dtext(th, 7, p8, 16, 16, 0, None, pc, None) == 0
    assert dtext(th, 7, p8, 16, 16, 4, ps, pc, p32) == 0
    assert out[0] == oc.expect_text(packed, st[:3], 7, th)[0] and (out[2:4] == oc.NO_MINIMIZER).all()
    dreads = lambda h, k, pk, nb, bo, mb, mr, s, c, o: L.mm_debug_one_minimizer_reads_counts(
        C.byref(h) if h is not None else None, k, pk, nb, bo, mb, mr, s, c, 0, o)
    assert dreads(hp, 0, p8, 16, 65, big, rec_big, ps, None, p32) == E["NULL"]
    assert dreads(hp, 0, p8, 16, 65, big, rec_big, ps, pc, p32) == E["K_ZERO"]
    assert dreads(hp, 21, p8, 16, 65, big, rec_big, ps, pc, p32) == E["LEN_TOO_LARGE"]
    assert dreads(hp, 21, p8, 16, 65, 64, 4, ps, pc, p32) == E["CAPACITY"]
    assert dreads(hp, 21, p8, 16, 1, 64, 4, ps, pc, p32) == E["CAPACITY"]
    assert dreads(hp, 21, p8, 16, 1, 63, 4, ps, pc, p32) == 0


def test_counts_view(sm):
    """Counts at, below and beyond each bound, zero records, n_sym below starts[n]."""
    view = sm.debug_one_minimizer_counts_view
    starts = np.array([5, 5, 40, 100, 100, 260], dtype=np.uint64)
    # (max_sym, max_records, n_sym, n) -> (n, limit, refused)
    assert view(300, 9, 260, 5, starts) == (5, 260, False)      # below both bounds
    assert view(260, 5, 260, 5, starts) == (5, 260, False)      # at both bounds
    assert view(300, 9, 300, 5, starts) == (5, 260, False)      # the records end before the symbols do
    assert view(300, 9, 259, 5, starts) == (5, 259, False)      # n_sym below starts[n]: the limit is n_sym
    assert view(300, 9, 99, 3, starts) == (3, 99, False)
    assert view(300, 9, 260, 3, starts) == (3, 100, False)      # fewer records than the starts hold
    assert view(300, 9, 260, 1, starts) == (1, 5, False)        # one empty record
    assert view(300, 9, 0, 5, starts) == (5, 0, False)          # no symbols at all
    assert view(300, 9, 4, 5, starts) == (5, 4, False)          # n_sym below starts[0]
    assert view(300, 9, 260, 0, starts) == (0, 0, False)        # zero records
    assert view(300, 9, 260, 0, None) == (0, 0, False)          # (... read no start)
    assert view(300, 0, 260, 0, None) == (0, 0, False)
    assert view(0, 9, 0, 0, None) == (0, 0, False)
    # beyond a bound: refused, n = limit = 0, and no start is read (None would crash)
    assert view(259, 9, 260, 5, None) == (0, 0, True)
    assert view(300, 4, 260, 5, None) == (0, 0, True)
    assert view(259, 4, 260, 5, None) == (0, 0, True)
    assert view(300, 9, (1 << 64) - 1, (1 << 64) - 1, None) == (0, 0, True)
    assert view(0, 0, 0, 1, None) == (0, 0, True)
    assert view(0, 0, 1, 0, None) == (0, 0, True)
    # a view that reads a start needs the starts
    assert sm.lib().mm_debug_one_minimizer_counts_view(300, 9, 260, 5, None, C.c_void_p(np.zeros(3, np.uint64).ctypes.data)) \
        == sm.ERR["NULL"]


def _padded(starts, extra, junk):
    """max_records + 1 starts: the words behind starts[n] hold ``junk`` (the kernels must not look at them)."""
    return np.concatenate([starts, np.full(extra, junk, dtype=np.uint64)])


@pytest.mark.parametrize("k", (1, 7, 31))
@pytest.mark.parametrize("tile", (16, 64))
def test_debug_text_counts_equal_the_checker(sm, k, tile):
    T = sm.one_minimizer_tile()
    lens = oc.shape_lengths(T, k, 40)
    text, starts = oc.text_records(lens, 50 + k, 3)
    n = len(lens)
    for hp in (sm.TextMulHasher(k, False), sm.TextMulHasher(k, True)):
        want = oc.expect_text(text, starts, k, hp)
        for junk in (0, (1 << 64) - 1):
            got = sm.debug_one_minimizer_text_batch_counts(hp, k, text, _padded(starts, EXTRA, junk), (int(starts[-1]), n),
                                                           tile=tile)
            assert len(got) == n + EXTRA
            assert np.array_equal(got[:n], want), np.nonzero(got[:n] != want)[0][:8]
            assert (got[n:] == oc.NO_MINIMIZER).all()
        # the host-n entry on the same records: bit for bit
        assert np.array_equal(sm.debug_one_minimizer_text_batch(hp, k, text, starts, tile=tile), want)
        # fewer records than were loaded: the first m, as the host-n call gives them for n_records = m
        m = 9
        got = sm.debug_one_minimizer_text_batch_counts(hp, k, text, _padded(starts, EXTRA, 0), (int(starts[-1]), m), tile=tile)
        assert np.array_equal(got[:m], want[:m]) and (got[m:] == oc.NO_MINIMIZER).all()
        # n_sym inside the last record: its k-mers that end below n_sym only
        cut = int(starts[-1]) - 150 + k + 2
        cut_starts = starts.copy()
        cut_starts[-1] = cut
        got = sm.debug_one_minimizer_text_batch_counts(hp, k, text, _padded(starts, EXTRA, 0), (cut, n), tile=tile)
        assert np.array_equal(got[:n], oc.expect_text(text, cut_starts, k, hp)) and (got[n:] == oc.NO_MINIMIZER).all()
        # counts {0, 0} and counts beyond each bound: "none" everywhere
        for counts, refused in (((0, 0), False), ((len(text) + 1, n), True), ((int(starts[-1]), n + EXTRA + 1), True)):
            got = sm.debug_one_minimizer_text_batch_counts(hp, k, text, _padded(starts, EXTRA, 0), counts, tile=tile,
                                                           refused_ok=True)
            assert (got == oc.NO_MINIMIZER).all(), counts
            if refused:
                with pytest.raises(sm.MinimizerError) as e:
                    sm.debug_one_minimizer_text_batch_counts(hp, k, text, _padded(starts, EXTRA, 0), counts, tile=tile)
                assert e.value.code == sm.ERR["CAPACITY"]


@pytest.mark.parametrize("k", (1, 7, 31))
@pytest.mark.parametrize("tile", (16, 64))
def test_debug_reads_counts_equal_the_oracle(sm, oracle, k, tile):
    T = sm.one_minimizer_tile()
    lens = oc.shape_lengths(T, k, 40)
    n = len(lens)
    for bo, canonical in ((0, False), (3, True)):
        packed, starts, _ = oc.packed_records(lens, 100 * k + bo, bo, 5 + bo)
        hp = sm.NtHasher(k, canonical)
        want = oc.expect_packed(oracle, packed, starts, k, oracle.default_hasher(canonical), bo)
        for junk in (0, (1 << 64) - 1):
            got = sm.debug_one_minimizer_reads_counts(hp, k, packed, _padded(starts, EXTRA, junk), (int(starts[-1]), n),
                                                      base_offset=bo, tile=tile)
            assert len(got) == n + EXTRA
            assert np.array_equal(got[:n], want), np.nonzero(got[:n] != want)[0][:8]
            assert (got[n:] == oc.NO_MINIMIZER).all()
        assert np.array_equal(sm.debug_one_minimizer_reads(hp, k, packed, n, starts, base_offset=bo, tile=tile), want)
        m = 9
        got = sm.debug_one_minimizer_reads_counts(hp, k, packed, _padded(starts, EXTRA, 0), (int(starts[-1]), m),
                                                  base_offset=bo, tile=tile)
        assert np.array_equal(got[:m], want[:m]) and (got[m:] == oc.NO_MINIMIZER).all()
        max_bases = 4 * len(packed) - bo
        for counts, refused in (((0, 0), False), ((max_bases + 1, n), True), ((int(starts[-1]), n + EXTRA + 1), True)):
            got = sm.debug_one_minimizer_reads_counts(hp, k, packed, _padded(starts, EXTRA, 0), counts, base_offset=bo,
                                                      tile=tile, refused_ok=True)
            assert (got == oc.NO_MINIMIZER).all(), counts
            if refused:
                with pytest.raises(sm.MinimizerError) as e:
                    sm.debug_one_minimizer_reads_counts(hp, k, packed, _padded(starts, EXTRA, 0), counts, base_offset=bo,
                                                        tile=tile)
                assert e.value.code == sm.ERR["CAPACITY"]


def test_counts_header_under_sanitizers(tmp_path):
    """tests/cxx/one_minimizer_counts_check.cpp: mm_one_min.h's counts view and per-tile logic in a stand-alone host
    program (its own main) built with -fsanitize=address,undefined and run directly; nothing is preloaded and nothing is
    loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: the counts header cannot be checked"
    exe = tmp_path / "one_minimizer_counts_check"
    inc = os.path.join(ROOT, "simd-minimizers_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc,
                    "-o", str(exe), os.path.join(ROOT, "tests", "cxx", "one_minimizer_counts_check.cpp")], check=True,
                   capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "records ok" in r.stdout and "refused views" in r.stdout
