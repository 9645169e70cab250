"""The text batch run and values that take their counts from the device (mm_run_text_batch_counts_*,
mm_values_*_text_batch_counts_*), without a GPU: the host twin of the function their kernels call to turn {counts, bounds}
into {real tiles, launched tiles, win_end, refused} (mm_debug_text_counts_view), the exported symbols, and the argument
refusals that need no workspace, in the documented order."""
import ctypes as C
import os
import subprocess

import pytest

TILE = 8192
NEW = ["mm_run_text_batch_counts_device_async", "mm_run_text_batch_counts_device",
       "mm_values_u64_text_batch_counts_device_async", "mm_values_u128_text_batch_counts_device_async",
       "mm_debug_text_counts_view"]


def test_symbols_exported(sm):
    L = sm.lib()
    for name in NEW:
        assert name in sm.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name


@pytest.mark.parametrize("k,w", [(7, 11), (21, 11), (3, 2), (5, 7)])
def test_view_tiles_and_win_end(sm, k, w):
    l = k + w - 1
    for n in [0, l - 1, l, 8191, 8192, 8193, 16384]:
        for max_chars in [n, 5 * TILE]:
            v = sm.text_counts_view(k, w, max_chars, 64, n, 3)
            assert not v["refused"]
            assert v["real_tiles"] == (n + 1 + TILE - 1) // TILE, (n, max_chars)
            assert v["launched_tiles"] == (max_chars + 1 + TILE - 1) // TILE
            assert 1 <= v["real_tiles"] <= v["launched_tiles"]
            assert v["win_end"] == (n - l + 1 if n >= l else 0), (n, max_chars)  # (never wraps)
            # no record at all: the same geometry, nothing refused
            v0 = sm.text_counts_view(k, w, max_chars, 64, n, 0)
            assert not v0["refused"] and v0["real_tiles"] == v["real_tiles"] and v0["win_end"] == v["win_end"]


def test_view_refused_exactly_when_a_count_exceeds_its_bound(sm):
    k, w = 7, 11
    for max_chars in [0, 17, 100, TILE, 5 * TILE]:
        for max_records in [0, 1, 64]:
            for n in [0, max_chars - 1, max_chars, max_chars + 1, max_chars + TILE, (1 << 32) + 5, (1 << 64) - 1]:
                if n < 0:
                    continue
                for r in [0, max_records, max_records + 1, 1 << 31, (1 << 64) - 1]:
                    v = sm.text_counts_view(k, w, max_chars, max_records, n, r)
                    assert v["refused"] == (n > max_chars or r > max_records), (max_chars, max_records, n, r)
                    if v["refused"]:
                        # the workgroup with ticket 0 alone: no window, one real tile
                        assert v["real_tiles"] == 1 and v["win_end"] == 0
                    assert v["real_tiles"] <= v["launched_tiles"]


def test_view_bounds_rule_of_the_entry_points(sm):
    out = (C.c_uint64 * 4)()
    L = sm.lib()
    assert L.mm_debug_text_counts_view(7, 11, 1 << 32, 1, 0, 0, out) == sm.ERR["LEN_TOO_LARGE"]
    assert L.mm_debug_text_counts_view(7, 11, 100, 1 << 31, 0, 0, out) == sm.ERR["LEN_TOO_LARGE"]
    assert L.mm_debug_text_counts_view(7, 11, (1 << 32) - 1, (1 << 31) - 1, 0, 0, out) == 0
    assert L.mm_debug_text_counts_view(7, 11, 100, 1, 0, 0, None) == sm.ERR["NULL"]
    assert L.mm_debug_text_counts_view(7, 0, 100, 1, 0, 0, out) == sm.ERR["W_ZERO"]


def _text_plan(sm, k=7, w=11, mode=0):
    L = sm.lib()
    th = sm.TextMulHasher(canonical=False)
    h = C.c_void_p()
    assert L.mm_plan_create_text(C.byref(h), k, w, 0, mode, C.byref(th)) == 0
    return h


def test_refusals_without_a_workspace_in_the_documented_order(sm):
    """NULL plan, packed plan, bounds too large, d_out_sk with syncmers, NULL arrays, max_chars > text_bytes, NULL text, a
    plan the fused text kernel does not take, NULL workspace: each wins over everything behind it."""
    L, E = sm.lib(), sm.ERR
    out3 = (C.c_uint64 * 3)()
    p = C.c_void_p(64)  # (a non-null pointer that no refusal may look through)
    text_plan = _text_plan(sm)
    sync_plan = _text_plan(sm, mode=1)
    wide_plan = _text_plan(sm, w=129)
    dna = C.c_void_p()
    assert L.mm_plan_create(C.byref(dna), 7, 11, 0, 0, None) == 0
    try:
        def run(plan, text=p, text_bytes=100, max_chars=100, max_records=4, starts=p, counts=p, sk=None, offs=p, ws=None):
            a = (plan, ws, text, text_bytes, max_chars, max_records, starts, counts, None, sk, 0, offs)
            ra = L.mm_run_text_batch_counts_device_async(*a, None)
            rs = L.mm_run_text_batch_counts_device(*a, out3)
            assert ra == rs, (ra, rs)
            return ra

        # every argument wrong at once: the first documented refusal wins, one fix at a time
        bad = dict(text=None, text_bytes=10, max_chars=1 << 32, max_records=1 << 31, starts=None, counts=None, sk=p, offs=None)
        assert run(None, **bad) == E["NULL"]
        assert run(dna, **bad) == E["BAD_MODE"]
        assert run(sync_plan, **bad) == E["LEN_TOO_LARGE"]
        bad.update(max_chars=100)
        assert run(sync_plan, **bad) == E["LEN_TOO_LARGE"]  # (max_records alone)
        bad.update(max_records=4)
        assert run(sync_plan, **bad) == E["BAD_MODE"]       # (d_out_sk with syncmers)
        assert run(text_plan, **bad) == E["NULL"]           # (offsets, starts, counts)
        bad.update(offs=p)
        assert run(text_plan, **bad) == E["NULL"]
        bad.update(starts=p)
        assert run(text_plan, **bad) == E["NULL"]           # (d_counts)
        bad.update(counts=p)
        assert run(text_plan, **bad) == E["CAPACITY"]       # (max_chars 100 > text_bytes 10)
        bad.update(text_bytes=100)
        assert run(text_plan, **bad) == E["NULL"]           # (max_chars > 0 without a text)
        bad.update(text=p)
        assert run(wide_plan, **bad) == E["BAD_MODE"]       # (w = 129: no fused text kernel)
        assert b"mm_run_text_batch_device" in L.mm_last_error()
        assert run(text_plan, **bad) == E["NULL"]           # (the workspace)
        # no record bound needs no starts, no character bound needs no text
        assert run(text_plan, text=None, text_bytes=0, max_chars=0, max_records=0, starts=None) == E["NULL"]  # (workspace)
        assert run(text_plan, max_chars=101) == E["CAPACITY"]
    finally:
        for h in (text_plan, sync_plan, wide_plan, dna):
            L.mm_plan_destroy(h)


def test_values_refusals_without_a_workspace(sm):
    L, E = sm.lib(), sm.ERR
    p = C.c_void_p(64)
    for f in (L.mm_values_u64_text_batch_counts_device_async, L.mm_values_u128_text_batch_counts_device_async):
        # the workspace first, whatever else is wrong
        assert f(None, None, 0, 1 << 32, 1 << 31, None, None, 7, 0, 1, None, None, 5, None) == E["NULL"]
        assert f(None, p, 100, 100, 4, p, p, sm.TEXT_VALUES_BYTES, 7, 0, p, p, 5, p) == E["NULL"]


def test_cxx_text_counts_example_compiles(sm, tmp_path):
    """tests/cxx/text_counts_example.cpp builds against the C header and the in-tree library (it runs on the GPU suite)."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    libdir = os.path.join(root, "simd-minimizers_amd")
    exe = str(tmp_path / "text_counts_example")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(root, "include"), "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", "-o", exe, os.path.join(here, "cxx", "text_counts_example.cpp"),
                    "-L" + libdir, "-lsimd_minimizers_amd", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    assert os.path.exists(exe)
