"""The packed reads run that takes its counts from the device (mm_run_packed_reads_counts_*), without a GPU: the host twin of
the function its table kernels call to turn {counts, bounds} into {reads the table is built for, refused}
(mm_debug_lane_counts_view), the exported symbols and their declarations, and the argument refusals that need no workspace,
in the documented order."""
import ctypes as C
import os
import re
import subprocess

NEW = ["mm_run_packed_reads_counts_device_async", "mm_run_packed_reads_counts_device",
       "mm_run_packed_reads_skip_ambiguous_counts_device_async", "mm_run_packed_reads_skip_ambiguous_counts_device",
       "mm_debug_lane_counts_view"]
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_symbols_exported_and_declared(sm):
    L = sm.lib()
    with open(os.path.join(ROOT, "include", "simd_minimizers_amd.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "include", "simd_minimizers_amd.hpp")) as f:
        mirror = f.read()
    for name in NEW:
        assert name in sm.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint %s\(" % name, header), name
    assert "mm_run_packed_reads_counts_device" in mirror
    for name in ("lane_counts_view", "run_packed_reads_counts_device", "fastx_pipeline_device"):
        assert callable(getattr(sm, name)), name


def _restated(max_bases, max_records, n_bases, n_records):
    refused = n_bases > max_bases or n_records > max_records
    return {"n_reads_eff": 0 if refused else n_records, "refused": refused, "lane_bound": max_records + max_bases + 1}


def test_view_against_a_restatement(sm):
    seen_refused = seen_fine = 0
    for max_bases in [0, 1, 150, 8192, (1 << 32) - 1]:
        for max_records in [0, 1, 64, 2048, 2049, (1 << 31) - 1]:
            for n_bases in [0, max_bases - 1, max_bases, max_bases + 1, (1 << 32) + 5, (1 << 64) - 1]:
                if n_bases < 0:
                    continue
                for n_records in [0, max_records - 1, max_records, max_records + 1, (1 << 32) + 5, (1 << 64) - 1]:
                    if n_records < 0:
                        continue
                    v = sm.lane_counts_view(max_bases, max_records, n_bases, n_records)
                    assert v == _restated(max_bases, max_records, n_bases, n_records), (max_bases, max_records, n_bases, n_records)
                    # refused exactly when a count exceeds its bound, and then no read is tabulated
                    assert v["refused"] == (n_bases > max_bases or n_records > max_records)
                    if v["refused"]:
                        assert v["n_reads_eff"] == 0
                        seen_refused += 1
                    else:
                        assert v["n_reads_eff"] == n_records <= max_records
                        seen_fine += 1
    assert seen_refused > 100 and seen_fine > 100


def test_view_bounds_rule_of_the_entry_points(sm):
    """MM_ERR_LEN_TOO_LARGE and MM_ERR_NULL.  (The view takes no window size - the table's reads do not depend on it - so it
    has no MM_ERR_W_ZERO of its own: w == 0 is refused where the plan is created.)"""
    out = (C.c_uint64 * 3)()
    L = sm.lib()
    assert L.mm_debug_lane_counts_view(1 << 32, 1, 0, 0, out) == sm.ERR["LEN_TOO_LARGE"]
    assert L.mm_debug_lane_counts_view(100, 1 << 31, 0, 0, out) == sm.ERR["LEN_TOO_LARGE"]
    assert L.mm_debug_lane_counts_view((1 << 32) - 1, (1 << 31) - 1, 0, 0, out) == 0
    assert L.mm_debug_lane_counts_view(100, 1, 0, 0, None) == sm.ERR["NULL"]
    h = C.c_void_p()
    assert L.mm_plan_create(C.byref(h), 7, 0, 0, 0, None) == sm.ERR["W_ZERO"]


def _plan(sm, k=21, w=11, canonical=0, mode=0):
    h = C.c_void_p()
    assert sm.lib().mm_plan_create(C.byref(h), k, w, canonical, mode, None) == 0
    return h


def test_refusals_without_a_workspace_in_the_documented_order(sm):
    """NULL plan, text plan, bounds too large, d_out_sk with syncmers, a forward plan in the skip-ambiguous form, NULL
    arrays, bounds beyond the packed bytes (or the ambiguity bits), a plan without a lane-table launch, NULL workspace: each
    wins over everything behind it, the same in the asynchronous and the synchronous form."""
    L, E = sm.lib(), sm.ERR
    out3 = (C.c_uint64 * 3)()
    p = C.c_void_p(64)  # (a non-null pointer that no refusal may look through)
    fwd = _plan(sm)
    canon = _plan(sm, canonical=1)
    sync_fwd = _plan(sm, k=15, w=17, mode=1)
    sync_canon = _plan(sm, k=15, w=17, canonical=1, mode=1)
    wide = _plan(sm, w=129)
    wide_canon = _plan(sm, w=129, canonical=1)
    th = sm.TextMulHasher(canonical=False)
    text = C.c_void_p()
    assert L.mm_plan_create_text(C.byref(text), 7, 11, 0, 0, C.byref(th)) == 0
    try:
        def run(plan, packed=p, packed_bytes=100, base_offset=0, max_bases=400, max_records=4, starts=p, counts=p, sk=None,
                offs=p, ws=None):
            a = (plan, ws, packed, packed_bytes, base_offset, max_bases, max_records, starts, counts, None, sk, 0, offs)
            ra = L.mm_run_packed_reads_counts_device_async(*a, None)
            rs = L.mm_run_packed_reads_counts_device(*a, out3)
            assert ra == rs, (ra, rs)
            return ra

        def run_skip(plan, packed=p, packed_bytes=100, base_offset=0, amb=p, amb_bytes=50, amb_offset=0, max_bases=400,
                     max_records=4, starts=p, counts=p, offs=p, ws=None):
            a = (plan, ws, packed, packed_bytes, base_offset, amb, amb_bytes, amb_offset, max_bases, max_records, starts,
                 counts, None, 0, offs)
            ra = L.mm_run_packed_reads_skip_ambiguous_counts_device_async(*a, None)
            rs = L.mm_run_packed_reads_skip_ambiguous_counts_device(*a, out3)
            assert ra == rs, (ra, rs)
            return ra

        # every argument wrong at once: the first documented refusal wins, one fix at a time
        bad = dict(packed=None, packed_bytes=10, max_bases=1 << 32, max_records=1 << 31, starts=None, counts=None, sk=p,
                   offs=None)
        assert run(None, **bad) == E["NULL"]
        assert run(text, **bad) == E["BAD_MODE"]
        assert run(sync_fwd, **bad) == E["LEN_TOO_LARGE"]
        bad.update(max_bases=400)
        assert run(sync_fwd, **bad) == E["LEN_TOO_LARGE"]  # (max_records alone)
        bad.update(max_records=4)
        assert run(sync_fwd, **bad) == E["BAD_MODE"]       # (d_out_sk with syncmers)
        assert run(wide, **bad) == E["NULL"]               # (offsets, starts, counts, packed)
        for fix in ("offs", "starts", "counts"):
            bad.update({fix: p})
            assert run(wide, **bad) == E["NULL"], fix
        bad.update(packed=p)
        assert run(wide, **bad) == E["CAPACITY"]           # (400 bases > 4 * 10 bytes)
        bad.update(packed_bytes=100)
        assert run(wide, **bad) == E["BAD_MODE"]           # (w = 129: no reads-mode kernel, no lane table)
        assert b"mm_run_packed_reads_device" in L.mm_last_error()
        assert run(fwd, **bad) == E["NULL"]                # (the workspace)
        assert run(fwd, base_offset=1) == E["CAPACITY"]    # (base_offset + max_bases beyond 4 * packed_bytes)
        assert run(fwd, max_bases=0, max_records=0) == E["NULL"]  # (no bound at all: still the workspace)

        # the skip-ambiguous form: the same order, the forward plan behind the bounds, the ambiguity bits with the arrays
        sbad = dict(packed=None, packed_bytes=10, amb=None, amb_bytes=4, max_bases=1 << 32, max_records=1 << 31, starts=None,
                    counts=None, offs=None)
        assert run_skip(None, **sbad) == E["NULL"]
        assert run_skip(text, **sbad) == E["BAD_MODE"]
        assert run_skip(sync_fwd, **sbad) == E["LEN_TOO_LARGE"]
        sbad.update(max_bases=400, max_records=4)
        assert run_skip(sync_fwd, **sbad) == E["HASHER_NOT_CANONICAL"]
        assert run_skip(fwd, **sbad) == E["HASHER_NOT_CANONICAL"]
        assert run_skip(wide_canon, **sbad) == E["NULL"]
        for fix in ("offs", "starts", "counts", "packed"):
            sbad.update({fix: p})
            assert run_skip(wide_canon, **sbad) == E["NULL"], fix
        sbad.update(amb=p)
        assert run_skip(wide_canon, **sbad) == E["CAPACITY"]  # (the packed bytes)
        sbad.update(packed_bytes=100)
        assert run_skip(wide_canon, **sbad) == E["CAPACITY"]  # (400 bases > 8 * 4 bytes of ambiguity bits)
        sbad.update(amb_bytes=50)
        assert run_skip(wide_canon, **sbad) == E["BAD_MODE"]
        assert b"mm_run_packed_reads_device" in L.mm_last_error()
        assert run_skip(canon, **sbad) == E["NULL"]           # (the workspace)
        assert run_skip(sync_canon, **sbad) == E["NULL"]
        assert run_skip(canon, amb_offset=1) == E["CAPACITY"]
    finally:
        for h in (fwd, canon, sync_fwd, sync_canon, wide, wide_canon, text):
            L.mm_plan_destroy(h)


def test_lane_table_switched_off_is_refused(sm, monkeypatch):
    """MM_LANE_TABLE=0: the one-lane-per-read launch needs the counts on the host (conftest makes the library read its
    switches at every call)."""
    L, E = sm.lib(), sm.ERR
    p = C.c_void_p(64)
    plan = _plan(sm)
    try:
        a = (plan, None, p, 100, 0, 400, 4, p, p, None, None, 0, p, None)
        assert L.mm_run_packed_reads_counts_device_async(*a) == E["NULL"]
        monkeypatch.setenv("MM_LANE_TABLE", "0")
        assert L.mm_run_packed_reads_counts_device_async(*a) == E["BAD_MODE"]
        assert b"MM_LANE_TABLE" in L.mm_last_error()
        monkeypatch.setenv("MM_LANE_TABLE", "1")
        assert L.mm_run_packed_reads_counts_device_async(*a) == E["NULL"]
    finally:
        L.mm_plan_destroy(plan)


def test_c_reads_counts_example_compiles(sm, tmp_path):
    """tests/cxx/reads_counts_example.cpp is plain C: it builds as C and as C++ against the header and the in-tree library
    (it runs on the GPU suite)."""
    libdir = os.path.join(ROOT, "simd-minimizers_amd")
    src = os.path.join(HERE, "cxx", "reads_counts_example.cpp")
    for cc, lang in (("gcc", "c"), ("g++", "c++")):
        exe = str(tmp_path / ("reads_counts_example_" + lang.replace("+", "x")))
        subprocess.run([cc, "-x", lang, "-O2", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", "-o", exe, src, "-L" + libdir, "-lsimd_minimizers_amd", "-L/opt/rocm/lib",
                        "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
        assert os.path.exists(exe)
