"""Many records of byte text in one call (mm_run_text_batch_*) on the GPU.  The checker is the single-text path: record r's
slice of the batch equals mm_run_text_host on record r alone (itself pinned to tests/text_checker.py), and text_checker.run
directly where sizes allow."""
import ctypes as C

import numpy as np
import pytest

import text_checker as tc

pytestmark = pytest.mark.gpu


def _ctor(sm, mode, canonical):
    if mode == 0:
        return sm.canonical_minimizers if canonical else sm.minimizers
    if mode == 1:
        return sm.canonical_closed_syncmers if canonical else sm.closed_syncmers
    return sm.canonical_open_syncmers if canonical else sm.open_syncmers


def _sweep_records(l, seed, alphabet=None):
    """Lengths 0, 1, l-1, l, l+1, 8191, 8192, 8193, 20000 in random order, with runs of empty records."""
    rng = np.random.default_rng(seed)
    lens = [0, 1, l - 1, l, l + 1, 8191, 8192, 8193, 20_000, 2 * l, 3, 100, 5000]
    lens = [int(x) for x in rng.permutation(lens)]
    lens[3:3] = [0] * 7
    lens += [0] * 5 + [l + 2]
    recs = []
    for n in lens:
        if alphabet is None:
            recs.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        else:
            recs.append(alphabet[rng.integers(0, len(alphabet), n)].tobytes())
    return recs


def _check_batch(sm, b, records, sk=False, checker=None):
    """Every slice, every offset and the count against the single-text path (and the numpy checker if given)."""
    pos, offs, idx = sm.run_text_batch_host(b, records, super_kmers=sk)
    assert len(offs) == len(records) + 1 and offs[0] == 0 and offs[-1] == len(pos)
    single = b.super_kmers([]) if sk else b
    for r, rec in enumerate(records):
        want, want_sk = single._run_arrays(rec)
        got = pos[offs[r]:offs[r + 1]]
        assert np.array_equal(got, want), (r, len(rec))
        if sk:
            assert np.array_equal(idx[offs[r]:offs[r + 1]], want_sk), (r, len(rec))
        if checker is not None and len(rec) <= 20_000:
            th, canonical, mode = checker
            c = tc.run(rec, b.k, b.w, th, canonical, mode, super_kmers=sk)
            if sk:
                assert np.array_equal(got, c[0]) and np.array_equal(idx[offs[r]:offs[r + 1]], c[1]), r
            else:
                assert np.array_equal(got, c), r
    return pos, offs, idx


@pytest.mark.parametrize("w", [11, 37])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_record_length_sweep_bytes(sm, gpu, mode, canonical, w):
    """Arbitrary bytes with TextMulHasher: prebuilt w (11) and run-time w (37), minimizers and both syncmers."""
    k = 21
    th = sm.TextMulHasher(canonical=canonical)
    b = _ctor(sm, mode, canonical)(k, w).hasher(th)
    recs = _sweep_records(k + w - 1, 100 + 10 * mode + w + canonical)
    _check_batch(sm, b, recs, checker=(th, canonical, mode))
    assert gpu.last_path() == sm.PATH_FUSED


@pytest.mark.parametrize("w", [11, 37])
@pytest.mark.parametrize("canonical", [False, True])
def test_record_length_sweep_super_kmers(sm, gpu, canonical, w):
    k = 21
    th = sm.TextMulHasher(canonical=canonical)
    b = _ctor(sm, 0, canonical)(k, w).hasher(th)
    _check_batch(sm, b, _sweep_records(k + w - 1, 7 + w + canonical), sk=True, checker=(th, canonical, 0))


@pytest.mark.parametrize("canonical", [False, True])
def test_record_length_sweep_dna_hasher(sm, gpu, canonical):
    """mm_text_hasher_from_dna on ASCII DNA (both cases), k=21 w=11 and k=5 w=19."""
    th = sm.TextHasher.from_dna(sm.NtHasher(canonical=canonical))
    alphabet = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
    for k, w in [(21, 11), (5, 19)]:
        b = _ctor(sm, 0, canonical)(k, w).hasher(th)
        _check_batch(sm, b, _sweep_records(k + w - 1, 3 + k, alphabet), sk=not canonical, checker=(th, canonical, 0))


def test_dense_boundaries_overflow_the_lds_list(sm, gpu):
    """100 000 records of 1-3 bytes among a few long ones: tiles hold far more record starts than the LDS list, and take
    the global-memory path.  k=1 w=2 (l = 2), so the short records have windows of their own."""
    rng = np.random.default_rng(11)
    lens = rng.integers(1, 4, 100_000)
    lens[[5, 40_000, 77_777]] = [30_000, 9000, 20_000]
    text = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    starts = np.concatenate([[0], np.cumsum(lens)])
    recs = [text[starts[i]:starts[i + 1]] for i in range(len(lens))]
    for canonical, mode, k, w in [(False, 0, 1, 2), (True, 0, 1, 3), (False, 1, 1, 2), (False, 0, 3, 5)]:
        th = sm.TextMulHasher(canonical=canonical)
        b = _ctor(sm, mode, canonical)(k, w).hasher(th)
        pos, offs, idx = sm.run_text_batch_host(b, recs, super_kmers=mode == 0)
        assert gpu.last_path() == sm.PATH_FUSED
        assert offs[-1] == len(pos)
        for r, rec in enumerate(recs):
            got = pos[offs[r]:offs[r + 1]]
            want = tc.run(rec, k, w, th, canonical, mode, super_kmers=mode == 0)
            if mode == 0:
                assert np.array_equal(got, want[0]) and np.array_equal(idx[offs[r]:offs[r + 1]], want[1]), (r, k, w)
            else:
                assert np.array_equal(got, want), (r, k, w)


def _protein_records(n_rec, seed, median=300.0):
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.lognormal(np.log(median), 0.555, n_rec), 30, 35_000).astype(np.int64)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    text = aa[rng.integers(0, 20, int(lens.sum()))]
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return text, starts


def test_scale_protein_like(sm, gpu):
    """About 50 Mchar over 150 000 protein-like records: every record against the single-text GPU path, 2 000 sampled
    records against text_checker."""
    import torch

    text, starts = _protein_records(150_000, 5)
    n_rec, n = len(starts) - 1, int(starts[-1])
    assert 40_000_000 < n < 60_000_000
    k, w = 7, 11
    th = sm.TextMulHasher(canonical=False)
    b = sm.minimizers(k, w).hasher(th)
    d_text = torch.from_numpy(text).cuda()
    d_starts = torch.from_numpy(starts.view(np.int64)).cuda()
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    offs = torch.empty(n_rec + 1, dtype=torch.int64, device="cuda")
    cnt = sm.run_text_batch_device(b, d_text, d_starts, n, out, offs)
    assert gpu.last_path() == sm.PATH_FUSED
    pos = out[:cnt].cpu().numpy().view(np.uint32)
    offs = offs.cpu().numpy()
    assert offs[0] == 0 and offs[-1] == cnt
    one = torch.empty(35_000, dtype=torch.int32, device="cuda")
    for r in range(n_rec):
        a, e = int(starts[r]), int(starts[r + 1])
        c = b.run_text_device(d_text[a:e], e - a, one)
        assert offs[r + 1] - offs[r] == c, r
        assert np.array_equal(pos[offs[r]:offs[r + 1]], one[:c].cpu().numpy().view(np.uint32)), r
    for r in np.random.default_rng(6).choice(n_rec, 2000, replace=False):
        a, e = int(starts[r]), int(starts[r + 1])
        assert np.array_equal(pos[offs[r]:offs[r + 1]], tc.run(text[a:e], k, w, th)), r


@pytest.mark.parametrize("force", [False, True])
def test_generic_route(sm, gpu, force):
    """w = 201 (past the fused kernel) and mm_workspace_force_generic: one generic launch per record, same contract."""
    w = 11 if force else 201
    for canonical, mode in [(False, 0), (True, 0), (False, 1)]:
        th = sm.TextMulHasher(canonical=canonical)
        b = _ctor(sm, mode, canonical)(21, w).hasher(th)
        rng = np.random.default_rng(w + canonical + mode)
        recs = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()
                for n in [0, 5, 230, 220, 221, 222, 0, 0, 3000, 40, 1500]]
        gpu.force_generic(force)
        try:
            pos, offs, idx = sm.run_text_batch_host(b, recs, super_kmers=mode == 0)
            assert gpu.last_path() == sm.PATH_GENERIC
        finally:
            gpu.force_generic(False)
        for r, rec in enumerate(recs):
            want = tc.run(rec, 21, w, th, canonical, mode, super_kmers=mode == 0)
            got = pos[offs[r]:offs[r + 1]]
            if mode == 0:
                assert np.array_equal(got, want[0]) and np.array_equal(idx[offs[r]:offs[r + 1]], want[1]), r
            else:
                assert np.array_equal(got, want), r


# ------------------------------------------------------------------ contracts


def _dev_batch(sm, b, d_text, d_starts, n_chars, cap, sk=False, count_only=False):
    import torch
    n_rec = d_starts.numel() - 1
    out = None if count_only else torch.zeros(max(1, cap), dtype=torch.int32, device="cuda")
    osk = torch.zeros(max(1, cap), dtype=torch.int32, device="cuda") if sk else None
    offs = torch.full((n_rec + 1,), -1, dtype=torch.int64, device="cuda")
    cnt = C.c_uint64()
    code = sm.lib().mm_run_text_batch_device(
        b.text_plan().h, b._ws().h, C.c_void_p(d_text.data_ptr()), d_text.numel(), n_rec,
        C.c_void_p(d_starts.data_ptr()), n_chars, C.c_void_p(out.data_ptr()) if out is not None else None,
        C.c_void_p(osk.data_ptr()) if osk is not None else None, cap if out is not None else 0,
        C.c_void_p(offs.data_ptr()), C.byref(cnt))
    return code, int(cnt.value), out, offs, osk


def test_nonzero_first_start_and_unaligned_text(sm, gpu):
    import torch
    rng = np.random.default_rng(21)
    raw = rng.integers(0, 256, 30_003, dtype=np.uint8)
    base = torch.from_numpy(raw).cuda()
    d_text = base[3:]  # (an unaligned pointer)
    text = raw[3:]
    starts = np.array([7, 7, 500, 9000, 9031, 20_000, 30_000], dtype=np.uint64)
    b = sm.minimizers(21, 11)
    code, cnt, out, offs, _ = _dev_batch(sm, b, d_text, torch.from_numpy(starts.view(np.int64)).cuda(), 30_000, 30_000)
    assert code == 0
    pos, offs = out[:cnt].cpu().numpy().view(np.uint32), offs.cpu().numpy()
    assert offs[0] == 0 and offs[-1] == cnt
    th = sm.TextMulHasher(canonical=False)
    for r in range(len(starts) - 1):
        want = tc.run(text[starts[r]:starts[r + 1]], 21, 11, th)
        assert np.array_equal(pos[offs[r]:offs[r + 1]], want), r


def test_empty_and_short_batches(sm, gpu):
    import torch
    b = sm.minimizers(21, 11)
    d_text = torch.zeros(64, dtype=torch.uint8, device="cuda")
    code, cnt, _, offs, _ = _dev_batch(sm, b, d_text, torch.zeros(1, dtype=torch.int64, device="cuda"), 0, 10)
    assert code == 0 and cnt == 0 and offs.cpu().tolist() == [0]
    pos, offs, idx = sm.run_text_batch_host(b, [])
    assert len(pos) == 0 and offs == [0] and idx is None
    recs = [b"x" * n for n in [0, 30, 1, 0, 29, 30]]  # every record shorter than l = 31
    pos, offs, _ = sm.run_text_batch_host(b, recs)
    assert len(pos) == 0 and offs == [0] * 7
    recs = [bytes(range(40))] + [b"y" * 30] * 300 + [bytes(range(50))]  # long enough in total, not per record
    pos, offs, _ = sm.run_text_batch_host(b, recs)
    assert offs[1:-1] == [offs[1]] * 301 and offs[-1] == len(pos)
    assert np.array_equal(pos[offs[-2]:], b._run_arrays(recs[-1])[0])


def test_count_only_and_capacity(sm, gpu):
    import torch
    text, starts = _protein_records(300, 9)
    n = int(starts[-1])
    b = sm.minimizers(21, 11)
    d_text, d_starts = torch.from_numpy(text).cuda(), torch.from_numpy(starts.view(np.int64)).cuda()
    code, cnt, out, offs, _ = _dev_batch(sm, b, d_text, d_starts, n, n)
    assert code == 0 and cnt > 0
    code2, cnt2, _, offs2, _ = _dev_batch(sm, b, d_text, d_starts, n, 0, count_only=True)
    assert code2 == 0 and cnt2 == cnt and torch.equal(offs, offs2)
    code3, cnt3, _, _, _ = _dev_batch(sm, b, d_text, d_starts, n, cnt - 1)
    assert code3 == sm.ERR["CAPACITY"] and cnt3 == cnt
    code4, _, _, _, _ = _dev_batch(sm, b, d_text[:n - 1], d_starts, n, n)  # n_chars > text_bytes
    assert code4 == sm.ERR["CAPACITY"]
    with pytest.raises(sm.MinimizerError) as e:
        sm.run_text_batch_device(b, d_text, d_starts, n, torch.empty(cnt - 1, dtype=torch.int32, device="cuda"),
                                 torch.empty(len(starts), dtype=torch.int64, device="cuda"))
    assert e.value.code == sm.ERR["CAPACITY"]


def test_refusals(sm, gpu):
    L = sm.lib()
    ws = gpu.h
    cnt = C.c_uint64()
    b = sm.minimizers(21, 11)
    # n_chars >= 2^32: refused before any pointer is looked at
    assert L.mm_run_text_batch_device(b.text_plan().h, ws, None, 1 << 33, 1, None, 1 << 32, None, None, 0, None,
                                      C.byref(cnt)) == sm.ERR["LEN_TOO_LARGE"]
    assert L.mm_run_text_batch_device_async(b.text_plan().h, ws, None, 1 << 33, 1, None, 1 << 32, None, None, 0, None,
                                            None) == sm.ERR["LEN_TOO_LARGE"]
    # a packed plan
    assert L.mm_run_text_batch_device(b.plan().h, ws, None, 0, 0, None, 0, None, None, 0, None,
                                      C.byref(cnt)) == sm.ERR["BAD_MODE"]
    with pytest.raises(sm.MinimizerError) as e:
        sm.run_text_batch_host(sm.closed_syncmers(21, 11), [b"a" * 100], super_kmers=True)
    assert e.value.code == sm.ERR["BAD_MODE"]
    text = np.zeros(100, dtype=np.uint8)
    starts = np.array([0, 50, 40, 100], dtype=np.uint64)
    offs = np.zeros(4, dtype=np.uint64)
    pos = np.zeros(100, dtype=np.uint32)
    assert L.mm_run_text_batch_host(b.text_plan().h, ws, text.ctypes.data_as(C.POINTER(C.c_uint8)), 3,
                                    starts.ctypes.data_as(C.POINTER(C.c_uint64)), pos.ctypes.data_as(C.POINTER(C.c_uint32)),
                                    None, 100, offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                    C.byref(cnt)) == sm.ERR["UNSORTED"]
    # every packed entry point still refuses a text plan
    assert L.mm_run_host(b.text_plan().h, ws, None, 0, 0, None, None, 0, C.byref(cnt)) == sm.ERR["BAD_MODE"]


def test_async_then_check_and_device_unchanged(sm, gpu):
    import torch
    text, starts = _protein_records(2000, 13)
    n = int(starts[-1])
    b = sm.minimizers(21, 11)
    d_text, d_starts = torch.from_numpy(text).cuda(), torch.from_numpy(starts.view(np.int64)).cuda()
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    offs = torch.empty(len(starts), dtype=torch.int64, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    dev = torch.cuda.current_device()
    L = sm.lib()
    assert L.mm_run_text_batch_device_async(b.text_plan().h, gpu.h, C.c_void_p(d_text.data_ptr()), n, len(starts) - 1,
                                            C.c_void_p(d_starts.data_ptr()), n, C.c_void_p(out.data_ptr()), None, n,
                                            C.c_void_p(offs.data_ptr()), C.c_void_p(d_cnt.data_ptr())) == 0
    assert L.mm_workspace_check(gpu.h) == 0
    assert torch.cuda.current_device() == dev
    cnt = int(d_cnt.item())
    pos, offs_h, _ = sm.run_text_batch_host(b, [text[starts[i]:starts[i + 1]] for i in range(len(starts) - 1)])
    assert cnt == len(pos) and offs.cpu().tolist() == offs_h
    assert np.array_equal(out[:cnt].cpu().numpy().view(np.uint32), pos)


def test_cxx_run_many_text_example(gpu, tmp_path):
    """The C++ mirror: Builder::run_many(std::vector<TextSeq>, pos, offsets) (tests/cxx/text_batch_example.cpp)."""
    import os
    import subprocess

    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    exe = str(tmp_path / "text_batch_example")
    libdir = os.path.join(root, "simd-minimizers_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(root, "include"), "-o", exe,
                    os.path.join(here, "cxx", "text_batch_example.cpp"), "-L" + libdir, "-lsimd_minimizers_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
