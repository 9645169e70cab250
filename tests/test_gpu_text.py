"""General byte text (``&[u8]``, src/lib.rs:59, :71-72) on the GPU, everything through the C ABI: the known answer of
the AsciiSeq doctest, metamorphic checks against the pinned 2-bit path, arbitrary bytes against the numpy checker
(tests/text_checker.py), and the entry points' contracts."""
import ctypes as C

import numpy as np
import pytest

import text_checker as tc

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1


def _ctor(sm, mode, canonical):
    if mode == 0:
        return sm.canonical_minimizers if canonical else sm.minimizers
    if mode == 1:
        return sm.canonical_closed_syncmers if canonical else sm.closed_syncmers
    return sm.canonical_open_syncmers if canonical else sm.open_syncmers


def _text_run(sm, k, w, canonical, mode, th, text, sk=False):
    """Host text entry point (mm_run_text_host) through the builder: (positions, super-k-mer indices or None)."""
    b = _ctor(sm, mode, canonical)(k, w).hasher(th)
    if sk:
        b = b.super_kmers([])
    return b._run_arrays(text)


def _dna_codes_hasher(sm, canonical):
    fw, rc = tc.text_tables_from_dna(sm.NtHasher(canonical=canonical))
    return sm.TextHasher.from_tables(fw, rc, rot=7, canonical=canonical)


def _random_text_hasher(sm, seed, canonical):
    rng = np.random.default_rng(seed)
    fw = rng.integers(0, 1 << 32, 256, dtype=np.uint64)
    rc = rng.integers(0, 1 << 32, 256, dtype=np.uint64)
    return sm.TextHasher.from_tables(fw, rc, rot=int(rng.integers(1, 32)), canonical=canonical,
                                     fw_xor=int(rng.integers(1, 1 << 32)), rc_xor=int(rng.integers(1, 1 << 32)))


# ------------------------------------------------------------------ (a) known answer


def test_ascii_doctest_known_answer(sm, gpu):
    """src/lib.rs:92-101: AsciiSeq(b"ACGTGCTCAGAGACTCAG"), k=5, w=7 -> [4, 5, 8, 13], here as byte text."""
    th = sm.TextHasher.from_dna(sm.NtHasher(canonical=False))
    b = sm.minimizers(5, 7).hasher(th)
    assert b.run_once(b"ACGTGCTCAGAGACTCAG") == [4, 5, 8, 13]
    assert gpu.last_path() == sm.PATH_FUSED
    gpu.force_generic(True)
    try:
        assert b.run_once(b"ACGTGCTCAGAGACTCAG") == [4, 5, 8, 13]
        assert gpu.last_path() == sm.PATH_GENERIC
    finally:
        gpu.force_generic(False)
    assert b.run_once(np.frombuffer(b"ACGTGCTCAGAGACTCAG", dtype=np.uint8)) == [4, 5, 8, 13]


# ------------------------------------------------------- (b) against the pinned path

KS = [1, 5, 21, 31, 63]
# every shipped fused text instance (mm_text_prebuilt_window_sizes) plus window sizes of the run-time-w instance
EXTRA_WS = [1, 2, 24, 33, 64, 127, 128]


def _sweep_ws(sm, canonical):
    return sorted(set(sm.text_prebuilt_window_sizes(canonical)) | set(EXTRA_WS))


def test_prebuilt_text_window_sizes(sm):
    """(e) the list the sweeps walk: the paper's windows (bench/src/bin/paper.rs:343-361), both strands."""
    for canonical in (False, True):
        ws = sm.text_prebuilt_window_sizes(canonical)
        assert ws == sorted(ws) and {5, 11, 19} <= set(ws)
        assert all(w <= 128 for w in ws)


def test_forward_ascii_dna_equals_packed_path(sm, gpu, oracle):
    """Random ASCII DNA: forward text minimizers / syncmers / super-k-mer indices with the DNA table equal the AsciiSeq
    entry point (mm_run_host_ascii, the fused kernels) and the oracle."""
    n = (1 << 20) + 12345
    rng = np.random.default_rng(11)
    text = np.frombuffer(b"ACGTacgt", dtype=np.uint8)[rng.integers(0, 8, n)]
    th = sm.TextHasher.from_dna(sm.NtHasher(canonical=False))
    packed = oracle.pack_ascii(text.tobytes())
    asc = sm.AsciiSeq(text.tobytes())
    for k in KS:
        for w in _sweep_ws(sm, False):
            for mode in (0, 1, 2):
                if mode == 2 and w % 2 == 0:
                    continue
                sk = mode == 0
                got, gsk = _text_run(sm, k, w, False, mode, th, text, sk=sk)
                assert gpu.last_path() == sm.PATH_FUSED
                b = _ctor(sm, mode, False)(k, w)
                if sk:
                    b = b.super_kmers([])
                want, wsk = b._run_arrays(asc)
                assert np.array_equal(got, want), (k, w, mode)
                if sk:
                    assert np.array_equal(gsk, wsk), (k, w)
                ref = oracle.run(packed, n, k, w, oracle.default_hasher(False), False, mode)
                assert np.array_equal(got, ref), (k, w, mode)


def test_canonical_code_bytes_equal_packed_path(sm, gpu, oracle):
    """Canonical windows: the code bytes 0..3 as text with fw[c] = nt.fw[c & 3] (c & 2 is then the packed strand vote)
    equal the canonical packed path on the same codes, and the oracle."""
    n = (1 << 20) + 777
    codes = np.random.default_rng(12).integers(0, 4, n, dtype=np.uint8)
    codes[100_000:140_000] = 3  # low complexity: ties and a one-sided vote
    th = _dna_codes_hasher(sm, True)
    pseq = sm.PackedSeqVec.from_codes(codes)
    packed = tc.pack_codes(codes)
    for k in KS:
        for w in _sweep_ws(sm, True):
            if (k + w - 1) % 2 == 0:
                continue
            for mode in (0, 1, 2):
                if mode == 2 and w % 2 == 0:
                    continue
                sk = mode == 0
                got, gsk = _text_run(sm, k, w, True, mode, th, codes, sk=sk)
                b = _ctor(sm, mode, True)(k, w)
                if sk:
                    b = b.super_kmers([])
                want, wsk = b._run_arrays(pseq)
                assert np.array_equal(got, want), (k, w, mode)
                if sk:
                    assert np.array_equal(gsk, wsk), (k, w)
                ref = oracle.run(packed, n, k, w, oracle.default_hasher(True), True, mode)
                assert np.array_equal(got, ref), (k, w, mode)


@pytest.mark.parametrize("canonical", [False, True])
def test_256M_text_equals_packed_device_path(sm, gpu, canonical):
    """256 Mchar, device against device: the fused text kernel equals the packed fused kernel element by element."""
    import torch

    n, k, w = 256 << 20, 21, 11
    g = torch.Generator(device="cuda").manual_seed(5 + canonical)
    codes = torch.randint(0, 4, (n,), dtype=torch.uint8, device="cuda", generator=g)
    q = codes.view(-1, 4).to(torch.int32)
    packed = torch.zeros(n // 4 + 64, dtype=torch.uint8, device="cuda")
    packed[: n // 4] = (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).to(torch.uint8)
    del q
    if canonical:
        text, th = codes, _dna_codes_hasher(sm, True)
    else:
        text = torch.tensor(list(b"ACTG"), dtype=torch.uint8, device="cuda")[codes.long()]
        th = sm.TextHasher.from_dna(sm.NtHasher(canonical=False))
    out_t = torch.zeros(n, dtype=torch.int32, device="cuda")
    out_p = torch.zeros(n, dtype=torch.int32, device="cuda")
    b = _ctor(sm, 0, canonical)(k, w).hasher(th)
    torch.cuda.synchronize()
    ct = b.run_text_device(text, n, out_t)
    assert gpu.last_path() == sm.PATH_FUSED
    cp = b.run_device(packed, n, out_p)
    assert gpu.last_path() == sm.PATH_FUSED
    assert ct == cp > n // 10
    assert torch.equal(out_t[:ct], out_p[:cp])


# ----------------------------------------------------------------- (c) arbitrary bytes


@pytest.mark.parametrize("canonical", [False, True])
def test_64M_fused_equals_generic(sm, gpu, canonical):
    """64 Mchar of uniform random bytes, device against device: the fused text kernel equals the generic text family,
    for every shipped window size and a run-time one, all three modes."""
    import torch

    n = 64 << 20
    g = torch.Generator(device="cuda").manual_seed(17 + canonical)
    text = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    th = sm.TextMulHasher(canonical=canonical)
    out_f = torch.zeros(n, dtype=torch.int32, device="cuda")
    out_g = torch.zeros(n, dtype=torch.int32, device="cuda")
    for w in sm.text_prebuilt_window_sizes(canonical) + [7]:
        k = 21 if (21 + w - 1) % 2 == 1 else 22
        for mode in (0, 1, 2):
            b = _ctor(sm, mode, canonical)(k, w).hasher(th)
            cf = b.run_text_device(text, n, out_f)
            assert gpu.last_path() == sm.PATH_FUSED
            gpu.force_generic(True)
            try:
                cg = b.run_text_device(text, n, out_g)
                assert gpu.last_path() == sm.PATH_GENERIC
            finally:
                gpu.force_generic(False)
            assert cf == cg > 0 and torch.equal(out_f[:cf], out_g[:cg]), (w, mode)


def _inputs(n):
    rng = np.random.default_rng(21)
    return {
        "uniform": rng.integers(0, 256, n, dtype=np.uint8),
        "english": tc.english_like(n, 22),
        "0_255": np.where(rng.integers(0, 2, n) == 1, 255, 0).astype(np.uint8),
        "repeat": np.full(n, ord("A"), dtype=np.uint8),
        "period2": np.resize(np.frombuffer(b"\x07\xf2", dtype=np.uint8), n),
        "period3": np.resize(np.frombuffer(b"xyz", dtype=np.uint8), n),
    }


@pytest.mark.parametrize("hasher", ["mul", "random"])
@pytest.mark.parametrize("canonical", [False, True])
def test_arbitrary_bytes_equal_checker(sm, gpu, hasher, canonical):
    n = 1 << 19
    th = sm.TextMulHasher(canonical=canonical) if hasher == "mul" else _random_text_hasher(sm, 31 + canonical, canonical)
    for name, text in _inputs(n).items():
        for k, w in [(21, 11), (5, 5), (31, 19), (1, 3)]:
            for mode in (0, 1, 2):
                sk = mode == 0
                got, gsk = _text_run(sm, k, w, canonical, mode, th, text, sk=sk)
                want = tc.run(text, k, w, th, canonical, mode, super_kmers=sk)
                if sk:
                    want, wsk = want
                    assert np.array_equal(gsk, wsk), (name, k, w)
                assert np.array_equal(got, want), (name, k, w, mode)


# ---------------------------------------------------------------------- (d) contracts


def test_short_lengths(sm, gpu):
    th = sm.TextMulHasher(canonical=True)
    for canonical in (False, True):
        k, w = 5, 7
        l = k + w - 1
        for n in (0, 1, l - 1, l, l + 1):
            text = bytes((i * 37 + 11) & 0xFF for i in range(n))
            got, _ = _text_run(sm, k, w, canonical, 0, th, text)
            assert list(got) == list(tc.run(text, k, w, th, canonical, 0)), n
            if n < l:
                assert len(got) == 0
            elif n == l:
                assert len(got) == 1
    import torch
    b = sm.minimizers(5, 7)
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert b.run_text_device(torch.zeros(0, dtype=torch.uint8, device="cuda"), 0, out) == 0


def test_unaligned_pointer_and_odd_size(sm, gpu):
    import torch

    n = 300_001
    text = np.random.default_rng(5).integers(0, 256, n, dtype=np.uint8)
    th = sm.TextMulHasher(canonical=True)
    want = tc.run(text, 21, 11, th, True, 0)
    for off in (1, 2, 3, 5):
        buf = torch.zeros(n + off + 2, dtype=torch.uint8, device="cuda")
        buf[off: off + n] = torch.from_numpy(text).cuda()
        d = buf[off: off + n]  # odd readable size, pointer not aligned
        assert d.data_ptr() % 4 != 0 or off % 4 == 0
        out = torch.zeros(n, dtype=torch.int32, device="cuda")
        cnt = sm.canonical_minimizers(21, 11).hasher(th).run_text_device(d, n, out)
        assert np.array_equal(out[:cnt].cpu().numpy().view(np.uint32), want), off


def test_window_ranges_concatenate(sm, gpu):
    import torch

    n, k, w = 200_003, 15, 9
    text = tc.english_like(n, 8)
    th = sm.TextMulHasher(canonical=False)
    d = torch.from_numpy(text).cuda()
    nw = n - (k + w - 1) + 1
    for mode in (0, 1, 2):
        b = _ctor(sm, mode, False)(k, w).hasher(th)
        full = torch.zeros(nw, dtype=torch.int32, device="cuda")
        cf = b.run_text_device(d, n, full)
        assert np.array_equal(full[:cf].cpu().numpy().view(np.uint32), tc.run(text, k, w, th, False, mode))
        cuts = sorted({0, 1, 2, 17, 4095, 4096, 4097, 65536, 100_000, 150_001, nw - 1, nw})
        parts = []
        for a, e in zip(cuts[:-1], cuts[1:]):
            o = torch.zeros(max(1, e - a), dtype=torch.int32, device="cuda")
            c = b.run_text_device(d, n, o, win_begin=a, win_end=e)
            parts.append(o[:c].cpu().numpy().view(np.uint32))
        assert np.array_equal(np.concatenate(parts), full[:cf].cpu().numpy().view(np.uint32)), mode


def test_capacity_too_small_and_count_only(sm, gpu):
    import torch

    L = sm.lib()
    n, k, w = 100_000, 21, 11
    text = np.random.default_rng(9).integers(0, 256, n, dtype=np.uint8)
    th = sm.TextMulHasher(canonical=False)
    want = tc.run(text, k, w, th, False, 0)
    b = sm.minimizers(k, w).hasher(th)
    d = torch.from_numpy(text).cuda()
    cap = len(want) // 3
    buf = torch.full((len(want) + 64,), -1, dtype=torch.int32, device="cuda")
    sk = torch.full((len(want) + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cnt = C.c_uint64()
    code = L.mm_run_text_device(b.text_plan().h, b._ws().h, C.c_void_p(d.data_ptr()), n, n, 0, U64_MAX,
                                C.c_void_p(buf.data_ptr()), C.c_void_p(sk.data_ptr()), cap, C.byref(cnt))
    assert code == sm.ERR["CAPACITY"] and cnt.value == len(want)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:cap].view(np.uint32), want[:cap])
    assert (got[cap:] == -1).all() and (sk.cpu().numpy()[cap:] == -1).all()
    # count only
    assert b.run_text_device(d, n, None) == len(want)
    pos = np.zeros(1, dtype=np.uint32)
    assert L.mm_run_text_host(b.text_plan().h, b._ws().h, text.ctypes.data_as(C.POINTER(C.c_uint8)), n, None, None, 0,
                              C.byref(cnt)) == 0 and cnt.value == len(want)
    # asynchronous, count to the device
    dc = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    b.run_text_device(d, n, out, sync=False, d_count=dc)
    b._ws().check()
    assert int(dc.item()) == len(want)
    assert np.array_equal(out[: len(want)].cpu().numpy().view(np.uint32), want)
    del pos


def test_large_w(sm, gpu):
    n = 200_000
    text = tc.english_like(n, 4)
    for canonical, k, w in [(False, 21, 200), (True, 22, 200), (True, 5, 1001)]:
        th = sm.TextMulHasher(canonical=canonical)
        for mode in (0, 1):
            got, _ = _text_run(sm, k, w, canonical, mode, th, text)
            assert np.array_equal(got, tc.run(text, k, w, th, canonical, mode)), (k, w, mode)
            assert gpu.last_path() == sm.PATH_GENERIC


def test_plan_kinds_are_not_mixed(sm, gpu):
    import torch

    L = sm.lib()
    ws = gpu
    d = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1024, dtype=torch.int32, device="cuda")
    cnt = C.c_uint64()
    tp = sm.Plan(5, 7, False, 0, None, text=True)
    pp = sm.Plan(5, 7, False, 0, None)
    args = (C.c_void_p(d.data_ptr()), 1024, 0, 1000, 0, U64_MAX, C.c_void_p(out.data_ptr()), None, 1024, C.byref(cnt))
    assert L.mm_run_device(tp.h, ws.h, *args) == sm.ERR["BAD_MODE"]
    targs = (C.c_void_p(d.data_ptr()), 1024, 1000, 0, U64_MAX, C.c_void_p(out.data_ptr()), None, 1024, C.byref(cnt))
    assert L.mm_run_text_device(pp.h, ws.h, *targs) == sm.ERR["BAD_MODE"]
    assert L.mm_run_text_device_async(pp.h, ws.h, *targs[:-1], None) == sm.ERR["BAD_MODE"]
    h = np.zeros(1000, dtype=np.uint8)
    assert L.mm_run_text_host(pp.h, ws.h, h.ctypes.data_as(C.POINTER(C.c_uint8)), 1000, None, None, 0,
                              C.byref(cnt)) == sm.ERR["BAD_MODE"]
    assert L.mm_run_text_device(tp.h, ws.h, *targs) == 0
    # super-k-mer indices with syncmers
    sp = sm.Plan(5, 7, False, 1, None, text=True)
    assert L.mm_run_text_device(sp.h, ws.h, C.c_void_p(d.data_ptr()), 1024, 1000, 0, U64_MAX,
                                C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr()), 1024,
                                C.byref(cnt)) == sm.ERR["BAD_MODE"]


def test_len_too_large_before_memory(sm, gpu):
    L = sm.lib()
    tp = sm.Plan(5, 7, False, 0, None, text=True)
    cnt = C.c_uint64()
    n = 1 << 32
    assert L.mm_run_text_device(tp.h, gpu.h, None, 0, n, 0, U64_MAX, None, None, 0, C.byref(cnt)) == sm.ERR["LEN_TOO_LARGE"]
    assert L.mm_run_text_device_async(tp.h, gpu.h, None, 0, n, 0, U64_MAX, None, None, 0, None) == sm.ERR["LEN_TOO_LARGE"]
    assert L.mm_run_text_host(tp.h, gpu.h, None, n, None, None, 0, C.byref(cnt)) == sm.ERR["LEN_TOO_LARGE"]


def test_current_device_unchanged(sm, gpu):
    """The caller's current device after a text call is what it was before.  With two devices the workspace lives on the
    other one, so the call must select it and put the caller's back; with one device the call must leave it selected."""
    import torch

    text = tc.english_like(50_000, 3)
    th = sm.TextMulHasher(canonical=False)
    want = tc.run(text, 21, 11, th, False, 0)
    ndev = torch.cuda.device_count()
    before = torch.cuda.current_device()
    ws_dev = ndev - 1
    ws = sm.Workspace(ws_dev) if ws_dev != 0 else gpu
    try:
        torch.cuda.set_device(0)
        got = sm.minimizers(21, 11).hasher(th).workspace(ws).run_once(text.tobytes())
        assert torch.cuda.current_device() == 0
        assert ws.last_path() == sm.PATH_FUSED
    finally:
        torch.cuda.set_device(before)
        if ws is not gpu:
            ws.close()
    assert got == list(want)


def test_cxx_text_example(gpu, tmp_path):
    """The C++ mirror: Builder::run(TextSeq, pos) and .hasher(mm_text_hasher_t) (tests/cxx/text_example.cpp)."""
    import os
    import subprocess

    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    exe = str(tmp_path / "text_example")
    libdir = os.path.join(root, "simd-minimizers_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(root, "include"), "-o", exe,
                    os.path.join(here, "cxx", "text_example.cpp"), "-L" + libdir, "-lsimd_minimizers_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
