"""The fixed-k flavour of the fused kernel (round 7; DESIGN.md 4.1 "One load stream"): for k=21 w=11, canonical and
forward (the forward instance only in builds with -DMM_KC_FORWARD), the launcher takes a kernel compiled for that k whose walk reads the sequence through ONE load stream - the
bases leaving the hash come out of the hash-in buffers of the current and the previous load group.  It must compute
what the run-time-k kernel computes: every case here is compared with the CPU oracle, and one test compares the two
kernels' whole output buffers on 64 Mbp."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (k, w, canonical) of every prebuilt fixed-k instance (mm_fused_inst_kc.hip; the forward k=21 w=11 instance is built only
# with -DMM_KC_FORWARD: it measured no faster than the run-time-k kernel and is not in the default dispatch)
INSTANCES = [(21, 11, True)]


def _dev(out, c):
    return out[:c].cpu().numpy().view(np.uint32)


def _range_expect(oracle, data, n, k, w, canonical, a, e, base_offset=0):
    """positions of a run over windows [a, e): that range's per-window stream, deduplicated against the window before it"""
    per_window = oracle.window_positions(data, n, k, w, oracle.default_hasher(canonical), canonical, base_offset=base_offset)
    sub = per_window[a:e]
    keep = np.ones(len(sub), dtype=bool)
    keep[1:] = sub[1:] != sub[:-1]
    if a > 0 and len(sub):
        keep[0] = sub[0] != per_window[a - 1]
    return sub[keep]


def test_launcher_selects_the_fixed_k_kernel(sm):
    """No GPU: the instances exist for exactly their (k, w, flavour); a k beside it, another w, or k=31 w=51 (whose load
    groups are no whole number of bytes, kc_rule) take the run-time-k kernel."""
    L = sm.lib()
    for k, w, canonical in INSTANCES:
        assert L.mm_debug_fixed_k_kernel(k, w, int(canonical)) == 1, (k, w, canonical)
        for k2 in (k - 2, k - 1, k + 1, k + 2):
            assert L.mm_debug_fixed_k_kernel(k2, w, int(canonical)) == 0, (k2, w, canonical)
        assert L.mm_debug_fixed_k_kernel(k, w + 2, int(canonical)) == 0
    assert L.mm_debug_fixed_k_kernel(31, 51, 1) == 0
    assert L.mm_debug_fixed_k_kernel(21, 11, 0) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("k,w,canonical", INSTANCES)
def test_lengths_and_offsets_vs_oracle(sm, oracle, gpu, k, w, canonical):
    """Sequence ends inside the lane's first block, inside its first load group (blocks 2 .. 5 of a lane: windows 11 .. 54),
    on a group boundary, on a lane boundary and on a tile boundary (short runs walk 6 blocks per lane: 66 windows a lane,
    16 896 a tile), each at base offsets whose byte part is 0 .. 3 (and larger ones)."""
    import torch
    assert sm.lib().mm_debug_fixed_k_kernel(k, w, int(canonical)) == 1
    l = k + w - 1
    tile = 256 * 6 * w
    windows = [1, 5, 11, 12, 30, 54, 55, 56, 66, 67, 99, 110, tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 45, 5 * tile + 54]
    big = windows[-1] + l + 64
    data = oracle.gen_packed(31, big)
    d = torch.from_numpy(data).cuda()
    out = torch.zeros(big, dtype=torch.int32, device="cuda")
    b = sm.Builder(k, w, canonical, 0)
    for nw in windows:
        for off in (0, 1, 2, 3, 5, 14, 63):
            n = nw + l - 1
            want = oracle.run(data, n, k, w, canonical=canonical, base_offset=off)
            c = b.run_device(d, n, out, base_offset=off)
            assert gpu.last_path() == sm.PATH_FUSED
            assert c == len(want) and np.array_equal(_dev(out, c), want), (nw, off)


@pytest.mark.gpu
@pytest.mark.parametrize("k,w,canonical", INSTANCES)
def test_default_lanes_and_window_ranges_vs_oracle(sm, oracle, gpu, k, w, canonical):
    """A run long enough for the default lanes (full tiles through the group-unrolled loop, a partial last tile, the
    tapered tail), whole and cut into window ranges that start and end mid-sequence, mid-tile and mid-group."""
    import torch
    n = 200_000_033
    data = oracle.gen_packed(32, n)
    d = torch.from_numpy(data).cuda()
    out = torch.zeros(n // 4, dtype=torch.int32, device="cuda")
    b = sm.Builder(k, w, canonical, 0)
    want = oracle.run_threads(data, n, k, w, canonical=canonical)
    c = b.run_device(d, n, out)
    assert gpu.last_path() == sm.PATH_FUSED
    assert c == len(want) and np.array_equal(_dev(out, c), want)
    # ranges (on a shorter prefix, so that the per-window oracle stays cheap)
    n2 = 3_000_017
    nw = n2 - (k + w - 1) + 1
    for off in (0, 3):
        for a, e in ((1, nw), (777_777, 777_778), (12_345, nw // 3 + 777), (78_848, 2 * 78_848), (1_000_001, nw - 13)):
            wr = _range_expect(oracle, data, n2, k, w, canonical, a, e, base_offset=off)
            c = b.run_device(d, n2, out, base_offset=off, win_begin=a, win_end=e)
            assert c == len(wr) and np.array_equal(_dev(out, c), wr), (off, a, e)


@pytest.mark.gpu
@pytest.mark.parametrize("k,w,canonical", INSTANCES)
def test_batch_of_contigs_vs_oracle(sm, oracle, gpu, k, w, canonical):
    """24 sequences of unequal lengths in one batch launch (the layout of a genome's contigs, scaled down): every sequence
    ends in a partial tile, some are shorter than a lane, one is shorter than a window; odd base offsets."""
    import torch
    rng = np.random.default_rng(7)
    lens = [int(x) for x in rng.integers(20_000, 900_000, size=20)] + [k + w - 2, k + w - 1, 77, 16_896 + k + w - 2]
    offs = [int(x) for x in rng.integers(0, 8, size=len(lens))]
    seqs = [oracle.gen_packed(100 + i, n + o) for i, (n, o) in enumerate(zip(lens, offs))]
    d_seqs = [torch.from_numpy(s).cuda() for s in seqs]
    out = torch.zeros(sum(lens) // 3 + 4096, dtype=torch.int32, device="cuda")
    got_offs = sm.run_batch_device(sm.Builder(k, w, canonical, 0), d_seqs, lens, out, base_offsets=offs)
    assert gpu.last_path() == sm.PATH_FUSED
    got = _dev(out, got_offs[-1])
    for i, (s, n, o) in enumerate(zip(seqs, lens, offs)):
        want = oracle.run(s, n, k, w, canonical=canonical, base_offset=o)
        part = got[got_offs[i]:got_offs[i + 1]]
        assert len(part) == len(want) and np.array_equal(part, want), (i, n, o)


@pytest.mark.gpu
@pytest.mark.parametrize("k,w,canonical", INSTANCES)
def test_low_complexity_vs_oracle(sm, oracle, gpu, k, w, canonical):
    """poly-A and short-period repeats: every window of a poly-A run emits a new position (the lane lists overflow and the
    tile is walked again storing directly - the redo walk is a fixed-k walk too), and on periodic sequence the leftmost and
    the rightmost minimum differ in most windows (the lazy strand vote's slow path)."""
    import torch
    n = 700_001
    rng = np.random.default_rng(9)
    random_part = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 50_000)].tobytes()
    for name, seq in (("poly-A", b"A" * n), ("poly-T", b"T" * n), ("AC", b"AC" * (n // 2 + 1)), ("ACG", b"ACG" * (n // 3 + 1)),
                      ("ACGTT", b"ACGTT" * (n // 5 + 1)), ("period 23", b"ACGGTCATTGACCGTTAAGCTAG" * (n // 23 + 1)),
                      ("random | poly-A | random", random_part + b"A" * 300_000 + random_part + b"GT" * 150_000)):
        seq = seq[:n]
        m = len(seq)
        data = oracle.pack_ascii(seq)
        d = torch.from_numpy(data).cuda()
        out = torch.zeros(m, dtype=torch.int32, device="cuda")
        for off in (0, 2):
            want = oracle.run(data, m - off, k, w, canonical=canonical, base_offset=off)
            c = sm.Builder(k, w, canonical, 0).run_device(d, m - off, out, base_offset=off)
            assert gpu.last_path() == sm.PATH_FUSED
            assert c == len(want) and np.array_equal(_dev(out, c), want), (name, off)


@pytest.mark.gpu
def test_neighbouring_k_takes_the_runtime_k_kernel_and_agrees(sm, oracle, gpu):
    """A k beside an instance's k has no fixed-k kernel: the launcher takes the run-time-k kernel of the same window size,
    as before.  Forward windows: k = 20 and 22; canonical windows need k + w - 1 odd, so the nearest legal ones: 19 and 23."""
    import torch
    n = 2_000_003
    data = oracle.gen_packed(33, n)
    d = torch.from_numpy(data).cuda()
    out = torch.zeros(n // 3, dtype=torch.int32, device="cuda")
    for k, canonical in ((20, False), (22, False), (19, True), (23, True)):
        assert sm.lib().mm_debug_fixed_k_kernel(k, 11, int(canonical)) == 0
        for off in (0, 1):
            want = oracle.run(data, n - off, k, 11, canonical=canonical, base_offset=off)
            c = sm.Builder(k, 11, canonical, 0).run_device(d, n - off, out, base_offset=off)
            assert gpu.last_path() == sm.PATH_FUSED
            assert c == len(want) and np.array_equal(_dev(out, c), want), (k, canonical, off)


_AB_SCRIPT = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "oracle"))
import numpy as np, torch
import mm_oracle as oracle
import simd_minimizers_amd as sm
n, k, w = 67_108_864 + 3, 21, 11
data = oracle.gen_packed(64, n)
d = torch.from_numpy(data).cuda()
L = sm.lib()
for canonical in (True,):
    res = []
    for no_kc in (False, True):
        if no_kc: os.environ["MM_NO_KC"] = "1"
        else: os.environ.pop("MM_NO_KC", None)
        assert L.mm_debug_fixed_k_kernel(k, w, int(canonical)) == (0 if no_kc else 1)
        out = torch.full((n // 4,), -1, dtype=torch.int32, device="cuda")
        c = sm.Builder(k, w, canonical, 0).run_device(d, n, out)
        assert sm.default_workspace(0).last_path() == sm.PATH_FUSED
        res.append((c, out))
    os.environ.pop("MM_NO_KC", None)
    assert res[0][0] == res[1][0] and res[0][0] > n // 8, (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]), "position buffers differ"
    want = oracle.run_fast(data, n, k, w, canonical=canonical, threads=8)
    assert res[0][0] == len(want) and np.array_equal(res[0][1][:res[0][0]].cpu().numpy().view(np.uint32), want)
    print("identical", canonical, res[0][0])
print("fixed-k ab ok")
"""


@pytest.mark.gpu
def test_fixed_k_and_runtime_k_kernels_are_byte_identical(sm, gpu):
    """64 Mbp of seeded sequence through the fixed-k instance and through the run-time-k kernel of the same window size:
    the counts and the WHOLE position buffers (the slots behind the count too) are equal, and equal to the oracle's.  The
    switch that leaves the fixed-k instances out inside one process (MM_NO_KC) exists in the experiments build only, so
    the comparison runs in a child process that loads that build."""
    lib = os.path.join(ROOT, "simd-minimizers_amd", "libsimd_minimizers_amd_exp.so")
    assert os.path.exists(lib), "experiments library not built (make -C simd-minimizers_amd/csrc exp)"
    env = dict(os.environ, MM_LIB_PATH=lib, MM_ENV_DYNAMIC="1")
    env.pop("MM_NO_KC", None)
    r = subprocess.run([sys.executable, "-c", _AB_SCRIPT, ROOT], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "fixed-k ab ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
