"""K-mer values of every read in one launch: what needs no GPU - the exports, the refusals that come before the device
is touched, the kernel's read lookup run on the host (mm_debug_values_read_of), the C++ example's compile, and the lookup
header under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mm_values_u64_reads_device_async", "mm_values_u128_reads_device_async", "mm_values_u64_reads_host",
           "mm_values_u128_reads_host")


def test_entry_points_exported_and_wrapped(sm):
    L = sm.lib()
    for name in ENTRIES + ("mm_debug_values_read_of", "mm_values_reads_lds_stage"):
        assert hasattr(L, name), name
        assert name in sm.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    for name in ("values_reads_device", "values_reads_host", "values_read_of", "values_reads_lds_stage"):
        assert callable(getattr(sm, name)), name
    stage = sm.values_reads_lds_stage()
    assert 2 <= stage <= 8192  # (8 bytes per offset: at most the 64 KiB a workgroup may hold)


def test_null_workspace_and_bad_lengths_need_no_device(sm):
    L, E = sm.lib(), sm.ERR
    fake = C.c_void_p(4096)  # (never dereferenced: the refusals come first)
    a8 = np.zeros(16, dtype=np.uint8)
    a32 = np.zeros(4, dtype=np.uint32)
    a64 = np.zeros(4, dtype=np.uint64)
    p8, p32, p64 = sm._p(a8, C.c_uint8), sm._p(a32, C.c_uint32), sm._p(a64, C.c_uint64)
    for name in ENTRIES[:2]:
        assert getattr(L, name)(None, fake, 16, 0, 1, fake, 0, 21, 1, fake, fake, 4, fake) == E["NULL"], name
    for name in ENTRIES[2:]:
        assert getattr(L, name)(None, p8, 16, 0, 1, p64, 0, 21, 1, p32, p64, p64) == E["NULL"], name
    # decreasing starts / offsets are refused by the host entries before the workspace is looked at ... but after NULL:
    # with a NULL workspace the answer is MM_ERR_NULL whatever else is wrong
    bad = np.array([5, 3], dtype=np.uint64)
    assert L.mm_values_u64_reads_host(None, p8, 16, 0, 1, sm._p(bad, C.c_uint64), 0, 0, 1, p32, p64, p64) == E["NULL"]


def _want(offsets, idx):
    return np.searchsorted(offsets, idx, "right").astype(np.int64) - 1


def _boundaries(offsets):
    """Every boundary, the index before and the index behind it."""
    o = np.asarray(offsets, dtype=np.int64)
    idx = np.unique(np.concatenate([o, o + 1, np.maximum(o - 1, 0)]))
    return idx.astype(np.uint64)


@pytest.mark.parametrize("case", ["duplicates", "leading_empty", "trailing_empty", "single", "single_empty", "dense"])
def test_read_lookup_equals_searchsorted(sm, case):
    rng = np.random.default_rng(11)
    if case == "duplicates":  # many empty reads among the others
        counts = rng.integers(0, 4, 5000) * (rng.random(5000) < 0.3)
    elif case == "leading_empty":
        counts = np.concatenate([np.zeros(3000, dtype=np.int64), rng.integers(1, 50, 40)])
    elif case == "trailing_empty":
        counts = np.concatenate([rng.integers(1, 50, 40), np.zeros(3000, dtype=np.int64)])
    elif case == "single":
        counts = np.array([977])
    elif case == "single_empty":
        counts = np.array([0])
    else:
        counts = rng.integers(1, 3000, 300)
    offsets = np.zeros(len(counts) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(counts)
    total = int(offsets[-1])
    idx = _boundaries(offsets)
    if total:
        idx = np.concatenate([idx, rng.integers(0, total, 4000).astype(np.uint64)])
    got = sm.values_read_of(offsets, idx)
    assert np.array_equal(got, _want(offsets, idx)), case
    # inside the range every answer is a NON-EMPTY read that holds the index
    inside = idx < total
    r = got[inside]
    assert np.all(offsets[r] <= idx[inside]) and np.all(idx[inside] < offsets[r + 1])


def test_cxx_values_many_example_compiles(sm):
    """tests/cxx/values_many_example.cpp builds against the header-only mirror and the in-tree library."""
    cxx = os.path.join(ROOT, "tests", "cxx")
    subprocess.run(["make", "-C", cxx, "-f", "values_many_example.mk"], check=True, capture_output=True)
    assert os.path.exists(os.path.join(cxx, "values_many_example"))


LOOKUP_MAIN = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "mm_values_reads.h"
int main() {
    uint64_t x = 88172645463325252ull;
    for (int round = 0; round < 200; ++round) {
        const size_t n_reads = 1 + (size_t)(x % 300);
        std::vector<uint64_t> off(n_reads + 1, 0);
        for (size_t r = 0; r < n_reads; ++r) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            off[r + 1] = off[r] + ((x >> 20) % 3 ? 0 : (x >> 40) % 17);
        }
        for (uint64_t i = 0; i <= off[n_reads] + 1; ++i) {
            const uint64_t r = mm::values_read_of(off.data(), (uint64_t)0, (uint64_t)n_reads, i);
            size_t want = 0;
            for (size_t q = 0; q <= n_reads; ++q)
                if (off[q] <= i) want = q;
            if (r != want) { printf("mismatch at %llu\n", (unsigned long long)i); return 1; }
        }
    }
    return 0;
}
"""


def test_lookup_header_under_sanitizers(tmp_path):
    """The lookup header in a stand-alone host program (its own main) built with -fsanitize=address,undefined and run
    directly: every index of random offset tables against a linear scan."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "lookup_main.cpp"
    src.write_text(LOOKUP_MAIN)
    exe = tmp_path / "lookup_main"
    inc = os.path.join(ROOT, "simd-minimizers_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc,
                    "-o", str(exe), str(src)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
