"""CPU-only checks of the first-call interface: the per-flavour table of prebuilt window sizes, the run-time compiler's
counters and mm_plan_prepare's argument checks need no device, and the C++ mirror's example compiles against the
header alone."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NEW_FLAVOUR_WINDOWS = [5, 7, 11, 15, 17, 19, 21, 31]


def _flavour_sizes(L, canonical, reads, mode, sk, capacity=None):
    n = L.mm_prebuilt_flavour_window_sizes(canonical, reads, mode, sk, None, 0)
    cap = n if capacity is None else capacity
    buf = (C.c_uint32 * (n + 4))(*([0xDEAD] * (n + 4)))
    got = L.mm_prebuilt_flavour_window_sizes(canonical, reads, mode, sk, buf, cap)
    return got, list(buf)


def test_flavour_window_sizes_of_reads_mode(sm):
    L = sm.lib()
    for c in (0, 1):
        for mode, sk in ((sm.MM_CLOSED_SYNCMERS, 0), (sm.MM_OPEN_SYNCMERS, 0), (sm.MM_MINIMIZERS, 1)):
            n, buf = _flavour_sizes(L, c, 1, mode, sk)
            assert n == len(NEW_FLAVOUR_WINDOWS) and buf[:n] == NEW_FLAVOUR_WINDOWS, (c, mode, sk, buf)
            assert sm.prebuilt_flavour_window_sizes(bool(c), True, mode, bool(sk)) == NEW_FLAVOUR_WINDOWS


def test_flavour_window_sizes_agree_with_the_minimizer_list(sm):
    L = sm.lib()
    for c in (0, 1):
        reads_list = sm.prebuilt_window_sizes(bool(c), True)
        seq_list = sm.prebuilt_window_sizes(bool(c), False)
        assert set(NEW_FLAVOUR_WINDOWS) <= set(reads_list)
        n, buf = _flavour_sizes(L, c, 1, sm.MM_MINIMIZERS, 0)
        assert buf[:n] == reads_list
        # a sequence-mode instance carries all four flavours
        for mode, sk in ((0, 0), (1, 0), (2, 0), (0, 1)):
            n, buf = _flavour_sizes(L, c, 0, mode, sk)
            assert buf[:n] == seq_list, (c, mode, sk)
        # super-k-mers are defined for minimizers only
        assert L.mm_prebuilt_flavour_window_sizes(c, 1, sm.MM_CLOSED_SYNCMERS, 1, None, 0) == 0


def test_flavour_window_sizes_respect_capacity(sm):
    L = sm.lib()
    n, buf = _flavour_sizes(L, 1, 1, sm.MM_OPEN_SYNCMERS, 0, capacity=3)
    assert n == len(NEW_FLAVOUR_WINDOWS)
    assert buf[:3] == NEW_FLAVOUR_WINDOWS[:3] and all(x == 0xDEAD for x in buf[3:])
    n, buf = _flavour_sizes(L, 1, 1, sm.MM_OPEN_SYNCMERS, 0, capacity=-1)
    assert n == len(NEW_FLAVOUR_WINDOWS) and all(x == 0xDEAD for x in buf)


def test_jit_stats_and_prepare_without_a_device():
    """In a fresh process that has compiled nothing the counters are zero, and the null checks of mm_plan_prepare come
    before anything that touches a device."""
    code = ("import simd_minimizers_amd as sm, ctypes as C\n"
            "L = sm.lib()\n"
            "out = (C.c_uint64 * 4)(7, 7, 7, 7)\n"
            "assert L.mm_jit_stats(out) == 0 and list(out) == [0, 0, 0, 0], list(out)\n"
            "assert sm.jit_stats() == {'compiled': 0, 'from_disk': 0, 'hits': 0, 'failed': 0}\n"
            "assert L.mm_jit_stats(None) == sm.ERR['NULL']\n"
            "assert L.mm_plan_prepare(None, None, 1, None) == sm.ERR['NULL']\n"
            "rep = sm.PrepareReport(9, 9, 9, 9)\n"
            "p = sm.Plan(21, 11, True, 0, None)\n"
            "assert L.mm_plan_prepare(p.h, None, 1, C.byref(rep)) == sm.ERR['NULL']\n"
            "assert (rep.kernels, rep.compiled, rep.from_disk, rep.unavailable) == (0, 0, 0, 0)\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-3000:])


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """Builder::prepare of the C++ mirror: the example builds with warnings on, against the header alone."""
    exe = str(tmp_path_factory.mktemp("cxx") / "prepare_example")
    libdir = os.path.join(ROOT, "simd-minimizers_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(HERE, "cxx", "prepare_example.cpp"), "-L" + libdir, "-lsimd_minimizers_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cxx_prepare_example_compiles(example):
    assert os.access(example, os.X_OK)


@pytest.mark.gpu
def test_cxx_prepare_example_runs(gpu, example):
    """prepare, then reads + super-k-mers through run_many: the example checks its report, every read against the read
    alone, and that nothing was compiled after prepare (exit codes 2..7)."""
    r = subprocess.run([example], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
