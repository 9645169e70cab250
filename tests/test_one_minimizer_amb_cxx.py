"""The C++ mirror of one minimizer per read that skips ambiguous bases: one_minimizer / one_minimizer_many over PackedNSeq
and a stream_fastx run with MM_FASTX_ONE_MINIMIZER that reads one_min in its callback
(tests/cxx/one_minimizer_amb_example.cpp).  Compiling it instantiates the templates without a device; running it needs
one."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cxx") / "one_minimizer_amb_example")
    libdir = os.path.join(ROOT, "simd-minimizers_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(HERE, "cxx", "one_minimizer_amb_example.cpp"), "-L" + libdir, "-lsimd_minimizers_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cxx_one_minimizer_amb_example_compiles(example):
    assert os.access(example, os.X_OK)


@pytest.mark.gpu
def test_cxx_one_minimizer_amb_example_runs(gpu, example):
    r = subprocess.run([example], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
