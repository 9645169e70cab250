"""FASTA records longer than a chunk through the C ABI and the C++ mirror (tests/cxx/fastx_long_example.cpp:
mm_fastx_stream_pieces and Builder::stream_fastx with an on_batch that takes the pieces, joined and compared with the
one-shot call).  Compiling it instantiates the template without a device; running it needs one."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cxx") / "fastx_long_example")
    libdir = os.path.join(ROOT, "simd-minimizers_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(HERE, "cxx", "fastx_long_example.cpp"), "-L" + libdir, "-lsimd_minimizers_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cxx_fastx_long_example_compiles(example):
    assert os.access(example, os.X_OK)


@pytest.mark.gpu
def test_cxx_fastx_long_example_runs(gpu, example):
    r = subprocess.run([example], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "fastx_long_example: OK" in r.stdout
