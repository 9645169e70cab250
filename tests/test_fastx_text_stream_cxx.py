"""The C++ mirror of the byte-text FASTA stream: Builder::stream_fasta_text (tests/cxx/fastx_text_stream_example.cpp; a
file -> the stream -> per-record positions, values and one minimizer, the first batch against the one-shot calls).
Compiling it instantiates the templates without a device; running it needs one."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cxx") / "fastx_text_stream_example")
    libdir = os.path.join(ROOT, "simd-minimizers_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(HERE, "cxx", "fastx_text_stream_example.cpp"), "-L" + libdir, "-lsimd_minimizers_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cxx_fastx_text_stream_example_compiles(example):
    assert os.access(example, os.X_OK)


@pytest.mark.gpu
def test_cxx_fastx_text_stream_example_runs(gpu, example):
    r = subprocess.run([example], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "batches ok" in r.stdout
