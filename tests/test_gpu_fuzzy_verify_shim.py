"""-m gpu: builds tests/cpp/fuzzy_verify_test.cpp (FUZZY with verify_text through the C++17 shim: ExecuteBatch,
BatchExecutor, a table with a delta index) against libmygram_shim.so + libmygram_gpu.so and runs it."""
import os
import subprocess

import pytest

from pkg import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_shim_fuzzy_verify(tmp_path):
    exe = str(tmp_path / "fuzzy_verify_test")
    lib_dir = os.path.join(ROOT, "mygram-db_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "fuzzy_verify_test.cpp"),
                    "-L" + lib_dir, "-lmygram_shim", "-lmygram_gpu", "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
