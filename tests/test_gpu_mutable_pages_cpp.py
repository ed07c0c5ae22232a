"""-m gpu: builds tests/cpp/mutable_pages_test.cpp (queries without a page bound — limit 0, docid pages past 16384, deep
SORT _score — on a table with a delta index, through search_pipeline::ExecuteBatch: term, expression and FUZZY queries;
the SORT _score pages also at two (k1, b) pairs other than the defaults)
against libmygram_shim.so + libmygram_gpu.so and runs it."""
import os
import subprocess

import pytest

from pkg import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_mutable_unbounded_pages(tmp_path):
    exe = str(tmp_path / "mutable_pages_test")
    lib_dir = os.path.join(ROOT, "mygram-db_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "mutable_pages_test.cpp"),
                    "-L" + lib_dir, "-lmygram_shim", "-lmygram_gpu", "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
