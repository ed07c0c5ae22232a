"""-m gpu: builds tests/cpp/mutation_commit_test.cpp (a mutable table commits recorded changes in one step: failed
applications and compactions under injected allocation failures, a failure reported until it is cured, writers beside
queries and compactions, the index-less SortByScore after delta builds) against libmygram_shim.so + libmygram_gpu.so
and runs it."""
import os
import subprocess

import pytest

from pkg import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_mutation_commit(tmp_path):
    exe = str(tmp_path / "mutation_commit_test")
    lib_dir = os.path.join(ROOT, "mygram-db_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "mutation_commit_test.cpp"),
                    "-L" + lib_dir, "-lmygram_shim", "-lmygram_gpu", "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
