"""-m gpu: builds tests/cpp/batch_conditions_test.cpp (FILTER conditions with a fresh literal per request through
BatchExecutor: results per document from the host values, the main index's mgx_index_memory_bytes unchanged after 3200
distinct literals, one cached row for `=` on a string value that exists, range conditions on a table with a delta)
against libmygram_shim.so + libmygram_gpu.so and runs it."""
import os
import subprocess

import pytest

from pkg import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_batch_conditions_through_the_executor(tmp_path):
    exe = str(tmp_path / "batch_conditions_test")
    lib_dir = os.path.join(ROOT, "mygram-db_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "batch_conditions_test.cpp"),
                    "-L" + lib_dir, "-lmygram_shim", "-lmygram_gpu", "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
