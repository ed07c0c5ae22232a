"""-m gpu: builds tests/cpp/expr_verify_test.cpp (expression queries with verify_text and / or FUZZY leaves through the
C++17 shim: ExecuteBatch, BatchExecutor, a table with a delta index) against libmygram_shim.so + libmygram_gpu.so and
runs it on the case file of expr_verify_ref.shim_case(): the reference's two vectors, the FUZZY tree without verify_text,
and the same queries after AddDocument / UpdateDocument / RemoveDocument, against the answers for the current documents."""
import os
import subprocess

import pytest

import expr_verify_ref as EV
from pkg import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_shim_expr_verify(tmp_path):
    lines, summary = EV.shim_case()
    assert summary["runs"] >= 4 and summary["cut"] >= 4 and summary["delta_runs"] >= 1, summary
    case = tmp_path / "expr_verify_case.txt"
    case.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "expr_verify_test")
    lib_dir = os.path.join(ROOT, "mygram-db_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "expr_verify_test.cpp"),
                    "-L" + lib_dir, "-lmygram_shim", "-lmygram_gpu", "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
