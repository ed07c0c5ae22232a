"""-m gpu: builds tests/cpp/funnel_test.cpp against libmygram_shim.so + libmygram_gpu.so and runs it on a case file
written here: a 20 000-document table that changes in three rounds (removes, updates, adds, delta documents changing,
Compact()), and at every checkpoint 13 queries (1-3-term AND with and without NOT terms, a term only changed documents
hold, a term whose documents were all removed, typed conditions, two expressions — one a lone NOT —, a FUZZY query, and a
two-term query whose terms swap their size order) whose total, four funnel counters and full doc-id list the CPU oracle
computed over the documents current at that checkpoint — never a second device index."""
import os
import subprocess

import pytest

import funnel_util as FU
from pkg import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_funnel_counters_of_a_changed_table(tmp_path):
    lines, summary = FU.mutable_case()  # (asserts that the oracle's term order of the swap query flips)
    case = tmp_path / "funnel_case.txt"
    case.write_text("\n".join(lines) + "\n", encoding="utf-8")
    exe = str(tmp_path / "funnel_test")
    lib_dir = os.path.join(ROOT, "mygram-db_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "funnel_test.cpp"),
                    "-L" + lib_dir, "-lmygram_shim", "-lmygram_gpu", "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=300)
    print(summary, r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "3 checkpoints, %d results compared, 0 failed" % (3 * 3 * summary["queries"]) in r.stdout
