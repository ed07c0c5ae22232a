"""CPU-only: the host side of page documents (mygram-db_amd/csrc/mgx_documents.hpp: record and arena plan, and the host
restatement of the gather). tests/cpp/documents_plan_check.cpp is a stand-alone program over that header, built here with
g++ and -fsanitize=address,undefined; it checks every shape itself and exits non-zero on the first property that fails."""
import os
import subprocess

from pkg import ROOT


def test_documents_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "documents_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "documents_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("documents plan ok: ")
    assert int(r.stdout.split()[3]) > 47000  # the sweep ran whole
