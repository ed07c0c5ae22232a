"""CPU-only: the page plan of the bitmap group's fetch (mygram-db_amd/csrc/mgx_pages.hpp: pages, what each side
materialises, runs, top-k jobs and the scratch layout). tests/cpp/pages_plan_check.cpp is a stand-alone program over that
header, built here with g++ and -fsanitize=address,undefined; it checks every case itself and exits non-zero on the first
property that fails."""
import os
import subprocess

from pkg import ROOT


def test_pages_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "pages_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "pages_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("pages plan ok: ")
    assert int(r.stdout.split()[3]) > 4000  # the hand-stated cases and the random sweep ran whole
