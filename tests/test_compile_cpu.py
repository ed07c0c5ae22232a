"""CPU only: the query compiler (mygram-db_amd/csrc/mgx_compile.cpp) as a stand-alone program. The compiler's decisions —
wave_ok, flat, fast_score_ok, fz_op, merged count instructions, the dropped live-row operand, the slot a repeated gram
keeps — pick the kernel route, and GPU parity passes whichever route was taken; here every field of every compiled query
of a fixed catalogue is pinned."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mygram-db_amd", "csrc")


def test_compiled_catalogue_matches_the_recorded_listing(tmp_path):
    """tests/cpp/compile_test.cpp built with plain g++ together with mgx_compile.cpp and nothing else of the library:
    its listing (one entry per catalogue query and view variant: every QuerySpec field, or the return code and message)
    equals tests/cpp/compile_test.expected byte for byte, and the entries the program asserts by hand hold (exit 0).
    The expected listing was recorded from the compiler as it stood inside mgx_api.cpp, before it became this unit."""
    exe = tmp_path / "compile_test"
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "compile_test.cpp"), os.path.join(CSRC, "mgx_compile.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    with open(os.path.join(ROOT, "tests", "cpp", "compile_test.expected"), "rb") as f:
        want = f.read()
    got_entries, want_entries = r.stdout.split(b"== "), want.split(b"== ")
    assert len(want_entries) > 450
    for g, w in zip(got_entries, want_entries):
        assert g == w, "entry differs:\n--- got\n%s--- expected\n%s" % (g.decode(), w.decode())
    assert r.stdout == want
