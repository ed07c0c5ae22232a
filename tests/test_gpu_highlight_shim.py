"""-m gpu: builds tests/cpp/highlight_test.cpp (HIGHLIGHT through the C++17 shim: BatchQuery::highlight through
ExecuteBatch, BatchExecutor::WaitInto with two batches in flight, MicroBatcher, a table with a delta index and Compact())
against libmygram_shim.so + libmygram_gpu.so and runs it; then the C face (mgxs_search_highlight)."""
import ctypes as C
import os
import subprocess

import pytest

import highlight_ref as R
from pkg import ROOT, mg

pytestmark = pytest.mark.gpu


def test_cpp_shim_highlight(tmp_path):
    exe = str(tmp_path / "highlight_test")
    lib_dir = os.path.join(ROOT, "mygram-db_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "highlight_test.cpp"),
                    "-L" + lib_dir, "-lmygram_shim", "-lmygram_gpu", "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr


def test_c_face_search_highlight():
    from mygram_db_amd import _shim_capi as S
    L = S.load()
    texts = ["tokyo tower by the river", "osaka castle and the old bridge", "the tower of tokyo 東京タワー",
             "a garden far away from any tower at all, with a pond, a tea house and a long path of stones"]
    idx = mg.Index(corpus=mg.Corpus.from_texts(texts), first_doc_id=1, ngram_size=2, kanji_ngram_size=0, device=0)
    idx.ensure_text()
    t = S.Table(idx)
    terms = (C.c_char_p * 1)(b"tower")
    total, n = C.c_uint64(), C.c_uint32()
    docs = (C.c_uint32 * 10)()
    buf = C.create_string_buffer(4096)
    off = (C.c_uint32 * 11)()
    rc = L.mgxs_search_highlight(t._h, 1, C.cast(terms, C.c_void_p), 0, None, 0, 0, 10, 0, b"[", b"]", 20, 2,
                                 C.byref(total), C.byref(n), C.cast(docs, C.c_void_p), None, C.cast(buf, C.c_void_p), 4096,
                                 C.cast(off, C.c_void_p))
    assert rc == 0, L.mgxs_last_error()
    assert n.value == 3 and total.value == 3
    for k in range(n.value):
        want = R.generate(texts[docs[k] - 1].encode(), [b"tower"], 20, 2, b"[", b"]")
        assert buf.raw[off[k]:off[k + 1]] == want
