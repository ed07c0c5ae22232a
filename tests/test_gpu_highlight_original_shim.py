"""-m gpu: builds tests/cpp/highlight_original_test.cpp (HIGHLIGHT from original texts through the C++17 shim: the
reference's vectors through Index + ExecuteBatch, BatchExecutor, MicroBatcher, a table that changes and Compact(), an
original that is not valid UTF-8, the pinned refusals) against libmygram_shim.so + libmygram_gpu.so and runs it; then the C
face (mgxs_search_highlight) over an index with originals attached."""
import ctypes as C
import os
import subprocess

import pytest

import highlight_original_ref as O
import highlight_ref as R
from pkg import ROOT, mg

pytestmark = pytest.mark.gpu


def test_cpp_shim_highlight_original(tmp_path):
    exe = str(tmp_path / "highlight_original_test")
    lib_dir = os.path.join(ROOT, "mygram-db_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "highlight_original_test.cpp"),
                    "-L" + lib_dir, "-lmygram_shim", "-lmygram_gpu", "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout


def test_c_face_search_highlight_from_originals():
    from mygram_db_amd import _shim_capi as S
    L = S.load()
    originals = ["Tokyo TOWER by the River", "Osaka castle", "The Tower of TOKYO", "no original here: tower"]
    texts = [o.lower() for o in originals]
    idx = mg.Index(corpus=mg.Corpus.from_texts(texts), first_doc_id=1, ngram_size=2, kanji_ngram_size=0, device=0)
    idx.attach_original_text(originals[:3] + [None], [1, 1, 1, 0])
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
    assert sorted(docs[:n.value]) == [1, 3, 4]
    for k in range(n.value):
        d = docs[k] - 1
        if d == 3:
            want = R.generate(texts[d].encode(), [b"tower"], 20, 2, b"[", b"]")
        else:
            o = originals[d].encode()
            segments = [(c, c.lower()) for c in O.split_characters(o)]
            want = O.generate_original(o, texts[d].encode(), segments, [b"tower"], 20, 2, b"[", b"]")
            assert b"[T" in want
        assert buf.raw[off[k]:off[k + 1]] == want


def test_a_table_from_a_dump_takes_the_stores_originals():
    """tests/golden/dump_v2_small.bin: the store section ("MGDS" v3) holds every document's original text — its text in
    upper case — so a table restored with Index::FromDump answers HIGHLIGHT with what the user wrote; engine.Index.from_dump
    hands the same originals out."""
    import json
    from mygram_db_amd import _shim_capi as S
    L = S.load()
    raw = open(os.path.join(ROOT, "tests", "golden", "dump_v2_small.bin"), "rb").read()
    exp = json.load(open(os.path.join(ROOT, "tests", "golden", "dump_v2_expected.json"), encoding="utf-8"))
    dev = mg.Index.from_dump(raw, exp["table"])
    first = dev.columns.first_doc_id
    for k, o in enumerate(dev.dump_original_texts):
        t = exp["texts"].get(str(first + k))
        assert o == (t.upper().encode() if t is not None else None)
    t = S.Table.from_dump(raw, exp["table"])
    for word in ("tokyo", "東京"):
        terms = (C.c_char_p * 1)(word.encode())
        total, n = C.c_uint64(), C.c_uint32()
        docs = (C.c_uint32 * 64)()
        buf = C.create_string_buffer(1 << 16)
        off = (C.c_uint32 * 65)()
        rc = L.mgxs_search_highlight(t._h, 1, C.cast(terms, C.c_void_p), 0, None, 0, 0, 64, 0, b"[", b"]", 12, 2,
                                     C.byref(total), C.byref(n), C.cast(docs, C.c_void_p), None, C.cast(buf, C.c_void_p),
                                     1 << 16, C.cast(off, C.c_void_p))
        assert rc == 0, L.mgxs_last_error()
        assert n.value >= 3
        for k in range(n.value):
            text = exp["texts"][str(docs[k])]
            o = text.upper().encode()
            segments = [(c, c.decode().lower().encode()) for c in O.split_characters(o)]
            want = O.generate_original(o, text.encode(), segments, [word.encode()], 12, 2, b"[", b"]")
            assert ("[%s]" % word.upper()).encode() in want
            assert buf.raw[off[k]:off[k + 1]] == want
