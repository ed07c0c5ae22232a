"""-m gpu: builds tests/cpp/primary_key_sort_test.cpp (SORT by primary key through the C++17 shim: BatchQuery::
sort_primary_key and the primary-key column's name through ExecuteBatch, BatchExecutor with two batches in flight and
MicroBatcher, on tables with a delta index — numeric keys, one string key, string keys on both sides — and after
Compact()) against libmygram_shim.so + libmygram_gpu.so and runs it; then the C face (mgxs_search_by_primary_key) on an
adopted index and on a table loaded from the golden dump, whose keys "pk<doc id>" sort bytewise."""
import json
import os
import subprocess

import numpy as np
import pytest

from pkg import ROOT, mg

import primary_key_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu


def test_cpp_shim_primary_key_sort(tmp_path):
    exe = str(tmp_path / "primary_key_sort_test")
    lib_dir = os.path.join(ROOT, "mygram-db_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "primary_key_sort_test.cpp"),
                    "-L" + lib_dir, "-lmygram_shim", "-lmygram_gpu", "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, MGX_VERBOSE="1"))
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "[mgx] key merge: " in r.stderr  # the tables with string keys were merged by key string


def test_c_face_search_by_primary_key():
    from mygram_db_amd import _shim_capi as S
    texts = ["tokyo tower", "osaka castle tower", "the tower of tokyo", "a garden", "tower bridge", "old tower"]
    keys = [b"10", b"9", b"pk", None, b"007", b"7"]
    idx = mg.Index(corpus=mg.Corpus.from_texts(texts), first_doc_id=1, ngram_size=2, kanji_ngram_size=0, device=0)
    idx.device_index.set_primary_keys(keys)
    t = S.Table(idx)
    hits = [d for d in range(1, 7) if "tower" in texts[d - 1]]
    for descending in (False, True):
        for limit, offset in ((10, 0), (2, 1), (3, 9)):
            total, docs = t.search_by_primary_key(["tower"], descending=descending, limit=limit, offset=offset)
            assert total == len(hits)
            assert docs.tolist() == P.page(hits, lambda d: keys[d - 1], not descending, offset, limit), (descending, limit, offset)
    assert t.search_by_primary_key(["tower"], descending=False, limit=10)[1].tolist() == [5, 6, 2, 1, 3]  # 007 = 7 < 9 < 10 < "pk"
    assert np.array_equal(t.search(["tower"], descending=False, limit=10)[1], np.asarray(hits, np.uint32))  # mgxs_search as before


def test_a_dump_keeps_its_primary_keys():
    """tests/golden/dump_v2_small.bin: every document's key is "pk<doc id>", so key order is bytewise — "pk10" sorts
    before "pk9" — and differs from doc-id order. Through Index::FromDump (the C face) and engine.Index.from_dump."""
    from mygram_db_amd import _shim_capi as S
    raw = open(os.path.join(ROOT, "tests", "golden", "dump_v2_small.bin"), "rb").read()
    exp = json.load(open(os.path.join(ROOT, "tests", "golden", "dump_v2_expected.json"), encoding="utf-8"))
    ids = [int(d) for d in exp["ids"]]
    t = S.Table.from_dump(raw, exp["table"])
    dev = mg.Index.from_dump(raw, exp["table"])
    first = min(ids)
    assert [k for k in dev.dump_primary_keys if k is not None] == [b"pk%d" % d for d in ids]
    for term in ("gamma", "tokyo"):
        hits = [d for d in ids if term in exp["texts"][str(d)]]
        assert len(hits) > 5 and any(d < 10 for d in hits) and any(d >= 10 for d in hits)
        for descending in (False, True):
            want = P.page(hits, lambda d: b"pk%d" % d, not descending, 0, 100)
            assert want != sorted(hits, reverse=descending)  # not the doc-id page
            total, docs = t.search_by_primary_key([term], descending=descending, limit=100)
            assert total == len(hits) and docs.tolist() == want, (term, descending)
            g = dev.search_batch([mg.engine.Query([term], sort_primary_key=True, descending=descending, limit=100)])[0]
            assert g.docs.tolist() == want and dev.dump_primary_keys[want[0] - first] == b"pk%d" % want[0]
