"""-m gpu: builds tests/cpp/documents_test.cpp (page documents through the C++17 shim: BatchQuery::return_documents and
document_columns through ExecuteBatch, BatchExecutor with two batches in flight and MicroBatcher, and
storage::DocumentStore::GetDocumentsBatch / GetPrimaryKeysBatch over an id list, on a mutable table: after the build, with
a delta index and after Compact()) against libmygram_shim.so + libmygram_gpu.so and runs it; then the C face
(mgxs_search_documents against the host arrays the table was given)."""
import os
import subprocess

import numpy as np
import pytest

from pkg import ROOT, mg

pytestmark = pytest.mark.gpu


def test_cpp_shim_documents(tmp_path):
    exe = str(tmp_path / "documents_test")
    lib_dir = os.path.join(ROOT, "mygram-db_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "documents_test.cpp"),
                    "-L" + lib_dir, "-lmygram_shim", "-lmygram_gpu", "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr


def test_c_face_search_documents():
    from mygram_db_amd import _shim_capi as S
    rng = np.random.default_rng(6)
    words = ["tokyo", "osaka", "tower", "river", "castle", "bridge"]
    n = 700
    texts = [" ".join(rng.choice(words, 3)) for _ in range(n)]
    idx = mg.Index(corpus=mg.Corpus.from_texts(texts), first_doc_id=1, ngram_size=2, kanji_ngram_size=0, device=0)
    idx.ensure_text()  # (SORT _score of a term longer than one n-gram counts it in the texts)
    keys = [None if i % 50 == 0 else (b"007" if i == 7 else b"k" * (i % 90) + b"%d" % i) for i in range(n)]
    idx.device_index.attach_primary_key_bytes(keys)
    idx.device_index.set_primary_keys(keys)
    t = S.Table(idx)
    status = rng.integers(-5, 5, n)
    status_null = rng.random(n) < 0.2
    city = [words[i] for i in rng.integers(0, 3, n)]
    t.add_filter_column("status", "int64", status.tolist(), status_null.tolist())
    t.add_filter_column("city", "string", city, [False] * n)
    rank = {w: r for r, w in enumerate(sorted(set(city)))}
    columns = ["city", "status", "city"]
    for kw in (dict(sort_by_score=True, limit=10), dict(sort_primary_key=True, descending=True, limit=100),
               dict(sort_column="status", descending=False, limit=40, offset=5), dict(limit=1024, descending=False)):
        total, docs, rows = t.search_documents(["tower"], columns, **kw)
        assert total > 100 and len(docs) == len(rows) == min(total, kw["limit"])
        for doc, row in zip(docs.tolist(), rows):
            i = doc - 1
            key, values, mask = row
            assert key == (keys[i] if keys[i] else None), doc
            assert mask == (2 if status_null[i] else 0), doc
            assert values[0] == values[2] == rank[city[i]], doc
            assert status_null[i] or int(values[1]) == int(status[i]) % (1 << 64), doc
    total, docs, rows = t.search_documents(["river"], [], limit=5)  # keys only
    assert len(rows) == 5 and all(len(r[1]) == 0 for r in rows)
    assert [r[0] for r in rows] == [keys[d - 1] if keys[d - 1] else None for d in docs.tolist()]
    assert t.search_documents(["zzqx9"], columns)[0] == 0
    with pytest.raises(Exception) as e:
        t.search_documents(["tower"], ["city", "no_such_column"])
    assert "no_such_column" in str(e.value)
    with pytest.raises(Exception):
        t.search_documents(["tower"], columns, limit=2000)
