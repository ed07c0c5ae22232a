"""-m gpu: builds tests/cpp/facet_batch_test.cpp (FACET in a batch through the C++17 shim: BatchQuery::facet_columns
through ExecuteBatch, BatchExecutor with two batches in flight and MicroBatcher against ExecuteFacet per column, on a
static table, on a table with a delta index and after Compact()) against libmygram_shim.so + libmygram_gpu.so and runs
it; then the C face (mgxs_facet_columns against mgxs_facet per column)."""
import os
import subprocess

import numpy as np
import pytest

from pkg import ROOT, mg

pytestmark = pytest.mark.gpu


def test_cpp_shim_facet_batch(tmp_path):
    exe = str(tmp_path / "facet_batch_test")
    lib_dir = os.path.join(ROOT, "mygram-db_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "facet_batch_test.cpp"),
                    "-L" + lib_dir, "-lmygram_shim", "-lmygram_gpu", "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr


def test_c_face_facet_columns():
    from mygram_db_amd import _shim_capi as S
    rng = np.random.default_rng(5)
    words = ["tokyo", "osaka", "tower", "river", "castle", "bridge"]
    texts = [" ".join(rng.choice(words, 3)) for _ in range(700)]
    idx = mg.Index(corpus=mg.Corpus.from_texts(texts), first_doc_id=1, ngram_size=2, kanji_ngram_size=0, device=0)
    t = S.Table(idx)
    status = rng.integers(0, 5, 700)
    t.add_filter_column("status", "int64", status.tolist(), (rng.random(700) < 0.2).tolist())
    t.add_filter_column("city", "string", [words[i] for i in rng.integers(0, 3, 700)], [False] * 700)
    columns = ["city", "status", "city"]
    for terms, conditions, limit, offset in ((["tower"], [], 100, 0), ([], [], 2, 1), (["river"], [("status", ">", "1")], 100, 0),
                                             (["zzqx9"], [], 100, 0)):
        matched, per_column = t.facet_columns(columns, terms=terms, conditions=conditions, limit=limit, offset=offset)
        assert len(per_column) == 3
        for name, (total_values, page) in zip(columns, per_column):
            want = t.facet(name, terms=terms, conditions=conditions, limit=limit, offset=offset)
            assert (matched, total_values, page) == want, (terms, name)
    assert matched == 0
    with pytest.raises(Exception) as e:
        t.facet_columns(["city", "no_such_column"], terms=["tower"])
    assert "no_such_column" in str(e.value)
