"""-m gpu: builds tests/cpp/column_sort_test.cpp (SORT <filter column> through the C++17 shim: BatchQuery::sort_column
through ExecuteBatch, BatchExecutor with two batches in flight, MicroBatcher, the reference's vectors as tables, a table
with a delta index and Compact()) against libmygram_shim.so + libmygram_gpu.so and runs it; then the C face
(mgxs_search_sorted)."""
import os
import subprocess

import numpy as np
import pytest

from pkg import ROOT, mg

import column_sort_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def test_cpp_shim_column_sort(tmp_path):
    exe = str(tmp_path / "column_sort_test")
    lib_dir = os.path.join(ROOT, "mygram-db_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "column_sort_test.cpp"),
                    "-L" + lib_dir, "-lmygram_shim", "-lmygram_gpu", "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr


def test_c_face_search_sorted():
    from mygram_db_amd import _shim_capi as S
    texts = ["tokyo tower", "osaka castle tower", "the tower of tokyo", "a garden", "tower bridge", "old tower"]
    idx = mg.Index(corpus=mg.Corpus.from_texts(texts), first_doc_id=1, ngram_size=2, kanji_ngram_size=0, device=0)
    t = S.Table(idx)
    year = [1958, None, 1958, 2000, 1894, -3]
    t.add_filter_column("year", "int32", [0 if y is None else y for y in year], is_null=[y is None for y in year])
    hits = [d for d in range(1, 7) if "tower" in texts[d - 1]]
    values = {d: (None if year[d - 1] is None else ("int32", year[d - 1])) for d in hits}
    for descending in (False, True):
        for limit, offset in ((10, 0), (2, 1)):
            total, docs = t.search_sorted(["tower"], "Year", descending=descending, limit=limit, offset=offset)
            assert total == len(hits)
            want = R.apply_offset_limit(R.sort_entries(hits, values, not descending), offset, limit)
            assert docs.tolist() == want, (descending, limit, offset)
    with pytest.raises(Exception) as e:
        t.search_sorted(["tower"], "decade")
    assert "not found" in str(e.value) and "decade" in str(e.value)
    assert np.array_equal(t.search(["tower"], descending=False, limit=10)[1], np.asarray(hits, np.uint32))  # mgxs_search as before
