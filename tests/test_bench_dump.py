"""bench.py --dump-outputs: the file layout two builds are compared by (no device needed)."""
import numpy as np

import bench


def test_dump_outputs_writes_float64_rows_with_empty_slots_zeroed(tmp_path):
    n_docs = np.array([0, 1, 3, 10], np.uint32)
    totals = np.array([0, 1, 3, 12345678], np.uint64)
    docs = np.full((4, 10), 7, np.uint32)  # stale entries past n_docs, as a reused result buffer holds them
    docs[3] = np.arange(9_999_990, 10_000_000)
    scores = np.full((4, 10), 2.5)
    bench.dump_outputs(str(tmp_path / "out"), totals, n_docs, docs, scores)
    got = {p.stem: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert sorted(got) == ["docs", "n_docs", "scores", "totals"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["totals"].tolist() == totals.tolist() and got["n_docs"].tolist() == n_docs.tolist()
    for i, k in enumerate(n_docs):
        assert got["docs"][i, :k].tolist() == docs[i, :k].tolist() and not got["docs"][i, k:].any()
        assert got["scores"][i, :k].tolist() == scores[i, :k].tolist() and not got["scores"][i, k:].any()
