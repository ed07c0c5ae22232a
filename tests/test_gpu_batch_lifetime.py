"""-m gpu: a PreparedBatch and its DeviceIndex that die together. A batch keeps its index alive, so reference counting
destroys the batch first. The cycle collector gives no such order: a caught MgxError's traceback holds the frame that
holds the batch, and once the index is unreachable too, either __del__ may run first. mgx_batch_destroy reads its index,
so the index takes its live batches with it (DeviceIndex._live_batches)."""
import numpy as np
import pytest

from pkg import mg

pytestmark = pytest.mark.gpu
Query = mg.engine.Query


def _dense_terms(idx, n):
    c = idx.columns
    sizes = np.diff(c.offsets.astype(np.int64))
    order = [g for g in np.argsort(-sizes, kind="stable") if b" " not in c.gram(g)]
    return [c.gram(g).decode() for g in order[:n]]


def test_an_index_finalised_before_its_batch_takes_the_batch_with_it():
    idx = mg.Index(corpus=mg.Corpus.synthetic(3_000, seed=5))
    terms = _dense_terms(idx, 2)
    qs = [Query(terms, sort_score=True, limit=5), Query([terms[0]], limit=5)]
    want = idx.search_batch(qs)
    a, b = idx.prepare(qs), idx.prepare(qs)
    a.execute()
    dev = idx.device_index
    assert sorted(dev._live_batches) == sorted([a._h.value, b._h.value])
    del a  # the usual order: the batch alone
    assert list(dev._live_batches) == [b._h.value]
    dev.__del__()  # the collector's other order: the index first, and with it the batch that is left
    assert dev._h is None and not dev._live_batches
    b.__del__()  # nothing is left to destroy, and the dead index is not read
    assert b._h is None
    # the next index on this thread meets no error left behind (its first scored batch builds contribution tables)
    other = mg.Index(corpus=mg.Corpus.synthetic(3_000, seed=5))
    got = other.search_batch(qs)
    for g, w in zip(got, want):
        assert g.total == w.total and g.docs.tolist() == w.docs.tolist() and np.array_equal(g.scores, w.scores)
