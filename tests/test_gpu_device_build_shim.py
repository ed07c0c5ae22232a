"""-m gpu: a shim table whose column arrays are built on the device (Index::SetDeviceBuild / mgxs_table_set_device_build).
Two tables get the same changes, one builds its delta and its compacted main index with mgx_columns_build_device, the
other on the host; after every step both answer alike, and as the oracle does over an index built from the current
documents (the Mirror / _check pattern of tests/test_gpu_mutable.py, restated)."""
import numpy as np
import pytest

from gpu_util import Pair
from pkg import mg

pytestmark = pytest.mark.gpu
Query = mg.engine.Query


def _shim():
    from mygram_db_amd import _shim_capi as S
    return S


class Mirror:
    """The table's current documents, changed alongside the shim tables."""

    def __init__(self, corpus):
        self.docs = {i + 1: corpus.text(i) for i in range(corpus.n_docs)}

    def rebuilt(self, ngram=2):
        return Pair(docs=sorted(self.docs.items()), ngram=ngram, kanji=0)


def _check(tables, want_pair, qs):
    for terms, nots in qs:
        for desc in (True, False):
            want = want_pair.oracle_query(Query(terms, not_terms=nots, sort_score=True, descending=desc, limit=10))
            got = [t.search(terms, not_terms=nots, sort_by_score=True, descending=desc, limit=10) for t in tables]
            for total, docs, scores in got:
                assert total == want[0], (terms, nots, desc, total, want[0])
                assert np.array_equal(docs, want[1]), (terms, nots, desc)
                assert np.array_equal(scores, want[2]), (terms, nots, desc, scores, want[2])
            assert np.array_equal(got[0][1], got[-1][1]) and np.array_equal(got[0][2], got[-1][2])
            want = want_pair.oracle_query(Query(terms, not_terms=nots, descending=desc, limit=7))
            for t in tables:
                total, docs, _ = t.search(terms, not_terms=nots, descending=desc, limit=7)
                assert total == want[0] and np.array_equal(docs, want[1]), (terms, nots, desc)


def test_a_table_that_builds_on_the_device_answers_as_one_that_builds_on_the_host():
    S = _shim()
    n = 3000
    corpus = mg.Corpus.synthetic(n, seed=5)
    pairs = [Pair(corpus=corpus), Pair(corpus=corpus)]
    for p in pairs:
        p.dev.ensure_text()
    host, dev = S.Table(pairs[0].dev), S.Table(pairs[1].dev)
    dev.set_device_build(1)
    tables = (host, dev)
    m = Mirror(corpus)
    rng = np.random.default_rng(6)
    c = pairs[0].dev.columns
    sizes = np.diff(c.offsets.astype(np.int64))
    grams = [c.gram(g).decode() for g in np.argsort(-sizes)[:40] if b" " not in c.gram(g)]
    words = [w.decode() for w in corpus.text(0).split()[:2] if len(w) >= 3]
    qs = []
    for i in range(10):
        terms = [grams[int(rng.integers(0, len(grams)))] for _ in range(int(rng.integers(1, 4)))]
        qs.append((terms, [grams[int(rng.integers(0, len(grams)))]] if i % 3 == 0 else []))
    qs += [([w], []) for w in words] + [(["zzqx"], []), ([grams[0], "zzqx"], [])]
    _check(tables, pairs[0], qs[:4])

    def each(fn):
        for t in tables:
            fn(t)

    def add(k, novel):
        top = max(max(m.docs), n)
        for j in range(k):
            new = corpus.text(int(rng.integers(0, n))) + (b" zzqx tail" if j < novel else b"")
            each(lambda t: t.add_document(top + 1 + j, new))
            m.docs[top + 1 + j] = new

    add(200, novel=4)
    for j, d in enumerate(rng.choice(sorted(m.docs), 100, replace=False).tolist()):
        new = corpus.text(int(rng.integers(0, n))) + (b" zzqx" if j < 3 else b"")
        each(lambda t: t.update_document(d, m.docs[d], new))
        m.docs[d] = new
    for d in rng.choice(sorted(m.docs), 100, replace=False).tolist():
        each(lambda t: t.remove_document(d, m.docs[d]))
        del m.docs[d]
    _check(tables, m.rebuilt(), qs)
    st = [t.mutation_stats() for t in tables]
    assert st[0] == st[1] and st[0]["delta_documents"] > 0, st
    each(lambda t: t.compact())
    st = [t.mutation_stats() for t in tables]
    assert st[0] == st[1] and st[0]["delta_documents"] == 0, st
    _check(tables, m.rebuilt(), qs)
    add(50, novel=2)
    _check(tables, m.rebuilt(), qs)
    st = [t.mutation_stats() for t in tables]
    assert st[0] == st[1] and st[0]["delta_documents"] == 50, st


def test_four_grams_are_built_on_the_host_behind_the_switch():
    S = _shim()
    n = 400
    corpus = mg.Corpus.synthetic(n, seed=8)
    p = Pair(corpus=corpus, ngram=4)
    p.dev.ensure_text()
    t = S.Table(p.dev)
    t.set_device_build(1)  # the device builder declines 4-grams: every build of this table falls back to the host
    m = Mirror(corpus)
    c = p.dev.columns
    sizes = np.diff(c.offsets.astype(np.int64))
    grams = [c.gram(g).decode() for g in np.argsort(-sizes)[:12] if b" " not in c.gram(g)]
    qs = [([g], []) for g in grams[:4]] + [(["zzqxy"], []), ([grams[0]], [grams[1]])]
    for j in range(30):
        new = corpus.text(j) + b" zzqxy"
        t.add_document(n + 1 + j, new)
        m.docs[n + 1 + j] = new
    _check((t,), m.rebuilt(ngram=4), qs)
    assert t.mutation_stats()["delta_documents"] == 30
    t.compact()
    assert t.mutation_stats()["delta_documents"] == 0
    _check((t,), m.rebuilt(ngram=4), qs)
