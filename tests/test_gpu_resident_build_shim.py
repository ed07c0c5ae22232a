"""-m gpu: a shim table in build mode kDeviceResident (Index::SetBuildMode / mgxs_table_set_build_mode): its delta, its
compacted main index and the deltas after it come from mgx_index_build_device, columns, device index and attached texts in
one call. Two tables get the same changes, one builds on the host; after every step both answer alike, and as the oracle
does over an index built from the current documents (the Mirror / _check pattern of tests/test_gpu_device_build_shim.py,
restated)."""
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


def test_a_table_that_builds_resident_answers_as_one_that_builds_on_the_host():
    S = _shim()
    n = 3000
    corpus = mg.Corpus.synthetic(n, seed=5)
    pairs = [Pair(corpus=corpus), Pair(corpus=corpus)]
    for p in pairs:
        p.dev.ensure_text()
    host, res = S.Table(pairs[0].dev), S.Table(pairs[1].dev)
    host.set_build_mode(S.Table.BUILD_HOST)
    res.set_build_mode(S.Table.BUILD_DEVICE_RESIDENT)
    tables = (host, res)
    m = Mirror(corpus)
    rng = np.random.default_rng(6)
    c = pairs[0].dev.columns
    sizes = np.diff(c.offsets.astype(np.int64))
    grams = [c.gram(g).decode() for g in np.argsort(-sizes)[:40] if b" " not in c.gram(g)]
    words = [w.decode() for w in corpus.text(0).split()[:2] if len(w) >= 3]  # multi-gram words: text-level BM25
    assert words
    qs = []
    for i in range(10):
        terms = [grams[int(rng.integers(0, len(grams)))] for _ in range(int(rng.integers(1, 4)))]
        qs.append((terms, [grams[int(rng.integers(0, len(grams)))]] if i % 3 == 0 else []))
    # "zzqx": a term only changed documents hold
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

    def same_stats(delta):
        st = [t.mutation_stats() for t in tables]
        assert st[0] == st[1], st
        assert delta(st[0]["delta_documents"]), st

    add(200, novel=4)
    _check(tables, m.rebuilt(), qs)
    for j, d in enumerate(rng.choice(sorted(m.docs), 100, replace=False).tolist()):
        new = corpus.text(int(rng.integers(0, n))) + (b" zzqx" if j < 3 else b"")
        each(lambda t: t.update_document(d, m.docs[d], new))
        m.docs[d] = new
    for d in rng.choice(sorted(m.docs), 100, replace=False).tolist():
        each(lambda t: t.remove_document(d, m.docs[d]))
        del m.docs[d]
    _check(tables, m.rebuilt(), qs)
    same_stats(lambda k: k > 0)
    each(lambda t: t.compact())
    same_stats(lambda k: k == 0)
    _check(tables, m.rebuilt(), qs)
    add(50, novel=2)
    _check(tables, m.rebuilt(), qs)
    same_stats(lambda k: k == 50)
    ch, cr = host.build_counters(), res.build_counters()
    assert cr["device_resident"] >= 3 and cr["host"] == 0 and cr["device_columns"] == 0, cr  # deltas, the compaction, a delta
    assert ch["device_resident"] == 0 and ch["device_columns"] == 0 and ch["host"] == cr["device_resident"], (ch, cr)
    assert set(host.mutation_stats()) == {"main_documents", "delta_documents", "removed_from_main", "epoch"}


def test_four_grams_in_resident_mode_are_built_on_the_host():
    S = _shim()
    n = 400
    corpus = mg.Corpus.synthetic(n, seed=8)
    p = Pair(corpus=corpus, ngram=4)
    p.dev.ensure_text()
    t = S.Table(p.dev)
    t.set_build_mode(S.Table.BUILD_DEVICE_RESIDENT)  # the device call declines 4-grams: every build falls back to the host
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
    bc = t.build_counters()
    assert bc["device_resident"] == 0 and bc["device_columns"] == 0 and bc["host"] >= 2, bc


def test_set_device_build_still_selects_the_device_column_builder():
    S = _shim()
    n = 300
    corpus = mg.Corpus.synthetic(n, seed=4)
    p = Pair(corpus=corpus)
    p.dev.ensure_text()
    t = S.Table(p.dev)
    t.set_device_build(1)
    m = Mirror(corpus)
    for j in range(20):
        new = corpus.text(j) + b" zzqx"
        t.add_document(n + 1 + j, new)
        m.docs[n + 1 + j] = new
    _check((t,), m.rebuilt(), [(["zzqx"], [])])
    bc = t.build_counters()
    assert bc["device_columns"] >= 1 and bc["device_resident"] == 0 and bc["host"] == 0, bc
    t.set_device_build(0)
    t.add_document(n + 100, b"zzqx again")
    m.docs[n + 100] = b"zzqx again"
    _check((t,), m.rebuilt(), [(["zzqx"], [])])
    assert t.build_counters()["host"] >= 1
