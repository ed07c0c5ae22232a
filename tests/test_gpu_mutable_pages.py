"""-m gpu: unbounded and deep result pages on a table with a delta index. Queries without a page bound — docid pages with
limit 0 or limit > 16384, SORT _score pages past offset+limit 1024 — are merged across the main and the delta index at
fetch time (rank_merge_kernel). The bar, as in test_gpu_mutable.py: after any sequence of changes, pages, totals and
BM25 scores equal those of an index built from the table's current documents, bit for bit. Also deep SORT _score with
text-level terms (words longer than one n-gram), on a static and on a changed table."""
import numpy as np
import pytest

from gpu_util import Pair
from oracle import filters as F
from pkg import mg

pytestmark = pytest.mark.gpu
Query = mg.engine.Query

N = 40_000
BIG = ["ee", "te", "et", "tx"]      # single grams held by more than 16384 documents of the corpus
WORDS = ["rveqe", "ths", "eeo"]     # text-level terms on the bigram index (>= 3 bytes)


def _shim():
    from mygram_db_amd import _shim_capi as S
    return S


class Mirror:
    """The table's current documents (and their filter values), changed alongside the shim table."""

    def __init__(self, corpus, status):
        self.docs = {i + 1: corpus.text(i) for i in range(corpus.n_docs)}
        self.status = {i + 1: int(status[i]) for i in range(corpus.n_docs)}

    def rebuilt(self):
        return Pair(docs=sorted(self.docs.items()), ngram=2, kanji=0)

    def columns(self):
        return {"status": lambda doc: ("int32", self.status[doc])}


def _score_page(want, terms, nots, desc, limit, offset, conds=None, columns=None):
    """(total, docs, scores) of SORT _score from the oracle over the rebuilt index; FILTER conditions keep the order."""
    total, docs, scores, _ = want.oracle_query(Query(terms, not_terms=nots, sort_score=True, descending=desc, limit=0))
    if conds:
        keep = set(F.apply_filters_with_bitmap(sorted(docs.tolist()), conds, columns))
        sel = np.asarray([d in keep for d in docs.tolist()], dtype=bool)
        docs, scores, total = docs[sel], scores[sel], int(sel.sum())
    return total, docs[offset: offset + limit], scores[offset: offset + limit], scores


def _doc_page(want, terms, nots, desc, limit, conds=None, columns=None):
    total, docs, _, _ = want.oracle_query(Query(terms, not_terms=nots, descending=desc, limit=0))
    if conds:
        keep = set(F.apply_filters_with_bitmap(sorted(docs.tolist()), conds, columns))
        docs = np.asarray([d for d in docs.tolist() if d in keep], dtype=np.uint32)
        total = len(docs)
    return total, docs[:limit] if limit else docs[:0]


def _check(t, m, want):
    """Every query shape without a page bound, through mgxs_search (ExecuteBatch), against the rebuilt index."""
    cols = m.columns()
    shapes = [([BIG[0]], []), ([BIG[1]], []), ([BIG[2], BIG[3]], []), ([BIG[0]], [BIG[3]]), (["zzqx"], []),
              ([BIG[1], "zzqx"], [])]
    ties = 0
    for terms, nots in shapes:
        for desc in (True, False):
            # docid order, limit 20000 (> 16384) and limit 0 (the total alone)
            wt, wd = _doc_page(want, terms, nots, desc, 20000)
            total, docs, _ = t.search(terms, not_terms=nots, descending=desc, limit=20000)
            assert total == wt and docs.tolist() == wd.tolist(), (terms, nots, desc, total, wt)
            total, docs, _ = t.search(terms, not_terms=nots, descending=desc, limit=0)
            assert total == wt and len(docs) == 0, (terms, nots, desc)
            # deep SORT _score pages
            for offset in (2000, 10000):
                wt, wd, ws, allsc = _score_page(want, terms, nots, desc, 100, offset)
                total, docs, scores = t.search(terms, not_terms=nots, sort_by_score=True, descending=desc, limit=100,
                                               offset=offset)
                assert total == wt and docs.tolist() == wd.tolist(), (terms, nots, desc, offset, total, wt)
                assert np.array_equal(scores, ws), (terms, nots, desc, offset)
                if 0 < offset < len(allsc) and allsc[offset - 1] == allsc[offset]:
                    ties += 1
    assert ties > 0  # some page boundary falls inside a tie class
    wt0 = want.oracle_query(Query([BIG[0]], limit=0))[0]
    assert wt0 > 16384 and want.oracle_query(Query([BIG[3]], limit=0))[0] > 16384, wt0
    # FILTER conditions on a typed column
    for conds in ([("status", "=", "2")], [("status", "!=", "1")], [("status", ">=", "3")]):
        for desc in (True, False):
            wt, wd = _doc_page(want, [BIG[0]], [], desc, 20000, conds, cols)
            total, docs, _ = t.search([BIG[0]], conditions=conds, descending=desc, limit=20000)
            assert total == wt and docs.tolist() == wd.tolist(), (conds, desc)
            wt, wd, ws, _ = _score_page(want, [BIG[1]], [BIG[3]], desc, 100, 2000, conds, cols)
            total, docs, scores = t.search([BIG[1]], not_terms=[BIG[3]], conditions=conds, sort_by_score=True,
                                           descending=desc, limit=100, offset=2000)
            assert total == wt and docs.tolist() == wd.tolist() and np.array_equal(scores, ws), (conds, desc)
    # text-level scored terms, alone and mixed with a one-gram term
    for terms in ([WORDS[0]], [WORDS[1]], [WORDS[2], BIG[1]], [BIG[0], WORDS[0]]):
        for desc in (True, False):
            wt, wd, ws, _ = _score_page(want, terms, [], desc, 100, 2000)
            total, docs, scores = t.search(terms, sort_by_score=True, descending=desc, limit=100, offset=2000)
            assert total == wt and docs.tolist() == wd.tolist(), (terms, desc, total, wt)
            assert np.array_equal(scores, ws), (terms, desc)


def _check_executor(ex, batcher, want):
    S = _shim()
    lists = [[BIG[0]], [BIG[2], BIG[3]], [BIG[1]], ["zzqx"], [WORDS[1]]]
    qb = S.QueryBatch(lists)
    t1 = ex.submit(qb, limit=20000, sort_by_score=False)
    t2 = ex.submit(qb, limit=100, offset=2000)
    totals, n_docs, docs, _, _ = ex.wait(t1)
    for qi, terms in enumerate(lists):
        wt, wd, _, _ = want.oracle_query(Query(terms, limit=20000))
        assert totals[qi] == wt and docs[qi, :n_docs[qi]].tolist() == wd.tolist(), terms
    totals, n_docs, docs, scores, _ = ex.wait(t2)
    for qi, terms in enumerate(lists):
        wt, wd, ws, _ = _score_page(want, terms, [], True, 100, 2000)
        assert totals[qi] == wt and docs[qi, :n_docs[qi]].tolist() == wd.tolist(), terms
        assert np.array_equal(scores[qi, :n_docs[qi]], ws), terms
    for terms in lists[:3]:
        total, docs, scores = batcher.search(terms, limit=100, offset=10000)
        wt, wd, ws, _ = _score_page(want, terms, [], True, 100, 10000)
        assert total == wt and docs.tolist() == wd.tolist() and np.array_equal(scores, ws), terms
        total, docs, _ = batcher.search(terms, limit=20000, sort_by_score=False, descending=False)
        wt, wd = _doc_page(want, terms, [], False, 20000)
        assert total == wt and docs.tolist() == wd.tolist(), terms


def test_unbounded_and_deep_pages_on_a_changed_table_equal_an_index_built_from_the_current_documents():
    S = _shim()
    corpus = mg.Corpus.synthetic(N, seed=41)
    p = Pair(corpus=corpus)
    p.dev.ensure_text()
    t = S.Table(p.dev)
    rng = np.random.default_rng(43)
    status = rng.integers(0, 6, N)
    t.add_filter_column("status", "int32", status)
    m = Mirror(corpus, status)
    ex = S.Executor(t, depth=2, planner_threads=2)
    _check_executor(ex, S.Batcher(t, max_batch=64, max_delay_us=100, depth=2, planner_threads=2), p)  # static

    def change(n_remove, n_update, n_add, novel):
        live = sorted(m.docs)
        for d in rng.choice(live, n_remove, replace=False).tolist():
            t.remove_document(d, m.docs[d])
            del m.docs[d]
        live = sorted(m.docs)
        for k, d in enumerate(rng.choice(live, n_update, replace=False).tolist()):
            new = corpus.text(int(rng.integers(0, N))) + (b" zzqx" if k < novel else b"")
            t.update_document(d, m.docs[d], new)  # (the document keeps its filter values)
            m.docs[d] = new
        top = max(max(m.docs), N)
        for k in range(n_add):
            d = top + 1 + k
            new = corpus.text(int(rng.integers(0, N))) + (b" zzqx tail" if k < novel else b"")
            s = int(rng.integers(0, 6))
            t.add_document(d, new, filters={"status": ("int32", s)})
            m.docs[d] = new
            m.status[d] = s

    # delta ids interleave main's (updates), some lie past the build range (adds), one word only the delta knows (zzqx)
    change(300, 400, 250, novel=40)
    gone = [d for d in range(1, N + 1) if d not in m.docs][:5]
    for d in gone:  # removed ids come back
        t.add_document(d, corpus.text(d - 1), filters={"status": ("int32", 4)})
        m.docs[d] = corpus.text(d - 1)
        m.status[d] = 4
    assert t.mutation_stats()["delta_documents"] > 0
    want = m.rebuilt()
    _check(t, m, want)
    batcher = S.Batcher(t, max_batch=64, max_delay_us=100, depth=2, planner_threads=2)
    _check_executor(ex, batcher, want)
    # second round: documents of the delta change and leave
    delta_docs = [d for d in m.docs if d > N][:40]
    for d in delta_docs[:20]:
        t.remove_document(d, m.docs[d])
        del m.docs[d]
    for d in delta_docs[20:]:
        new = corpus.text(int(rng.integers(0, N)))
        t.update_document(d, m.docs[d], new)
        m.docs[d] = new
    change(100, 100, 50, novel=10)
    want = m.rebuilt()
    _check(t, m, want)
    _check_executor(ex, batcher, want)
    # compaction: one index again
    t.compact()
    assert t.mutation_stats()["delta_documents"] == 0
    _check_executor(ex, batcher, want)
    total, docs, _ = t.search([BIG[0]], descending=False, limit=20000)
    wt, wd = _doc_page(want, [BIG[0]], [], False, 20000)
    assert total == wt and docs.tolist() == wd.tolist()


def test_deep_score_pages_with_text_level_terms_on_a_static_table():
    corpus = mg.Corpus.synthetic(N, seed=41)
    p = Pair(corpus=corpus)
    p.dev.ensure_text()
    qs = []
    for terms in ([WORDS[0]], [WORDS[1]], [WORDS[0], WORDS[2]], [WORDS[1], BIG[1]], [BIG[0], WORDS[0]]):
        for desc in (True, False):
            for offset, limit in ((2000, 100), (10000, 100), (0, 0)):
                qs.append(Query(terms, sort_score=True, descending=desc, limit=limit, offset=offset))
    got = p.dev.search_batch(qs)
    for q, g in zip(qs, got):
        total, page, scores, _ = p.oracle_query(q)
        ctx = (q.terms, q.descending, q.offset, q.limit)
        assert g.total == total, ctx
        assert g.docs.tolist() == page.tolist(), ctx
        assert np.array_equal(g.scores, scores), ctx
