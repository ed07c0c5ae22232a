"""-m gpu: FACET in a batch (facet_batch_kernel) through the C ABI (mgx_batch_set_facets / mgx_batch_fetch_facets) and
engine.py (Query(facet_columns=...), SearchResult.facets).

Every count array must equal oracle.filters.facet_counts over the oracle's result set of the query AND what
mgx_facet_counts returns for the same (query, column), exactly; totals and funnel counters must not depend on the
request; a batch's other results must not depend on its faceted queries.

The main table holds 40 000 documents (three tiles, the last one partial); the second one 5 003 documents from doc id
1000 on (a partial tile whose document count is no multiple of 64). SORT <column> pages and highlighted queries sit in
two mixed batches, not one: a highlighted batch that holds a column-sorted query is refused (tests/test_gpu_column_sort.py).
"""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpu_util import Pair
from oracle import filters as F
from pkg import ROOT, mg

pytestmark = pytest.mark.gpu
Query = mg.engine.Query
_capi = mg._capi
NULL = 0xFFFFFFFF


def _lds_bins():
    src = open(os.path.join(ROOT, "include", "mygram_gpu.h")).read()
    return int(re.search(r"#define MGX_FACET_LDS_BINS (\d+)u", src).group(1))


BINS = _lds_bins()


class Table:
    """A Pair with facet columns: name -> (column id, n_values, value ids by slot)."""

    def __init__(self, n_docs, first_doc_id, seed):
        self.p = Pair(corpus=mg.Corpus.synthetic(n_docs, seed=seed), first_doc_id=first_doc_id)
        self.n, self.first = n_docs, first_doc_id
        self.rng = np.random.default_rng(seed)
        self.cols = {}
        self.stored = {}  # column id -> what F.facet_counts looks up per slot: ("int64", value id) or None
        self.words = self._frequent_words()

    def _frequent_words(self):
        cnt = collections.Counter()
        for i in range(min(self.n, 5000)):
            for wd in bytes(self.p.corpus.text(i)).decode("utf-8").split():
                if len(wd) >= 3:
                    cnt[wd] += 1
        return [wd for wd, _ in cnt.most_common(16)]

    def add(self, name, n_values, null_share):
        ids = self.rng.integers(0, max(n_values, 1), self.n).astype(np.uint32)
        nul = self.rng.random(self.n) < null_share if n_values else np.ones(self.n, bool)
        ids[nul] = NULL
        vals = np.where(nul, 0, ids).astype(np.int64)
        cid = self.p.dev.device_index.add_filter_column(vals, nul, value_ids=ids, n_values=n_values)
        self.cols[name] = (cid, n_values, ids)
        self.stored[cid] = [None if i == NULL else ("int64", int(i)) for i in ids.tolist()]
        return cid

    def oracle_counts(self, docs, cid):
        n_values = next(nv for c, nv, _ in self.cols.values() if c == cid)
        lst, first = self.stored[cid], self.first
        got = F.facet_counts(docs.tolist(), lambda d: lst[d - first])
        out = np.zeros(n_values, np.uint64)
        for (_, v), c in got.items():
            out[v] = c
        return out

    def null_matches(self, docs, cid):
        ids = next(i for c, _, i in self.cols.values() if c == cid)
        return int(np.count_nonzero(ids[docs.astype(np.int64) - self.first] == NULL))


def _standard_columns(t):
    t.add("c2", 2, 0.0)
    t.add("c10", 10, 0.3)
    t.add("cnull", 0, 1.0)
    t.add("below", BINS - 1, 0.1)
    t.add("exact", BINS, 0.1)
    t.add("above", BINS + 1, 0.1)
    t.add("c30k", 30_000, 0.05)
    # a signed column for conditions, added WITHOUT value ids (the refusal's column too)
    cond_vals = t.rng.integers(-50, 50, t.n)
    cond_nul = t.rng.random(t.n) < 0.1
    t.cond = t.p.add_column(cond_vals, cond_nul)


def _column_sets(t):
    c = {k: v[0] for k, v in t.cols.items()}
    return [
        [c["c2"]],
        [c["c10"], c["c2"]],
        [c["c2"], c["c2"]],                       # the same column twice
        [c["below"], c["c2"]],                    # BINS - 1 + 2: the two straddle the LDS budget together
        [c["exact"]],
        [c["above"], c["c10"]],                   # the first counts in global memory, the second in LDS
        [c["c30k"], c["c2"]],                     # 30 000 values beside a small column
        [c["cnull"], c["c10"]],
        [c["c10"], c["below"]],
        [c["c2"], c["c10"], c["cnull"], c["below"], c["exact"], c["above"], c["c30k"], c["c10"]],  # eight
    ]


def _queries(t, n_queries):
    """The shapes of the issue's list, round robin, each with the next column set."""
    w = t.words
    sets = _column_sets(t)
    out = []
    for i in range(n_queries):
        a, b, c = w[i % len(w)], w[(i * 7 + 3) % len(w)], w[(i * 5 + 1) % len(w)]
        cols = sets[i % len(sets)]
        kind = i % 8 if i >= 8 else i
        if i == 0:
            q = Query(expr=("not", "0909"), facet_columns=cols)                      # the universe: NOT(<empty>)
        elif i == 1:
            q = Query(["09090909"], fuzzy=1, facet_columns=cols)                          # MGX_GRAM_ABSENT
        elif i == 2:
            q = Query(["zz09qq"], facet_columns=cols)                                     # resolved on the host: empty
        elif kind == 3:
            q = Query([a], not_terms=[b], facet_columns=cols)
        elif kind == 4:
            q = Query([a], conditions=[(t.cond, 4, int(i % 40) - 30)], facet_columns=cols)  # column > literal
        elif kind == 5:
            q = Query(expr=("or", a, ("and", b, c)), facet_columns=cols)
        elif kind == 6:
            q = Query([a[:-1] + "q"], fuzzy=1, facet_columns=cols)
        elif kind == 7:
            q = Query([a, b], facet_columns=cols)
        else:
            q = Query([a], facet_columns=cols)
        out.append(q)
    return out


def _plain(q, **changes):
    c = Query.__new__(Query)
    c.__dict__.update(q.__dict__)
    c.facet_columns = None
    c.__dict__.update(changes)
    return c


class World:
    def __init__(self, n_docs, first_doc_id, seed, n_queries):
        self.t = Table(n_docs, first_doc_id, seed)
        _standard_columns(self.t)
        self.queries = _queries(self.t, n_queries)
        self.got = self.t.p.dev.search_batch(self.queries)
        self.base = self.t.p.dev.search_batch([_plain(q) for q in self.queries])
        self.oracle = [self.t.p.oracle_query(_plain(q, descending=False)) for q in self.queries]


@pytest.fixture(scope="module")
def main():
    return World(40_000, 1, 91, 300)


@pytest.fixture(scope="module")
def second():
    return World(5_003, 1000, 17, 40)


def _check_oracle(w):
    t = w.t
    non_empty = 0
    for q, g, (total, docs, _, r) in zip(w.queries, w.got, w.oracle):
        assert g.total == total and len(g.docs) == 0, (q.terms, q.expr)
        non_empty += 1 if total else 0
        assert len(g.facets) == len(q.facet_columns)
        cache = {}
        for cid, counts in zip(q.facet_columns, g.facets):
            if cid not in cache:
                cache[cid] = t.oracle_counts(docs, cid)
            assert counts.dtype == np.uint64 and np.array_equal(counts, cache[cid]), (q.terms, q.expr, cid)
            assert int(counts.sum()) + t.null_matches(docs, cid) == total
    return non_empty


def test_parity_with_the_oracle(main):
    non_empty = _check_oracle(main)
    totals = [o[0] for o in main.oracle]
    assert non_empty * 4 >= 3 * len(main.queries), non_empty  # (the oracle alone meets the share)
    assert totals[0] == main.t.n  # the universe matches every document
    assert totals[1] == 0 and totals[2] == 0 and main.got[2].empty_term_detected


def test_parity_on_a_table_that_starts_at_doc_1000(second):
    assert _check_oracle(second) * 4 >= 3 * len(second.queries)
    assert second.oracle[0][0] == second.t.n


def test_parity_with_mgx_facet_counts(main):
    t, dev = main.t, main.t.p.dev
    n_values = {c: nv for c, nv, _ in t.cols.values()}
    for i, (q, g) in enumerate(zip(main.queries, main.got)):
        single = {}
        for cid, counts in zip(q.facet_columns, g.facets):
            if cid not in single:
                single[cid] = dev.facet_counts(_plain(q), cid, n_values[cid])
            matched, want = single[cid]
            assert matched == g.total, (i, cid)
            assert np.array_equal(counts, want), (i, cid)


def test_totals_and_funnel_counters_do_not_depend_on_the_request(main):
    for q, g, b, (total, docs, _, r) in zip(main.queries, main.got, main.base, main.oracle):
        assert g.total == b.total == total
        assert len(b.docs) == total  # (without the request the query returns every match)
        for k in ("total_candidates", "after_intersection", "after_not", "after_filters"):
            assert getattr(g, k) == getattr(b, k), (q.terms, q.expr, k)
            if not r["empty_term_detected"]:
                assert getattr(g, k) == r[k], (q.terms, q.expr, k)


def _same(a, b):
    assert a.total == b.total and a.docs.tolist() == b.docs.tolist() and np.array_equal(a.scores, b.scores)
    assert a.snippets == b.snippets
    assert (a.total_candidates, a.after_intersection, a.after_not, a.after_filters) == \
        (b.total_candidates, b.after_intersection, b.after_not, b.after_filters)


def test_mixed_batches(main):
    t, dev = main.t, main.t.p.dev
    w, c = t.words, {k: v[0] for k, v in t.cols.items()}
    facets = [Query([w[0], w[1]], facet_columns=[c["c2"], c["c30k"]]), Query([w[2]], facet_columns=[c["c10"]])]
    pages = [Query([w[0], w[1]], sort_score=True, limit=10), Query([w[2]], limit=20, offset=5, descending=False),
             Query([w[3]], limit=0), Query([w[4]], limit=50, offset=20_000)]  # SORT _score, doc ids, unbounded, deep
    first = [facets[0], pages[0], Query([w[1]], sort_column=t.cond, limit=15, offset=2), pages[1], facets[1], pages[2], pages[3]]
    second = [pages[0], facets[0], Query([w[5]], sort_score=True, limit=10, highlight=True), pages[3], facets[1], pages[1]]
    for batch in (first, second):
        got = dev.search_batch(batch)
        base = dev.search_batch([_plain(q) for q in batch])
        for q, g, b in zip(batch, got, base):
            if q.facet_columns:
                assert len(g.docs) == 0 and g.total == b.total == len(b.docs)
                want = [main.t.oracle_counts(np.sort(b.docs), cid) for cid in q.facet_columns]
                assert all(np.array_equal(x, y) for x, y in zip(g.facets, want))
            else:
                _same(g, b)
                assert g.facets == []
    assert len(got[2].snippets) == 10


def _fetch_view(batch):
    fv = _capi.FacetView()
    rc = _capi.load().mgx_batch_fetch_facets(batch._h, C.byref(fv))
    return rc, fv


def test_lifecycle(main):
    t, dev = main.t, main.t.p.dev
    w, c = t.words, {k: v[0] for k, v in t.cols.items()}
    small = [Query([w[0]], facet_columns=[c["c2"]]), Query([w[1], w[2]], limit=10)]
    b = dev.prepare(small)
    b.execute()
    one = b.fetch()
    b.execute()  # every execute zeroes its counts
    two = b.fetch()
    assert np.array_equal(one[0].facets[0], two[0].facets[0]) and int(one[0].facets[0].sum()) == one[0].total > 0
    dev.prepare([Query([w[3]], limit=10)], into=b)  # reset drops the requests
    b.execute()
    assert b.fetch()[0].facets == []
    rc, fv = _fetch_view(b)
    assert rc == 0 and fv.n_entries == 0
    larger = [Query([w[i]], facet_columns=[c["c30k"], c["above"], c["c10"]]) for i in range(6)]  # the arena grows
    dev.prepare(larger, into=b)
    b.execute()
    for q, g in zip(larger, b.fetch()):
        total, docs, _, _ = t.p.oracle_query(_plain(q, descending=False))
        assert g.total == total > 0
        for cid, counts in zip(q.facet_columns, g.facets):
            assert np.array_equal(counts, t.oracle_counts(docs, cid))


def test_live_row(second):
    """Last in the module: it changes the second table's index."""
    t, dev = second.t, second.t.p.dev
    L = _capi.load()
    h = dev.device_index._h
    every = np.arange(t.first, t.first + t.n, dtype=np.uint32)
    live = dev.device_index.add_filter_bitmap(every)
    dead = np.unique(t.rng.integers(t.first, t.first + t.n, 700)).astype(np.uint32)
    assert L.mgx_index_set_live_bitmap(C.c_void_p(h.value), C.c_uint32(live), C.c_int(1)) == 0
    assert L.mgx_index_update_filter_bitmap(C.c_void_p(h.value), C.c_uint32(live), None, C.c_uint64(0),
                                            C.c_void_p(dead.ctypes.data), C.c_uint64(len(dead))) == 0
    assert L.mgx_index_synchronize(C.c_void_p(h.value)) == 0
    w, c = t.words, {k: v[0] for k, v in t.cols.items()}
    queries = [Query([w[0]], facet_columns=[c["c2"], c["c10"]]), Query([w[1], w[2]], facet_columns=[c["exact"]]),
               Query([w[3]], not_terms=[w[4]], facet_columns=[c["c30k"], c["c2"]])]
    try:
        got = dev.search_batch(queries)
        n_dead = 0
        for q, g in zip(queries, got):
            _, docs, _, _ = t.p.oracle_query(_plain(q, descending=False))
            alive = docs[~np.isin(docs, dead)]
            n_dead += len(docs) - len(alive)
            assert g.total == len(alive)
            for cid, counts in zip(q.facet_columns, g.facets):
                assert np.array_equal(counts, t.oracle_counts(alive, cid))
        assert n_dead > 0
    finally:
        assert L.mgx_index_set_live_bitmap(C.c_void_p(h.value), C.c_uint32(live), C.c_int(0)) == 0


# ---- the C ABI's refusals -------------------------------------------------------------------------------------------

def _set(batch, column_lists, n=None):
    L = _capi.load()
    keep = [(C.c_uint32 * max(len(cl), 1))(*cl) for cl in column_lists]
    reqs = (_capi.FacetRequest * max(len(column_lists), 1))(
        *[_capi.FacetRequest(len(cl), 0, k) for cl, k in zip(column_lists, keep)])
    rc = L.mgx_batch_set_facets(batch._h, reqs, len(column_lists) if n is None else n)
    return rc, L.mgx_last_error().decode()


def test_refusals(main):
    L = _capi.load()
    t, dev = main.t, main.t.p.dev
    w, c = t.words, {k: v[0] for k, v in t.cols.items()}
    INVALID, RANGE, NOT_IMPL = 2, 3, 4
    q0 = Query([w[0]], limit=0, descending=False)
    # null arguments, a wrong n_queries, twice, after the first execute
    b = dev.prepare([q0])
    assert L.mgx_batch_set_facets(None, None, 0) == INVALID and "null" in L.mgx_last_error().decode()
    assert L.mgx_batch_set_facets(b._h, None, 1) == INVALID and "null" in L.mgx_last_error().decode()
    rc, msg = _set(b, [[c["c2"]], [c["c2"]]])
    assert rc == INVALID and "one request per query" in msg
    assert _set(b, [[c["c2"]]])[0] == 0
    rc, msg = _set(b, [[c["c2"]]])
    assert rc == INVALID and "once" in msg
    b = dev.prepare([q0])
    b.execute()
    b.fetch()
    rc, msg = _set(b, [[c["c2"]]])
    assert rc == INVALID and "before the first execute" in msg
    # another sort, a limit
    for q in (Query([w[0]], sort_score=True, limit=10), Query([w[0]], sort_score=True, limit=0), Query([w[0]], limit=10),
              Query([w[0]], limit=20_000), Query([w[0]], sort_column=t.cond, limit=0)):
        rc, msg = _set(dev.prepare([q0, q]), [[], [c["c2"]]])
        assert rc == INVALID and "query 1" in msg and "limit 0" in msg, (rc, msg)
    # an unknown column, a column without value ids, too many columns
    rc, msg = _set(dev.prepare([q0]), [[c["c2"], 9999]])
    assert rc == RANGE and "query 0" in msg and "unknown filter column" in msg
    rc, msg = _set(dev.prepare([q0, q0]), [[], [t.cond]])
    assert rc == INVALID and "query 1" in msg and "without value ids" in msg
    rc, msg = _set(dev.prepare([q0]), [[c["c2"]] * 9])
    assert rc == RANGE and "query 0" in msg and "MGX_FACET_MAX_COLUMNS" in msg
    assert _set(dev.prepare([q0]), [[c["c2"]] * 8])[0] == 0
    # counts above the arena's cap: 256 MiB / 8 bytes = 33 554 432 values; 140 queries x 8 x 30 000 values pass it
    many = [q0] * 140
    rc, msg = _set(dev.prepare(many), [[c["c30k"]] * 8] * 140)
    assert rc == RANGE and "MGX_FACET_ARENA_CAP" in msg and "query 139" in msg  # (139 x 8 x 30 000 x 8 bytes still fit)
    # fetch_facets before fetch
    b = dev.prepare([Query([w[0]], facet_columns=[c["c2"]])])
    b.execute()
    rc, _ = _fetch_view(b)
    assert rc == INVALID and "mgx_batch_fetch" in L.mgx_last_error().decode()
    # a sharded table: every entry point refuses a faceted batch before it touches anything
    dummy = (C.c_uint64 * 64)()
    stride = C.c_uint32(0)
    blob, nbytes, off32 = C.c_void_p(), C.c_uint64(), C.c_uint64()
    fn = _capi.GATHER_FN(lambda *a: 7)
    calls = [lambda: L.mgx_batch_merge_shards(b._h, 1, dummy, 0, C.cast(dummy, C.c_void_p), 0, None),
             lambda: L.mgx_batch_export_topk(b._h, None, None, C.byref(stride), None),
             lambda: L.mgx_batch_export_buffer(b._h, C.byref(blob), C.byref(nbytes), C.byref(off32)),
             lambda: L.mgx_batch_execute_gather(b._h, 2, fn, None, None),
             lambda: L.mgx_batch_exchange(b._h, None, None),
             lambda: L.mgx_batch_execute_sharded(b._h, None, None)]
    for call in calls:
        assert call() == NOT_IMPL
        assert "sharded" in L.mgx_last_error().decode() and "facets" in L.mgx_last_error().decode()
    r = b.fetch()[0]
    assert int(r.facets[0].sum()) == r.total > 0
