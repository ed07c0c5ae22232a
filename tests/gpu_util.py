"""Shared helpers of the parity tests: build the same corpus on the device (through the C ABI) and in the oracle, and
run one query through both. OracleSide alone needs no device: it adopts the host-built columns (mg.Columns)."""
import numpy as np

import golden_util as G
from oracle import oracle as O
from pkg import mg


def densify(docs):
    """[(doc_id, text)] with arbitrary ids -> (first_doc_id, texts over the dense id range; gaps = empty text,
    which produces no n-grams and no BM25 weight, i.e. the doc does not exist for the hot path)."""
    ids = [d for d, _ in docs]
    first, last = min(ids), max(ids)
    texts = [""] * (last - first + 1)
    for d, t in docs:
        texts[d - first] = t if t is not None else ""
    return first, texts


OPS = ("=", "!=", "<", "<=", ">", ">=")  # mgx_condition.op


class OracleSide:
    """The oracle's copy of one index (its CSR columns and texts) and what the reference would answer to a Query."""

    def __init__(self, columns, corpus, first_doc_id=1, total_docs=None, avg_doc_length=None):
        c = self.columns = columns
        self.corpus = corpus
        self.ngram_size, self.kanji_ngram_size, self.cross_boundary = c.ngram_size, c.kanji_ngram_size, c.cross_boundary
        # the oracle adopts the CSR arrays; tests/test_host_cpu.py pins those arrays to the oracle's own text-level build
        self.oidx = O.Index.from_csr(c.ngram_size, c.kanji_ngram_size, c.cross_boundary, c.key_bytes, c.key_off,
                                     c.offsets, c.docids)
        if first_doc_id == 1:
            self.ostore = O.DocumentStore.from_arrays(corpus.text_bytes, corpus.text_off)
        else:
            self.ostore = O.DocumentStore()
            for i in range(corpus.n_docs):
                t = corpus.text(i)
                if t:
                    self.ostore.add(first_doc_id + i, t)
        self.N, self.total_len = c.bm25_doc_count, c.bm25_total_len
        self.avgdl = c.avg_doc_length()
        if total_docs is not None:
            self.N = total_docs
        if avg_doc_length is not None:
            self.avgdl = avg_doc_length
        self.filters = {}  # bitmap id -> sorted docids
        self.typed = {}    # filter column id -> (int64 values by slot, is-NULL by slot)

    def condition_docs(self, cond):
        """One Query(conditions=[...]) entry over a signed column registered with add_column -> (sorted docids, negate):
        the comparison written out in numpy (NULL matches only when null_matches says so)."""
        col, op, lit, eps, null_matches, never_matches, negate = (tuple(cond) + (0.0, False, False, False))[:7]
        v, nul = self.typed[col]
        b = np.int64(lit)
        m = {"=": v == b, "!=": v != b, "<": v < b, "<=": v <= b, ">": v > b, ">=": v >= b}[OPS[op]]
        if never_matches:
            m = np.zeros(len(v), bool)
        m = np.where(nul, bool(null_matches), m)
        return (np.nonzero(m)[0] + self.columns.first_doc_id).astype(np.uint32), bool(negate)

    def _df(self, term):
        return O.execute(self.oidx, self.ostore, [term], compute_df=True, ngram_size=self.ngram_size,
                         kanji_ngram_size=self.kanji_ngram_size, cross_boundary=self.cross_boundary)["term_df"][0]

    def _scored_page(self, q, res, terms):
        """SORT _score over `res` by the (normalized) `terms` in that order: df per term as
        PopulateTermDocumentFrequency counts it, BM25Scorer::ScoreDocuments, ResultSorter::SortByScore."""
        sc = O.score_documents(self.ostore, res, terms, [self._df(t) for t in terms], self.N, self.avgdl, q.k1, q.b)
        page = O.sort_by_score(res, sc, q.descending, q.limit, q.offset)
        lookup = dict(zip(res.tolist(), sc.tolist()))
        return page, np.asarray([lookup[d] for d in page.tolist()])

    def oracle_query(self, q):
        """(total, page docids, page scores or None, funnel dict) the reference would produce."""
        filters = [(self.filters[bid], neg) for bid, neg in q.filters] + [self.condition_docs(c) for c in q.conditions]
        # the C oracle restates the non-ICU NormalizeText branch; the ICU branch is applied here (idempotent under it)
        q_terms = [O.normalize_text(t) for t in q.terms]
        q_not = [O.normalize_text(t) for t in q.not_terms]
        kw = dict(ngram_size=self.ngram_size, kanji_ngram_size=self.kanji_ngram_size, cross_boundary=self.cross_boundary)
        if q.expr is not None:
            # ExecuteWithBooleanAst; q.fuzzy makes every leaf a FUZZY term (search_pipeline.cpp:1424-1445, :1470-1471)
            c = self.columns
            first, count = q.universe if q.universe is not None else (c.first_doc_id, c.n_docs)
            all_docs = np.arange(max(first, c.first_doc_id), min(first + count, c.first_doc_id + c.n_docs), dtype=np.uint32)

            def norm(e):
                return O.normalize_text(e) if isinstance(e, str) else (e[0],) + tuple(norm(k) for k in e[1:])
            tree = norm(q.expr)
            r = O.execute_boolean_ast(self.oidx, self.ostore, tree, (), q_not, filters, all_docs=all_docs, fuzzy=q.fuzzy,
                                      **kw)
            scored_terms = O.collect_ast_scoring_terms(tree)
        elif q.fuzzy:
            r = O.execute_fuzzy(self.oidx, self.ostore, q_terms, q.fuzzy, q_not, filters, verify_text=q.verify_text, **kw)
            scored_terms = q_terms  # the exact terms, in the order given (search_pipeline.cpp:1895-1899)
        else:
            r = O.execute(self.oidx, self.ostore, q_terms, q_not, filters, compute_df=q.sort_score,
                          verify_text=q.verify_text, **kw)
            res = r["results"]
            if q.sort_score:
                terms = [q_terms[i] for i in r["term_order"]]
                sc = O.score_documents(self.ostore, res, terms, r["term_df"], self.N, self.avgdl, q.k1, q.b)
                page = O.sort_by_score(res, sc, q.descending, q.limit, q.offset)
                lookup = dict(zip(res.tolist(), sc.tolist()))
                return len(res), page, np.asarray([lookup[d] for d in page.tolist()]), r
            scored_terms = None
        res = r["results"]
        if q.sort_score:
            page, scores = self._scored_page(q, res, scored_terms)
            return len(res), page, scores, r
        page = res[::-1] if q.descending else res
        if q.limit:
            page = page[: q.limit]
        return len(res), page, None, r


class Pair(OracleSide):
    """The same index on the device (mg.Index) and in the oracle."""

    def __init__(self, docs=None, corpus=None, first_doc_id=1, ngram=2, kanji=0, cross=True, dense_threshold=0.0,
                 total_docs=None, avg_doc_length=None):
        """total_docs / avg_doc_length: BM25 statistics other than the index's own (a shard scores with the table's),
        used by the device index and the oracle alike; None keeps the index's own."""
        if corpus is None:
            first_doc_id, texts = densify(docs)
            corpus = mg.Corpus.from_texts(texts)
        self.dev = mg.Index(corpus=corpus, first_doc_id=first_doc_id, ngram_size=ngram, kanji_ngram_size=kanji,
                            cross_boundary=cross, dense_threshold=dense_threshold, total_docs=total_docs,
                            avg_doc_length=avg_doc_length)
        OracleSide.__init__(self, self.dev.columns, corpus, first_doc_id, total_docs, avg_doc_length)

    def add_filter(self, docids):
        docids = np.asarray(sorted(docids), dtype=np.uint32)
        bid = self.dev.device_index.add_filter_bitmap(docids)
        self.filters[bid] = docids
        return bid

    def add_column(self, values, nulls):
        """A signed typed column for Query(conditions=...), known to the device and to oracle_query."""
        values, nulls = np.asarray(values, np.int64), np.asarray(nulls, bool)
        col = self.dev.device_index.add_filter_column(values, nulls)
        self.typed[col] = (values, nulls)
        return col

    def check(self, queries):
        got = self.dev.search_batch(queries)
        for q, g in zip(queries, got):
            total, page, scores, r = self.oracle_query(q)
            ctx = (q.terms, q.not_terms, q.filters, q.limit, q.offset, q.descending, q.expr, q.fuzzy)
            assert g.total == total, ctx
            assert g.docs.tolist() == page.tolist(), ctx
            if scores is not None:
                # fp64 arithmetic in the reference's operation order: bit-exact, far inside the 1e-5 relative bar
                assert np.array_equal(g.scores, scores), (ctx, g.scores, scores)
            assert g.empty_term_detected == r["empty_term_detected"], ctx
            if not r["empty_term_detected"]:
                for k in ("total_candidates", "after_intersection", "after_not", "after_filters"):
                    assert getattr(g, k) == r[k], (ctx, k, getattr(g, k), r[k])
        return got
