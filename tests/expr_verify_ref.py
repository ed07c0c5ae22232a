"""What the reference answers to a boolean-expression query under verify_text (the text post-filter of
ExecuteWithBooleanAst, src/server/search_pipeline.cpp:1505-1578), built from the oracle's primitives — the oracle does
not restate that branch. Nothing here needs a device: a `side` is a gpu_util.OracleSide (or a Pair, which is one).

The rule (BooleanAstMatchesExpandedText :298-318 over PostFilterByBooleanText :404-416 / the FUZZY lambda :1538-1555):
after NOT terms and filters, a candidate stays when the TREE is true over its stored normalized text. A TERM leaf is
true when its normalized term is non-empty and text.find(term) hits, or, with FUZZY d, ContainsFuzzyMatch(text, term, d)
does; AND = all children, OR = any child, NOT = negation. The filter only narrows the set-algebra result.

Also here: the generators of the second corpus of test_gpu_expr_verify.py (short words over a three-letter alphabet, on
which n-gram set algebra returns many false positives) and the coverage figures the tests assert."""
import json
import os

import numpy as np

import funnel_util as FU
from oracle import oracle as O
from pkg import mg

Query = mg.engine.Query
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expr_verify.json")
PAGE_KEYS = ("sort_score", "limit", "offset", "descending")


def golden():
    return json.load(open(GOLDEN))


def tuple_tree(t):
    return t if isinstance(t, str) else tuple([t[0]] + [tuple_tree(k) for k in t[1:]])


def normalized_tree(e):
    return O.normalize_text(e) if isinstance(e, str) else (e[0],) + tuple(normalized_tree(k) for k in e[1:])


def tree_terms(e, out=None):
    """The distinct leaves of a tree, in first-use order."""
    out = [] if out is None else out
    if isinstance(e, str):
        if e not in out:
            out.append(e)
    else:
        for k in e[1:]:
            tree_terms(k, out)
    return out


def tree_true(e, leaf):
    """BooleanAstMatchesExpandedText, search_pipeline.cpp:298-318."""
    if isinstance(e, str):
        return leaf(e)
    if e[0] == "and":
        return all(tree_true(k, leaf) for k in e[1:])
    if e[0] == "or":
        return any(tree_true(k, leaf) for k in e[1:])
    return not tree_true(e[1], leaf)


class Reference:
    """Expected answers over one side. The unverified candidates of a (tree, NOT terms, filters, universe, fuzzy) and
    every (leaf, doc) match are computed once, whatever the number of page shapes that ask for them."""

    def __init__(self, side):
        self.side = side
        self._leaf = {}   # (term bytes, fuzzy, doc) -> bool
        self._cand = {}   # query key -> (funnel dict of the unverified query, kept ids, every-term-rule ids)
        self._df = {}

    def _text(self, doc):
        if hasattr(self.side, "text_of"):
            return self.side.text_of(doc)
        return bytes(self.side.corpus.text(doc - self.side.columns.first_doc_id))

    def leaf_matches(self, term, fuzzy, doc):
        key = (term, fuzzy, doc)
        hit = self._leaf.get(key)
        if hit is None:
            text = self._text(doc)
            hit = bool(term) and (term in text or (fuzzy > 0 and O.contains_fuzzy_match(text, term, fuzzy)))
            self._leaf[key] = hit
        return hit

    def candidates(self, q):
        """-> (funnel dict, candidates after NOT terms and filters, of them the tree rule keeps, of them the every-term
        rule — each leaf of the tree must match — would keep)."""
        key = (repr(q.expr), tuple(q.not_terms), tuple(q.filters), repr(q.conditions), q.universe, q.fuzzy)
        if key not in self._cand:
            plain = Query(q.terms, q.not_terms, q.filters, expr=q.expr, universe=q.universe, fuzzy=q.fuzzy,
                          conditions=q.conditions, limit=0, descending=False)
            _, cand, _, r = self.side.oracle_query(plain)
            tree = normalized_tree(q.expr)
            terms = [t.encode("utf-8") for t in tree_terms(tree)]
            kept, every = [], []
            for doc in cand.tolist():
                if tree_true(tree, lambda t: self.leaf_matches(t.encode("utf-8"), q.fuzzy, doc)):
                    kept.append(doc)
                if all(self.leaf_matches(t, q.fuzzy, doc) for t in terms):
                    every.append(doc)
            self._cand[key] = (r, cand, np.asarray(kept, np.uint32), np.asarray(every, np.uint32))
        return self._cand[key]

    def df(self, term):
        if term not in self._df:
            self._df[term] = self.side._df(term)
        return self._df[term]

    def expected(self, q):
        """(total, page docids, page scores or None, funnel dict) of a Query(expr=..., verify_text=True)."""
        assert q.expr is not None and q.verify_text
        r, _, kept, _ = self.candidates(q)
        if q.sort_score:
            terms = O.collect_ast_scoring_terms(normalized_tree(q.expr))
            sc = O.score_documents(self.side.ostore, kept, terms, [self.df(t) for t in terms], self.side.N,
                                   self.side.avgdl, q.k1, q.b)
            page = O.sort_by_score(kept, sc, q.descending, q.limit, q.offset)
            lookup = dict(zip(kept.tolist(), sc.tolist()))
            return len(kept), page, np.asarray([lookup[d] for d in page.tolist()]), r
        page = kept[::-1] if q.descending else kept
        if q.limit:
            page = page[: q.limit]
        return len(kept), page, None, r

    def coverage(self, queries):
        """Figures over `queries`, one per tree (the page shape does not matter here)."""
        c = self.side.columns
        last_tile = (c.n_docs - 1) >> 14
        cov = dict(trees=0, cut=0, differs=0, nonempty=0, multi_round=0, last_tile=0, candidates=0, kept=0)
        for q in queries:
            _, cand, kept, every = self.candidates(q)
            tiles = np.bincount((cand.astype(np.int64) - c.first_doc_id) >> 14, minlength=last_tile + 1)
            cov["trees"] += 1
            cov["cut"] += len(kept) < len(cand)
            cov["differs"] += kept.tolist() != every.tolist()
            cov["nonempty"] += len(kept) > 0
            cov["multi_round"] += int(tiles.max(initial=0)) > 2048  # more candidates in one tile than one compaction round
            cov["last_tile"] += bool(len(kept)) and ((int(kept[-1]) - c.first_doc_id) >> 14) == last_tile
            cov["candidates"] += len(cand)
            cov["kept"] += len(kept)
        return cov


def compare(queries, got, ref):
    """Device results against Reference.expected: total, page, scores bit for bit and the four funnel counters."""
    for q, g in zip(queries, got):
        total, page, scores, r = ref.expected(q)
        ctx = (q.expr, q.not_terms, q.filters, q.conditions, q.universe, q.fuzzy, {k: getattr(q, k) for k in PAGE_KEYS})
        got_c = tuple(int(getattr(g, k)) for k in FU.COUNTERS)
        assert not g.empty_term_detected and not r["empty_term_detected"], ctx
        assert g.total == total, (ctx, g.total, total, got_c)
        assert g.docs.tolist() == page.tolist(), ctx
        if scores is not None:
            assert np.array_equal(g.scores, scores), (ctx, g.scores, scores)
        assert got_c == tuple(int(r[k]) for k in FU.COUNTERS), (ctx, got_c, [r[k] for k in FU.COUNTERS])


def funnel_queries(side, row, col, fuzzy=0):
    """funnel_util.expression_specs(seed=101) — 60 trees x 5 page shapes — each with verify_text."""
    specs = FU.expression_specs(side, seed=101, fuzzy=fuzzy)
    for s in specs:
        s.verify_text = True
    return [s.query(row, col) for s in specs]


def assert_funnel_coverage(cov, fuzzy):
    assert cov["trees"] == 60, cov
    assert cov["cut"] >= (25 if fuzzy else 6), cov
    assert cov["differs"] >= 40 and cov["nonempty"] >= 45 and cov["multi_round"] >= 25 and cov["last_tile"] >= 35, cov


# ---- the second corpus: words of 2-5 letters over "abc" --------------------------------------------------------------------
HARD_SEED, HARD_DOCS, HARD_TREES = 85, 16384 + 300, 40
HARD_PAGES = (dict(limit=0, descending=False), dict(sort_score=True, limit=10))


def _word(rng, lo, hi):
    return "".join("abc"[int(k)] for k in rng.integers(0, 3, int(rng.integers(lo, hi + 1))))


def hard_case(seed=HARD_SEED):
    """-> (texts, [(tree, NOT terms, with filter row)]). One seeded generator: the corpus first (documents of 2-4 words of
    2-5 letters), then 40 trees by funnel_util's recipe (depth <= 3, NOT 20 %, AND / OR of 2-3 children) over leaves of
    3-5 letters; every second tree carries a NOT term, every second pair a filter row.

    A tree whose root is a NOT over positive leaves is never cut in plain mode (what the set algebra leaves out of the
    child it leaves out of the text match too), and the recipe draws about a quarter of such roots. Measured with the
    oracle for the seed committed here: plain 30 of 40 trees cut, 18.9 % of 259,229 candidates dropped, 34 non-empty, 28
    with more than 2048 candidates in a tile; FUZZY 1: 34 cut, 29.9 % of 297,112 dropped, 36 non-empty, 30 multi-round."""
    rng = np.random.default_rng(seed)
    texts = [" ".join(_word(rng, 2, 5) for _ in range(int(rng.integers(2, 5)))) for _ in range(HARD_DOCS)]

    def tree(depth):
        if depth == 0 or rng.random() < 0.2:
            return _word(rng, 3, 5)
        r = rng.random()
        if r < 0.2:
            return ("not", tree(depth - 1))
        return ("and" if r < 0.55 else "or",) + tuple(tree(depth - 1) for _ in range(int(rng.integers(2, 4))))

    cases = []
    while len(cases) < HARD_TREES:
        t = tree(3)
        if isinstance(t, str):
            continue
        i = len(cases)
        cases.append((t, [_word(rng, 3, 4)] if i % 2 else [], (i // 2) % 2 == 1))
    return texts, cases


def hard_queries(cases, row, fuzzy=0):
    return [Query(not_terms=nots, filters=[(row, False)] if filt else [], expr=t, fuzzy=fuzzy, verify_text=True, **page)
            for t, nots, filt in cases for page in HARD_PAGES]


def assert_hard_coverage(cov):
    assert cov["trees"] == HARD_TREES, cov
    assert cov["cut"] >= 25 and cov["nonempty"] >= 20 and cov["multi_round"] >= 10, cov
    assert cov["candidates"] - cov["kept"] >= 0.10 * cov["candidates"], cov


# ---- a table by its documents (ids with gaps), and the case file of tests/cpp/expr_verify_test.cpp -------------------------
class DocSide:
    """What Reference needs of a side, over {doc id: text}: the oracle's own index and store of exactly these documents
    (the NOT universe is the ids that exist), n-gram size 2, no kanji size, cross_boundary_ngrams off."""

    def __init__(self, docs):
        self.docs = dict(docs)
        ids = sorted(self.docs)
        self.kw = dict(ngram_size=2, kanji_ngram_size=0, cross_boundary=False)
        self.oidx, self.ostore = O.Index(2, 0, False), O.DocumentStore()
        for d in ids:
            self.oidx.add_document(d, self.docs[d])
            self.ostore.add(d, self.docs[d])
        self.all_docs = np.asarray(ids, np.uint32)
        n, total_len = self.ostore.bm25_stats()
        self.N, self.avgdl = n, total_len / n

    def text_of(self, doc):
        return O.normalize_text(self.docs[doc]).encode("utf-8")

    def _df(self, term):
        return O.execute(self.oidx, self.ostore, [term], compute_df=True, **self.kw)["term_df"][0]

    def oracle_query(self, q):
        """The unverified, unpaged expression query (all Reference.candidates asks for)."""
        assert q.expr is not None and not q.filters and not q.conditions and q.limit == 0 and not q.sort_score
        r = O.execute_boolean_ast(self.oidx, self.ostore, normalized_tree(q.expr), (),
                                  [O.normalize_text(t) for t in q.not_terms], (), all_docs=self.all_docs, fuzzy=q.fuzzy,
                                  **self.kw)
        return len(r["results"]), r["results"], None, r


def _prefix(e):
    if isinstance(e, str):
        return "T:" + e
    head = "!" if e[0] == "not" else {"and": "&", "or": "|"}[e[0]] + str(len(e) - 1)
    return " ".join([head] + [_prefix(k) for k in e[1:]])


SHIM_QUERIES = [
    ("or-false-positive", dict(expr=("or", "abab", "cats"), verify_text=True)),
    ("fuzzy-or", dict(expr=("or", "goleng", "python"), fuzzy=1, verify_text=True)),
    ("fuzzy-or-unverified", dict(expr=("or", "goleng", "python"), fuzzy=1)),  # (FUZZY leaves alone)
    ("and-not", dict(expr=("and", "basics", ("not", "abab")), verify_text=True)),
    ("lone-not", dict(expr=("not", "abab"), not_terms=["machine"], verify_text=True)),
    ("fuzzy-unknown-under-not", dict(expr=("and", ("or", "learnig", "cats", "tutorial"), ("not", "zebra")), fuzzy=1,
                                     verify_text=True)),
    ("repeat", dict(expr=("or", ("and", "abab", "abzz"), ("and", "cats", ("not", "abab")), "abab"), verify_text=True)),
]


def shim_case():
    """-> (lines, summary): the reference's two vectors on their own tables, then one table that is built, queried,
    changed (a delta index exists) and queried again. Expected lines come from Reference over a DocSide of the documents
    current at that point."""
    lines, summary = [], dict(runs=0, cut=0, delta_runs=0, queries=0)

    def emit_queries(docs, queries):
        ref = Reference(DocSide(docs))
        for label, kw in queries:
            kw = dict(kw)
            q = Query(limit=0, descending=False, **kw)
            lines.append("q %s" % label)
            lines.append("ast %s" % _prefix(q.expr))
            for t in q.not_terms:
                lines.append("notterm %s" % t)
            lines.append("fuzzy %d" % q.fuzzy)
            lines.append("verify %d" % int(q.verify_text))
            if q.verify_text:
                total, page, _, r = ref.expected(q)
                top = ref.expected(Query(sort_score=True, limit=10, **kw))
                summary["cut"] += total < r["after_filters"]
            else:
                side = ref.side
                total, page, _, r = side.oracle_query(q)
                terms = O.collect_ast_scoring_terms(normalized_tree(q.expr))
                sc = O.score_documents(side.ostore, page, terms, [ref.df(t) for t in terms], side.N, side.avgdl, q.k1, q.b)
                tp = O.sort_by_score(page, sc, True, 10, 0)
                lookup = dict(zip(page.tolist(), sc.tolist()))
                top = (total, tp, np.asarray([lookup[d] for d in tp.tolist()]), r)
            lines.append("expect %d %s %s" % (total, " ".join(str(int(r[k])) for k in FU.COUNTERS),
                                              " ".join(map(str, page.tolist()))))
            bits = np.asarray(top[2], np.float64).view(np.uint64) if len(top[1]) else []
            lines.append("expectscore " + " ".join("%d:%x" % (d, b) for d, b in zip(top[1].tolist(), bits)))
            summary["queries"] += 1

    def run(name):
        lines.append("run %s" % name)
        summary["runs"] += 1

    g = golden()
    for case in g["cases"]:
        docs = {d: t for d, t in g["docs"] + case["extra_docs"]}
        lines.append("table")
        lines.extend("doc %d %s" % (d, docs[d]) for d in sorted(docs))
        q = dict(expr=tuple_tree(case["tree"]), fuzzy=case["fuzzy"], verify_text=True)
        emit_queries(docs, [(case["id"], q)])
        assert lines[-2].split(" ", 6)[6:] == [" ".join(map(str, case["expect"]))], (case["id"], lines[-2])
        if case["fuzzy"]:
            emit_queries(docs, [(case["id"] + "-unverified", dict(expr=q["expr"], fuzzy=case["fuzzy"]))])
        run(case["id"])
    docs = dict(FU.SMALL_DOCS + [(8, "abzzba"), (9, "golang tutorial"), (10, "python tutorial")])
    lines.append("table")
    lines.extend("doc %d %s" % (d, docs[d]) for d in sorted(docs))
    lines.append("build")
    emit_queries(docs, SHIM_QUERIES)
    run("main index only")
    changes = [("add", 20, "abab and cats"), ("add", 21, "abba baab zzab"), ("update", 3, "old article about dogs"),
               ("remove", 5, None), ("add", 22, "pithon and goleng"), ("update", 21, "abba baab dogs"),
               ("update", 2, "deep learning abzzba"), ("add", 25, "zebra tutorial")]
    for op, d, text in changes:
        if op == "remove":
            lines.append("remove %d" % d)
            del docs[d]
        else:
            lines.append("%s %d %s" % (op, d, text))
            docs[d] = text
    lines.append("delta 6")  # 20, 21, 22, 25 and the new versions of 2 and 3
    emit_queries(docs, SHIM_QUERIES)
    run("with a delta index")
    summary["delta_runs"] += 1
    return lines, summary
