"""Seeded query generators of the funnel-counter tests (test_gpu_funnel.py on the device, test_funnel_queries_cpu.py
with the oracle alone), and the coverage conditions both assert. Nothing here needs a device: a `side` is a
gpu_util.OracleSide (or a Pair, which is one).

A generated query is a Spec: everything a Query takes, with the filter row and the typed column named symbolically
("row" / "col") so that the device test can register them and the CPU test can stand them in."""
import numpy as np

from gpu_util import OPS
from pkg import mg

Query = mg.engine.Query
COUNTERS = ("total_candidates", "after_intersection", "after_not", "after_filters")
# page shapes every expression tree is run at: docid pages of limit 0 / 17 / 20000, SORT _score top 10, and a score page
# with offset + limit > 1024 (the full-sort path)
PAGES = (dict(limit=0, descending=False), dict(limit=17), dict(limit=20000, descending=False),
         dict(sort_score=True, limit=10), dict(sort_score=True, limit=40, offset=1000))
BITMAP_DOCS, LISTS_DOCS = 2 * 16384 + 77, 16384 + 300
SMALL_DOCS = [(1, "machine learning basics"), (2, "deep learning techniques"), (3, "old article about cats"),
              (4, "learning learning learning"), (5, "cats and machine cats"), (6, "basics of basics"),
              (7, "golang tutorial basics")]


class Spec:
    def __init__(self, kind, terms=(), expr=None, not_terms=(), filt=None, universe=None, fuzzy=0, verify_text=False,
                 page=None):
        self.kind, self.terms, self.expr, self.not_terms = kind, list(terms), expr, list(not_terms)
        self.filt, self.universe, self.fuzzy, self.verify_text = filt, universe, fuzzy, verify_text
        self.page = dict(page or {})

    def query(self, row, col):
        """The Query of this spec: `row` = id of the registered filter row, `col` = id of the typed column."""
        kw = dict(self.page)
        if self.filt in ("row", "not-row"):
            kw["filters"] = [(row, self.filt == "not-row")]
        elif self.filt == "cond":
            kw["conditions"] = [(col, OPS.index("<"), COND_LITERAL, 0.0, False, False, False)]
        return Query(self.terms, self.not_terms, expr=self.expr, universe=self.universe, fuzzy=self.fuzzy,
                     verify_text=self.verify_text, **kw)


# ---- the filter row and the typed column of an index --------------------------------------------------------------------
COND_LITERAL = 10


def filter_row_docs(side, seed=7):
    """About 60% of the documents, the last one among them (a set bit in the last, partial bitmap word)."""
    c = side.columns
    m = np.random.default_rng(seed).random(c.n_docs) < 0.6
    m[-1] = True
    return (np.nonzero(m)[0] + c.first_doc_id).astype(np.uint32)


def typed_column(side, seed=8):
    """(int64 values in [-40, 40), is-NULL) by slot; `value < COND_LITERAL` holds for about 56% of the documents."""
    n = side.columns.n_docs
    rng = np.random.default_rng(seed)
    values = rng.integers(-40, 40, n).astype(np.int64)
    nulls = rng.random(n) < 0.1
    nulls[0], nulls[-1] = False, True
    return values, nulls


def register_cpu(side):
    """The row and the column on an OracleSide without a device: ids 0 and 0."""
    side.filters[0] = filter_row_docs(side)
    side.typed[0] = typed_column(side)
    return 0, 0


# ---- vocabulary ----------------------------------------------------------------------------------------------------------
def vocabulary(side):
    """-> dict: 'dense' single-gram terms (the 24 longest lists), 'mid' single-gram terms (lists of 2-25% of the documents),
    'words' whole words of 4-8 letters out of the documents (multi-gram terms), 'unknown' grams no document holds,
    'docs' a few documents' word lists (terms that occur together)."""
    c = side.columns
    sizes = np.diff(c.offsets.astype(np.int64))
    order = [int(g) for g in np.argsort(-sizes, kind="stable") if b" " not in c.gram(g)]
    dense = [c.gram(g).decode() for g in order[:24]]
    mid = [c.gram(g).decode() for g in order if 0.02 * c.n_docs <= sizes[g] <= 0.25 * c.n_docs][:40]
    step = max(1, c.n_docs // 400)
    docs = [[w for w in side.corpus.text(i).decode().split(" ") if 4 <= len(w) <= 8] for i in range(0, c.n_docs, step)]
    docs = [d for d in docs if len(d) >= 2]
    words = sorted({w for d in docs for w in d})
    unknown = [g for g in ("7q", "x9", "99", "0z") if c.lookup(g) is None]  # (the corpus holds letters and spaces only)
    assert len(dense) == 24 and len(mid) >= 8 and len(words) >= 40 and len(unknown) >= 2
    return {"dense": dense, "mid": mid, "words": words, "unknown": unknown, "docs": docs}


# ---- expression queries --------------------------------------------------------------------------------------------------
def expression_trees(side, seed, n=60):
    """n seeded trees of depth <= 3: AND / OR of 2-3 children and NOT; leaves that are a single gram, a whole word, or
    an unknown gram; the first few are fixed shapes: a lone NOT, a leaf repeated inside one tree, a bare leaf, NOT of an
    unknown leaf (the universe), AND with an empty child first (the reference's early exit)."""
    v = vocabulary(side)
    rng = np.random.default_rng(seed)

    def leaf():
        r = rng.random()
        if r < 0.55:
            return v["dense"][int(rng.integers(0, len(v["dense"])))]
        if r < 0.7:
            return v["mid"][int(rng.integers(0, len(v["mid"])))]
        if r < 0.9:
            return v["words"][int(rng.integers(0, len(v["words"])))]
        return v["unknown"][int(rng.integers(0, len(v["unknown"])))]

    def tree(depth):
        if depth == 0 or rng.random() < 0.2:
            return leaf()
        r = rng.random()
        if r < 0.2:
            return ("not", tree(depth - 1))
        return ("and" if r < 0.55 else "or",) + tuple(tree(depth - 1) for _ in range(int(rng.integers(2, 4))))

    a, b, w, u = v["dense"][0], v["dense"][3], v["words"][0], v["unknown"][0]
    trees = [("not", a), ("or", a, ("and", a, b)), a, ("not", u), ("and", u, a, b), ("and", ("not", w), ("or", w, b)),
             ("or", ("and", a, ("not", b)), ("and", b, ("not", a)), w)]
    while len(trees) < n:
        t = tree(3)
        if not isinstance(t, str):
            trees.append(t)
    return trees


def _depth(e):
    return 0 if isinstance(e, str) else 1 + max(_depth(k) for k in e[1:])


def expression_specs(side, seed, fuzzy=0):
    """Every tree with one combination of {no NOT term, one NOT term} x {no filter, filter row, negated filter row, typed
    condition} (all eight within any eight consecutive trees), every sixth tree with a universe narrower than the index,
    and each of those at every page shape of PAGES."""
    v = vocabulary(side)
    c = side.columns
    specs = []
    for i, t in enumerate(expression_trees(side, seed)):
        assert _depth(t) <= 3
        nots = [v["dense"][(5 + i) % len(v["dense"])]] if i % 2 else []
        filt = (None, "row", "not-row", "cond")[(i // 2) % 4]
        universe = (c.first_doc_id + 100, c.n_docs - 5000) if i % 6 == 5 else None
        for page in PAGES:
            specs.append(Spec("expr", expr=t, not_terms=nots, filt=filt, universe=universe, fuzzy=fuzzy, page=page))
    return specs


def is_flat(spec):
    """A bare leaf compiles to a flat program (the wave kernels may take it); every other tree pushes and pops."""
    return isinstance(spec.expr, str)


# ---- FUZZY term queries --------------------------------------------------------------------------------------------------
def _typo(word, rng):
    """One substitution in the middle of the word (edit distance 1)."""
    i = int(rng.integers(1, len(word) - 1))
    ch = "abcdefghijklmnopqrstuvwxyz"[int(rng.integers(0, 26))]
    if ch == word[i]:
        ch = "z" if ch != "z" else "y"
    return word[:i] + ch + word[i + 1:]


def fuzzy_specs(side, seed, n=40):
    """n FUZZY term queries: one and two terms in the order given (two terms out of ONE document, so the AND keeps
    something), a typo in the first or the second term, a term whose grams are all unknown, a three-letter term at
    distance 1 and a five-letter term at distance 2 (theta clamps to 1), NOT terms, the filter row, the typed condition,
    docid pages and SORT _score, with and without verify_text. Two queries carry a term shorter than one n-gram: the
    reference ends those with empty_term_detected, and they are the only ones whose counters may go uncompared."""
    v = vocabulary(side)
    rng = np.random.default_rng(seed)
    u = v["unknown"]
    pages = (dict(limit=0, descending=False), dict(limit=17), dict(sort_score=True, limit=10),
             dict(sort_score=True, limit=40, offset=1000))
    specs = []
    for i in range(n):
        d = v["docs"][int(rng.integers(0, len(v["docs"])))]
        pick = rng.choice(len(d), size=2, replace=False)
        first, second = d[int(pick[0])], d[int(pick[1])]
        distance = 1
        shape = i % 10
        if shape in (0, 5):
            terms = [_typo(first, rng)]
        elif shape in (1, 6):
            terms = [_typo(first, rng), second]
        elif shape in (2, 7):
            terms = [first, _typo(second, rng)]
        elif shape == 3:
            terms = [first, second]
        elif shape == 4:
            terms = [first[:3]]  # two grams, drop 2: theta = 1, the union of the grams
        elif shape == 8:
            terms, distance = [first[:5], second], 2  # four grams, drop 4: theta clamps to 1
        else:
            terms = [u[0] + u[1] + u[0]] if i < 20 else [first, u[0] + u[1]]  # every gram unknown
        if i in (13, 27):
            terms = terms[:1] + ["a"]  # shorter than one n-gram
        nots = [v["dense"][i % len(v["dense"])]] if i % 3 == 1 else []
        filt = (None, "row", "cond", "not-row", None)[i % 5]
        specs.append(Spec("fuzzy", terms=terms, not_terms=nots, filt=filt, fuzzy=distance, verify_text=i % 4 == 3,
                          page=pages[(i // 2) % 4]))
    return specs


# ---- expected values and coverage ----------------------------------------------------------------------------------------
def expected(side, specs, row, col):
    """[(total, page, scores or None, funnel dict)] of the oracle, one per spec."""
    return [side.oracle_query(s.query(row, col)) for s in specs]


def coverage(specs, want):
    """The shares the tests assert, from the oracle's side alone."""
    compared = [(s, r) for s, (_, _, _, r) in zip(specs, want) if not r["empty_term_detected"]]
    two = [(s, r) for s, r in compared if s.kind == "fuzzy" and len(s.terms) == 2]
    n = max(len(compared), 1)
    return {
        "queries": len(specs),
        "compared": len(compared),
        "skipped": len(specs) - len(compared),
        "total>0": sum(len(w[1]) > 0 or w[0] > 0 for w in want if not w[3]["empty_term_detected"]) / n,
        "after_not<after_intersection": sum(r["after_not"] < r["after_intersection"] for _, r in compared) / n,
        "after_filters<after_not": sum(r["after_filters"] < r["after_not"] for _, r in compared) / n,
        "two_term_fuzzy": len(two),
        "after_intersection<total_candidates": (sum(r["after_intersection"] < r["total_candidates"] for _, r in two)
                                                / max(len(two), 1)),
    }


def assert_coverage(cov, kind):
    """The conditions that keep a comparison from passing vacuously."""
    if kind == "expr":
        assert cov["skipped"] == 0, cov
    else:
        assert cov["skipped"] <= 4, cov
        assert cov["two_term_fuzzy"] >= 8 and cov["after_intersection<total_candidates"] >= 0.25, cov
    assert cov["total>0"] >= 0.5, cov
    assert cov["after_not<after_intersection"] >= 0.25, cov
    assert cov["after_filters<after_not"] >= 0.25, cov


def compare(specs, got, want):
    """Device results against the oracle's: total, page, scores bit for bit, empty_term_detected and — whenever the
    oracle did not end the query early — all four funnel counters. -> number of queries whose counters were compared."""
    n = 0
    for s, g, (total, page, scores, r) in zip(specs, got, want):
        ctx = (s.kind, s.expr, s.terms, s.not_terms, s.filt, s.universe, s.fuzzy, s.verify_text, s.page)
        got_c = tuple(int(getattr(g, k)) for k in COUNTERS)
        assert g.total == total, (ctx, g.total, total, got_c, [r[k] for k in COUNTERS])
        assert g.docs.tolist() == page.tolist(), ctx
        if scores is not None:
            assert np.array_equal(g.scores, scores), ctx
        assert g.empty_term_detected == r["empty_term_detected"], ctx
        if r["empty_term_detected"]:
            continue
        assert got_c == tuple(int(r[k]) for k in COUNTERS), (ctx, got_c, [r[k] for k in COUNTERS])
        n += 1
    return n


# ---- a table that changes after its build (tests/cpp/funnel_test.cpp replays this) ---------------------------------------
MUTABLE_WORDS = ("alpha", "beta", "gamma", "delta", "omega", "theta", "lambda", "sigma", "kappa")
SWAP_A, SWAP_B = "qxa", "qxb"  # their grams xa / xb occur in no other word: estimated size = the word's document count


def _ast_prefix(e):
    if isinstance(e, str):
        return "T:" + e
    return " ".join([{"and": "&", "or": "|", "not": "!"}[e[0]]] + [_ast_prefix(k) for k in e[1:]])


def mutable_case(seed=77, n_docs=20000):
    """-> (lines of the case file, summary). 20 000 initial documents over a small vocabulary (two tiles), then three
    checkpoints: after removes + updates + adds; after a second round that also changes and removes delta documents;
    after Compact() and one more round. The expected total, counters and ids of every query at every checkpoint come from
    the oracle over an index built from the documents current at that checkpoint.

    The term-order swap: SWAP_A holds fewer documents than SWAP_B at build time (300 / 320); round 1 removes 60 of
    SWAP_B's, so the reference would then start the query [SWAP_A, SWAP_B] from SWAP_B: total_candidates becomes SWAP_B's
    live count. That the oracle's term_order flips is asserted here."""
    from oracle import oracle as O
    rng = np.random.default_rng(seed)

    def text(extra=()):
        return " ".join([MUTABLE_WORDS[int(k)] for k in rng.integers(0, 9, int(rng.integers(2, 7)))] + list(extra))

    docs, lines = {}, []
    for d in range(1, n_docs + 1):
        extra = []
        if d % 50 == 7 and len([1 for v in docs.values() if SWAP_A in v[1]]) < 300:
            extra.append(SWAP_A)
        if d % 50 in (7, 9) and d > 5000 and len([1 for v in docs.values() if SWAP_B in v[1]]) < 320:
            extra.append(SWAP_B)
        if d % 500 == 3:
            extra.append("vanish")
        docs[d] = (int(rng.integers(-20000, 80000)), text(extra))
        lines.append("doc %d %d %s" % (d, docs[d][0], docs[d][1]))
    lines.append("build")

    def state():
        idx, store = O.Index(2, 0, False), O.DocumentStore()
        for d in sorted(docs):
            idx.add_document(d, docs[d][1])
            store.add(d, docs[d][1])
        return idx, store, np.asarray(sorted(docs), np.uint32)

    kw = dict(ngram_size=2, kanji_ngram_size=0, cross_boundary=False)
    queries = [("and1", dict(terms=["alpha"])), ("and2", dict(terms=["gamma", "ta"])),
               ("and3-not", dict(terms=["alpha", "ta", "ma"], nots=["kappa"])),
               ("and2-not", dict(terms=["sigma", "delta"], nots=["omega"])),
               ("changed-only", dict(terms=["zzqx"])), ("changed-and", dict(terms=["zzqx", "alpha"])),
               ("all-removed", dict(terms=["vanish"])), ("cond", dict(terms=["beta"], cond=30000)),
               ("cond-not", dict(terms=["theta", "am"], nots=["alpha"], cond=0)),
               ("swap", dict(terms=[SWAP_A, SWAP_B])),
               ("expr", dict(ast=("and", ("or", "alpha", "beta"), ("not", "omega")), nots=["kappa"])),
               ("lone-not", dict(ast=("not", "gamma"), cond=10000)),
               ("fuzzy", dict(terms=["lambda", "sigmq"], fuzzy=1, nots=["beta"]))]
    summary = {"checkpoints": [], "queries": len(queries)}

    def swap_order(idx, store):
        return O.execute(idx, store, [SWAP_A, SWAP_B], **kw)["term_order"]

    idx0, store0, _ = state()
    assert swap_order(idx0, store0) == [0, 1]  # at build time SWAP_A is the smaller
    assert idx0.posting_size("xa") == 300 and idx0.posting_size("xb") == 320

    def checkpoint(name):
        idx, store, all_docs = state()
        lines.append("checkpoint %s" % name)
        stats = {"name": name, "docs": len(docs), "term_order": swap_order(idx, store), "nonzero": 0,
                 "not_cut": 0, "filter_cut": 0}
        for label, q in queries:
            nots = q.get("nots", [])
            filters = []
            if "cond" in q:
                filters = [(np.asarray([d for d in sorted(docs) if docs[d][0] >= q["cond"]], np.uint32), False)]
            if "ast" in q:
                r = O.execute_boolean_ast(idx, store, q["ast"], (), nots, filters, all_docs=all_docs, **kw)
            elif q.get("fuzzy"):
                r = O.execute_fuzzy(idx, store, q["terms"], q["fuzzy"], nots, filters, **kw)
            else:
                r = O.execute(idx, store, q["terms"], nots, filters, **kw)
            lines.append("q %s" % label)
            for t in q.get("terms", []):
                lines.append("term %s" % t)
            for t in nots:
                lines.append("notterm %s" % t)
            if "ast" in q:
                lines.append("ast %s" % _ast_prefix(q["ast"]))
            if q.get("fuzzy"):
                lines.append("fuzzy %d" % q["fuzzy"])
            if "cond" in q:
                lines.append("cond %d" % q["cond"])
            res = r["results"].tolist()
            lines.append("expect %d %d %d %d %d %d %s" % (r["empty_term_detected"], len(res), r["total_candidates"],
                                                          r["after_intersection"], r["after_not"], r["after_filters"],
                                                          " ".join(map(str, res))))
            lines.append("end")
            if label == "swap":
                stats["swap_total_candidates"] = r["total_candidates"]
                stats["swap_b_live"] = sum(SWAP_B in v[1].split(" ") for v in docs.values())
            if label == "all-removed":
                stats["all_removed_empty"] = r["empty_term_detected"]
            stats["nonzero"] += len(res) > 0
            stats["not_cut"] += r["after_not"] < r["after_intersection"]
            stats["filter_cut"] += r["after_filters"] < r["after_not"]
        lines.append("run")
        summary["checkpoints"].append(stats)
        return stats

    def remove(d):
        lines.append("remove %d" % d)
        del docs[d]

    def update(d, extra=()):
        docs[d] = (docs[d][0], text(extra))
        lines.append("update %d %s" % (d, docs[d][1]))

    def add(d, extra=()):
        docs[d] = (int(rng.integers(-20000, 80000)), text(extra))
        lines.append("add %d %d %s" % (d, docs[d][0], docs[d][1]))

    # round 1: every "vanish" document and 60 of SWAP_B's leave, 100 more are removed, 200 change, 150 arrive
    for d in [d for d in sorted(docs) if "vanish" in docs[d][1]]:
        remove(d)
    for d in [d for d in sorted(docs) if SWAP_B in docs[d][1] and SWAP_A not in docs[d][1]][:60]:
        remove(d)
    for d in rng.choice(sorted(docs), size=100, replace=False).tolist():
        if SWAP_A not in docs[d][1] and SWAP_B not in docs[d][1]:
            remove(d)
    for k, d in enumerate(rng.choice(sorted(docs), size=200, replace=False).tolist()):
        if SWAP_A not in docs[d][1] and SWAP_B not in docs[d][1]:
            update(d, ["zzqx"] if k % 4 == 0 else [])
    for d in range(n_docs + 1, n_docs + 151):
        add(d, ["zzqx"] if d % 5 == 0 else [])
    s1 = checkpoint("round 1")
    # round 2: delta documents change and leave too
    for k, d in enumerate([d for d in sorted(docs) if d > n_docs][:40]):
        remove(d) if k % 2 == 0 else update(d, ["zzqx"] if k % 3 == 0 else [])
    for d in rng.choice([d for d in sorted(docs) if d <= n_docs], size=80, replace=False).tolist():
        if SWAP_A not in docs[d][1] and SWAP_B not in docs[d][1]:
            remove(d) if d % 2 else update(d)
    s2 = checkpoint("round 2")
    # round 3: the delta is folded back, then one more round
    lines.append("compact")
    for d in rng.choice(sorted(docs), size=60, replace=False).tolist():
        if SWAP_A not in docs[d][1] and SWAP_B not in docs[d][1]:
            update(d, ["zzqx"] if d % 7 == 0 else [])
    for d in range(n_docs + 151, n_docs + 201):
        add(d)
    s3 = checkpoint("round 3")
    for s in (s1, s2, s3):
        # the order flipped: the query now starts from SWAP_B, whose live count is what total_candidates must be
        assert s["term_order"] == [1, 0] and s["swap_total_candidates"] == s["swap_b_live"] == 260, s
        assert s["all_removed_empty"] and s["nonzero"] >= 10 and s["not_cut"] >= 4 and s["filter_cut"] >= 3, s
    return lines, summary
