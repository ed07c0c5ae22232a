"""CPU only: the boolean-AST oracle (oracle/mygram_oracle.c orc_execute_boolean_ast / orc_collect_ast_scoring_terms)
against the reference's own vectors and against a second, independent restatement; and the query generators of the
funnel-counter tests run through the oracle alone, with the coverage conditions the device tests rely on."""
import os
import subprocess

import numpy as np
import pytest

import funnel_util as FU
import golden_util as G
from gpu_util import OracleSide
from oracle import oracle as O
from pkg import mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ast_fixture(g, case):
    docs = g["docs"] + case["extra_docs"]
    idx = O.Index(g["index"]["ngram"], g["index"]["kanji"], True)
    store = O.DocumentStore()
    for d, t in docs:
        idx.add_document(d, t)
        store.add(d, t)
    return idx, store, [d for d, _ in docs]


def _tuple_tree(t):
    return t if isinstance(t, str) else tuple([t[0]] + [_tuple_tree(k) for k in t[1:]])


def test_boolean_ast_vectors():
    """tests/server/search_pipeline_test.cpp:1122-1392 (fixture :916-951): the result ids of ExecuteFullPipeline's
    boolean-AST branch, and_terms and FUZZY leaves included, and the scored terms of :1350-1392 / :1303-1319."""
    g = G.load("pipeline.json")["boolean_ast"]
    qp = g["query_params"]
    assert len(g["cases"]) >= 8 and any(c["and_terms"] for c in g["cases"])
    for case in g["cases"]:
        idx, store, all_docs = _ast_fixture(g, case)
        tree = _tuple_tree(case["tree"])
        r = O.execute_boolean_ast(idx, store, tree, case["and_terms"], case["not_terms"], (), all_docs=all_docs,
                                  fuzzy=case["fuzzy"], ngram_size=qp["ngram"], kanji_ngram_size=qp["kanji"],
                                  cross_boundary=qp["cross_boundary"])
        assert r["results"].tolist() == case["expect_results"], (case["id"], case["source"])
        assert r["after_filters"] == len(case["expect_results"]) and not r["empty_term_detected"], case["id"]
        if "expect_scoring_terms" in case:
            assert O.collect_ast_scoring_terms(tree) == case["expect_scoring_terms"], case["id"]


def test_boolean_ast_and_terms_exit_and_null_children():
    """search_pipeline.cpp:1488-1492: an and_term without documents ends the query with empty_term_detected and leaves
    after_intersection / after_not / after_filters at 0 while total_candidates keeps the tree's count; :337-339, :358,
    :366-368: a null child empties an AND, is skipped by an OR and makes a NOT the universe."""
    g = G.load("pipeline.json")["boolean_ast"]
    idx, store, all_docs = _ast_fixture(g, g["cases"][0])
    kw = dict(all_docs=all_docs, ngram_size=2, kanji_ngram_size=0, cross_boundary=False)
    r = O.execute_boolean_ast(idx, store, ("or", "basics", "cats"), ["zebra"], **kw)
    assert r["empty_term_detected"] and r["results"].tolist() == []
    assert (r["total_candidates"], r["after_intersection"], r["after_not"], r["after_filters"]) == (2, 0, 0, 0)
    assert O.execute_boolean_ast(idx, store, ("and", "learning", None), **kw)["results"].tolist() == []
    assert O.execute_boolean_ast(idx, store, ("or", None, "cats"), **kw)["results"].tolist() == [3]
    assert O.execute_boolean_ast(idx, store, ("not", None), **kw)["results"].tolist() == [1, 2, 3]
    # the universe is read only for a tree that holds a NOT (:1469)
    assert O.execute_boolean_ast(idx, store, ("or", "cats", ("not", "old")), **kw)["results"].tolist() == [1, 2, 3]


def test_boolean_ast_replay_program(tmp_path):
    """The vectors once more through a stand-alone C program over mygram_oracle.c (tests/cpp/oracle_ast_replay.c): the
    restatement as C sees it, without ctypes in between. (`make -C oracle replay-asan` builds the same program with
    -fsanitize=address,undefined.)"""
    g = G.load("pipeline.json")["boolean_ast"]
    case_file = tmp_path / "ast_cases.txt"
    case_file.write_text("\n".join(replay_lines(g)) + "\n", encoding="utf-8")
    exe = tmp_path / "oracle_ast_replay"
    subprocess.run(["gcc", "-O1", "-std=c11", "-I", os.path.join(ROOT, "oracle"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "oracle_ast_replay.c"),
                    os.path.join(ROOT, "oracle", "mygram_oracle.c"), "-lm"], check=True)
    r = subprocess.run([str(exe), str(case_file)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases ok" % len(g["cases"]) in r.stdout, r.stdout


def replay_lines(g):
    """The boolean_ast vectors in the line format tests/cpp/oracle_ast_replay.c reads (text last on every line)."""
    qp = g["query_params"]
    lines = []
    for case in g["cases"]:
        lines.append("case %s" % case["id"])
        lines.append("config %d %d %d %d %d" % (g["index"]["ngram"], g["index"]["kanji"], qp["ngram"], qp["kanji"],
                                                int(qp["cross_boundary"])))
        for d, t in g["docs"] + case["extra_docs"]:
            lines.append("doc %d %s" % (d, t))
        arr, kids, leaves = O._flatten_tree(_tuple_tree(case["tree"]))
        for leaf in leaves:
            lines.append("leaf %s" % leaf)
        for n in arr:
            lines.append("node %d %d %d %d" % (n.type, n.term, n.first_kid, n.n_kids))
        for k in kids[:-1].tolist():
            lines.append("kid %d" % k)
        for t in case["and_terms"]:
            lines.append("and %s" % t)
        for t in case["not_terms"]:
            lines.append("not %s" % t)
        lines.append("fuzzy %d" % case["fuzzy"])
        lines.append("expect %s" % " ".join(str(d) for d in case["expect_results"]))
        if "expect_scoring_terms" in case:
            at, where = 0, []  # the expected terms as leaf positions: each the next leaf of that text, left to right
            for t in case["expect_scoring_terms"]:
                at = leaves.index(t, at) + 1
                where.append(at - 1)
            lines.append("scoring %s" % " ".join(str(k) for k in where))
        lines.append("run")
    return lines


# ---- the second restatement: a Python set fold ---------------------------------------------------------------------------

def _fold(side, e, universe, fuzzy=0):
    """EvaluateBooleanAstExpanded (src/server/search_pipeline.cpp:327-378) over Python sets; a leaf is the AND of its
    query n-grams (Index::SearchAnd) or, with fuzzy, Index::SearchByThreshold at the leaf's theta."""
    if isinstance(e, str):
        grams = sorted(set(O.generate_query_ngrams(O.normalize_text(e), side.ngram_size, side.kanji_ngram_size,
                                                  side.cross_boundary)))
        if not grams:
            return set()
        if fuzzy:
            drop = fuzzy * side.ngram_size
            return set(side.oidx.search_by_threshold(grams, len(grams) - drop if len(grams) > drop else 1).tolist())
        return set(side.oidx.search_and(grams).tolist())
    kids = [_fold(side, c, universe, fuzzy) for c in e[1:]]
    if e[0] == "and":
        return set.intersection(*kids)
    if e[0] == "or":
        return set.union(*kids)
    return universe - kids[0]


@pytest.fixture(scope="module")
def side():
    corpus = mg.Corpus.synthetic(6000, seed=23)
    s = OracleSide(mg.Columns(corpus, 1, 2, 0, True), corpus)
    FU.register_cpu(s)
    return s


def test_boolean_ast_agrees_with_a_set_fold_on_random_trees(side):
    """240 seeded random trees (depth <= 3, NOT nodes, unknown leaves, multi-gram leaves; half of them with FUZZY 1 on
    every leaf), each with 0-1 NOT terms and 0-2 filters: the C restatement's result set equals a Python set fold's,
    total_candidates == after_intersection == |tree result| (no and_terms), after_not and after_filters equal the
    fold's sizes after the NOT terms and after the filters.

    The reference's tests assert no funnel counter for the boolean-AST branch (only
    tests/server/search_pipeline_test.cpp:990-993, for the plain path), so the counters of that branch rest on the
    line-cited restatement in oracle/mygram_oracle.c plus this fold."""
    c = side.columns
    v = FU.vocabulary(side)
    rng = np.random.default_rng(99)
    trees = FU.expression_trees(side, seed=5, n=120) + FU.expression_trees(side, seed=6, n=120)
    assert len(trees) >= 200
    row = side.filters[0]
    cond_docs, _ = side.condition_docs((0, FU.OPS.index("<"), FU.COND_LITERAL))
    shapes = {"not": 0, "unknown": 0, "word": 0, "nonempty": 0}
    for i, t in enumerate(trees):
        fuzzy = i % 2
        lo, hi = (c.first_doc_id, c.first_doc_id + c.n_docs) if i % 5 else (c.first_doc_id + 50, c.first_doc_id + 4000)
        universe = set(range(lo, hi))
        nots = [v["dense"][int(rng.integers(0, 24))]] if i % 3 else []
        filters = [(row, bool(i % 4 == 1))] * (i % 4 in (1, 2)) + [(cond_docs, False)] * (i % 4 in (2, 3))
        r = O.execute_boolean_ast(side.oidx, side.ostore, t, (), nots, filters,
                                  all_docs=np.arange(lo, hi, dtype=np.uint32), fuzzy=fuzzy, ngram_size=2,
                                  kanji_ngram_size=0, cross_boundary=True)
        res = _fold(side, t, universe, fuzzy)
        assert r["total_candidates"] == r["after_intersection"] == len(res), (i, t)
        for nt in nots:
            res = res - _fold(side, nt, universe)
        assert r["after_not"] == len(res), (i, t, nots)
        for docs, neg in filters:
            res = (res - set(docs.tolist())) if neg else (res & set(docs.tolist()))
        assert r["after_filters"] == len(res), (i, t)
        assert r["results"].tolist() == sorted(res), (i, t)
        assert not r["empty_term_detected"]
        text = repr(t)
        shapes["not"] += "'not'" in text
        shapes["unknown"] += any(repr(u) in text for u in v["unknown"])
        shapes["word"] += any(repr(w) in text for w in v["words"])
        shapes["nonempty"] += len(res) > 0
    assert shapes["not"] >= 60 and shapes["unknown"] >= 30 and shapes["word"] >= 60 and shapes["nonempty"] >= 80, shapes


def test_scoring_terms_of_random_trees(side):
    """CollectAstScoringTerms against its definition written the other way round: walk the leaves left to right and
    keep those with no NOT among their ancestors."""
    def walk(e, path, out):
        if isinstance(e, str):
            if "not" not in path:
                out.append(e)
            return out
        for k in e[1:]:
            walk(k, path + (e[0],), out)
        return out
    for t in FU.expression_trees(side, seed=7, n=80):
        assert O.collect_ast_scoring_terms(t) == walk(t, (), []), t


# ---- the generators of test_gpu_funnel.py, through the oracle alone ------------------------------------------------------

@pytest.fixture(scope="module", params=["bitmap", "lists"])
def big_side(request):
    n = FU.BITMAP_DOCS if request.param == "bitmap" else FU.LISTS_DOCS
    corpus = mg.Corpus.synthetic(n, seed=61 if request.param == "bitmap" else 62)
    s = OracleSide(mg.Columns(corpus, 1, 2, 0, True), corpus)
    FU.register_cpu(s)
    return s


@pytest.mark.parametrize("fuzzy", [0, 1])
def test_expression_generator_meets_its_coverage_conditions(big_side, fuzzy):
    specs = FU.expression_specs(big_side, seed=101, fuzzy=fuzzy)
    want = FU.expected(big_side, specs, 0, 0)
    cov = FU.coverage(specs, want)
    print("expression fuzzy=%d n_docs=%d: %s" % (fuzzy, big_side.columns.n_docs, cov))
    assert cov["queries"] == 60 * len(FU.PAGES)
    FU.assert_coverage(cov, "expr")
    assert sum(not FU.is_flat(s) for s in specs) >= 50 * len(FU.PAGES)
    assert any(s.universe for s in specs) and any(s.expr[0] == "not" for s in specs if not FU.is_flat(s))


def test_fuzzy_generator_meets_its_coverage_conditions(big_side):
    specs = FU.fuzzy_specs(big_side, seed=202)
    want = FU.expected(big_side, specs, 0, 0)
    cov = FU.coverage(specs, want)
    print("fuzzy terms n_docs=%d: %s" % (big_side.columns.n_docs, cov))
    assert cov["queries"] == 40
    FU.assert_coverage(cov, "fuzzy")
    thetas = [O.execute_fuzzy(big_side.oidx, big_side.ostore, s.terms, s.fuzzy, ngram_size=2, kanji_ngram_size=0,
                              cross_boundary=True)["thetas"] for s in specs if len(s.terms[-1]) >= 2]
    assert sum(th[0] == 1 for th in thetas) >= 6  # theta clamped to 1
    assert sum(s.verify_text for s in specs) >= 8 and sum(bool(s.page.get("sort_score")) for s in specs) >= 16


def test_changed_table_case_file_and_the_term_order_swap():
    """The case file of tests/test_gpu_funnel_cpp.py, with the oracle alone: the swap query's term order flips between the
    build and every checkpoint, its expected total_candidates is the second term's live count, the term whose documents
    were all removed ends the query with empty_term_detected, and enough queries match, lose documents to their NOT
    terms and to their conditions (mutable_case asserts all of it)."""
    lines, summary = FU.mutable_case()
    print(summary)
    assert len(summary["checkpoints"]) == 3 and summary["queries"] == 13
    assert sum(ln == "compact" for ln in lines) == 1 and sum(ln == "run" for ln in lines) == 3


def test_seven_document_known_answers_hold_in_the_oracle():
    """The hand-written counters and ids of test_gpu_funnel.py's seven-document table, with the oracle alone."""
    from gpu_util import densify
    from test_gpu_funnel import SMALL
    first, texts = densify(FU.SMALL_DOCS)
    corpus = mg.Corpus.from_texts(texts)
    s = OracleSide(mg.Columns(corpus, first, 2, 0, True), corpus)
    s.filters[0] = np.asarray([1, 2, 3, 4], np.uint32)
    s.typed[0] = (np.asarray([5, 20, 5, 20, 5, 20, 5], np.int64), np.asarray([False] * 6 + [True]))
    for kw, counters, ids in SMALL:
        kw = dict(kw)
        kw["filters"] = [(0, neg) for _, neg in kw.get("filters", [])]
        kw["conditions"] = [(0, FU.OPS.index(op), lit, 0.0, False, False, False) for _, op, lit in kw.get("conditions", [])]
        total, page, _, r = s.oracle_query(mg.engine.Query(limit=0, descending=False, **kw))
        assert tuple(r[k] for k in FU.COUNTERS) == counters and page.tolist() == ids and total == len(ids), kw
