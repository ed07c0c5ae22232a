"""-m gpu: verify_text on boolean-expression queries — the tree re-evaluated over each candidate's text on the device
(kOpVerifyTree) — through engine.py. ExecuteWithBooleanAst (src/server/search_pipeline.cpp:1505-1578) applies the filter
after NOT terms and filters: a candidate stays when the tree is true over its stored text, a leaf being text.find(term)
or, under FUZZY d, that or ContainsFuzzyMatch. The oracle does not restate that branch: expectations come from
expr_verify_ref.py (test_expr_verify_cpu.py pins it to the reference's own vectors and checks the coverage conditions of
the generated sets). Everything compared is an integer or an fp64 score bit for bit: total, page, scores and the four
funnel counters (after_filters counts the documents BEFORE the text filter, total those after it)."""
import ctypes as C

import numpy as np
import pytest

import expr_verify_ref as EV
import funnel_util as FU
from gpu_util import Pair
from pkg import mg
from test_gpu_batch_conditions import _routes

pytestmark = pytest.mark.gpu
Query = mg.engine.Query

SMALL_DOCS = FU.SMALL_DOCS + [(8, "abzzba")]
_ROW = "row"  # the filter row {1, 2, 3, 4, 8}
# (query, (total_candidates, after_intersection, after_not, after_filters), ascending doc ids), all with verify_text —
# worked out by hand. "abab" is the grams ab + ba: document 8 holds both, its text does not hold "abab".
SMALL = [
    (dict(expr=("or", "abab", "cats")), (3, 3, 3, 3), [3, 5]),
    (dict(expr=("not", "abab")), (7, 7, 7, 7), [1, 2, 3, 4, 5, 6, 7]),  # 8 stays out: the filter only narrows
    (dict(expr=("and", "cats", ("not", "abab"))), (2, 2, 2, 2), [3, 5]),
    (dict(expr=("or", "abab", "cats"), not_terms=["machine"]), (3, 3, 2, 2), [3]),
    (dict(expr=("or", "abab", "basics"), filters=[(_ROW, False)]), (4, 4, 4, 2), [1]),
    # FUZZY 1: goleng = at least 3 of go ol le en ng -> {7}; abab = ab or ba -> {1, 3, 6, 7, 8}; no word is within one
    # edit of abab, golang is one edit from goleng
    (dict(expr=("or", "goleng", "abab"), fuzzy=1), (5, 5, 5, 5), [7]),
    # zebra has unknown grams: the empty set under the NOT, and false on every text
    (dict(expr=("and", "basics", ("not", "zebra"))), (3, 3, 3, 3), [1, 6, 7]),
    # "a" is shorter than one n-gram: a FUZZY leaf without grams is the empty set (:1431-1433), so the set algebra keeps
    # 1, 6, 7 — but every text holds "a", so NOT a is false on all of them
    (dict(expr=("and", "basics", ("not", "a")), fuzzy=1), (3, 3, 3, 3), []),
]


def small_queries(row):
    """Every case as an ascending docid page and (where the engine scores the shape) as SORT _score top 10."""
    qs = []
    for kw, _, _ in SMALL:
        kw = dict(kw)
        kw["filters"] = [(row, neg) for _, neg in kw.get("filters", [])]
        qs.append(Query(limit=0, descending=False, verify_text=True, **kw))
        short = any(len(t) < 2 for t in EV.tree_terms(kw["expr"]))  # (a leaf without n-grams is not scored on the device)
        qs.append(Query(verify_text=True, **(dict(limit=17) if short else dict(sort_score=True, limit=10)), **kw))
    return qs


@pytest.mark.parametrize("dense_threshold", [0.0, 2.0])
def test_reference_vectors_and_hand_worked_cases(dense_threshold):
    g = EV.golden()
    for case in g["cases"]:
        p = Pair(docs=[tuple(d) for d in g["docs"] + case["extra_docs"]], ngram=g["index"]["ngram"],
                 kanji=g["index"]["kanji"], cross=g["index"]["cross_boundary"], dense_threshold=dense_threshold)
        q = Query(expr=EV.tuple_tree(case["tree"]), fuzzy=case["fuzzy"], verify_text=True, limit=0, descending=False)
        qs = [q, Query(expr=q.expr, fuzzy=q.fuzzy, verify_text=True, sort_score=True, limit=10)]
        got = p.dev.search_batch(qs)
        assert got[0].docs.tolist() == case["expect"] and got[0].total == len(case["expect"]), (case["id"], got[0].docs)
        assert sorted(got[1].docs.tolist()) == case["expect"], case["id"]
        EV.compare(qs, got, EV.Reference(p))
    p = Pair(docs=SMALL_DOCS, ngram=2, kanji=0, dense_threshold=dense_threshold)
    row = p.add_filter([1, 2, 3, 4, 8])
    qs = small_queries(row)
    got = p.dev.search_batch(qs)
    EV.compare(qs, got, EV.Reference(p))
    for i, (kw, counters, ids) in enumerate(SMALL):
        for g_ in got[2 * i: 2 * i + 2]:
            assert tuple(int(getattr(g_, k)) for k in FU.COUNTERS) == counters, kw
            assert g_.total == len(ids) and sorted(g_.docs.tolist()) == ids, (kw, g_.docs)


class Table:
    def __init__(self, p):
        self.p = p
        self.row = p.add_filter(FU.filter_row_docs(p))
        self.col = p.add_column(*FU.typed_column(p))
        self.ref = EV.Reference(p)  # (candidates and leaf matches are computed once and shared)


@pytest.fixture(scope="module")
def bitmap():
    return Table(Pair(corpus=mg.Corpus.synthetic(FU.BITMAP_DOCS, seed=61), dense_threshold=0.0))


@pytest.fixture(scope="module")
def lists():
    return Table(Pair(corpus=mg.Corpus.synthetic(FU.LISTS_DOCS, seed=62), dense_threshold=2.0))


@pytest.mark.parametrize("fuzzy", [0, 1])
@pytest.mark.parametrize("index", ["bitmap", "lists"])
def test_funnel_generator_verified(index, fuzzy, request, monkeypatch, capfd):
    """60 trees x 5 page shapes (docid pages of limit 0 / 17 / 20000, SORT _score top 10 and the deep score page), plain
    and FUZZY 1, on the three-tile bitmap index and the lists-only index, default routing and MGX_FORCE_BLOCK_KERNEL=1."""
    t = request.getfixturevalue(index)
    qs = EV.funnel_queries(t.p, t.row, t.col, fuzzy)
    assert len(qs) == 300
    EV.assert_funnel_coverage(t.ref.coverage(qs[::len(FU.PAGES)]), fuzzy)
    for env in ({}, {"MGX_FORCE_BLOCK_KERNEL": "1"}):
        got, n = _routes(t.p.dev, qs, monkeypatch, capfd, env)
        assert n["block"] > 0 and n["fast"] == n["wave"] == n["cand"] == 0, (env, n)  # the op runs on the general kernel only
        EV.compare(qs, got, t.ref)


@pytest.fixture(scope="module")
def hard():
    texts, cases = EV.hard_case()
    p = Pair(corpus=mg.Corpus.from_texts(texts))
    return p, cases, p.add_filter(FU.filter_row_docs(p)), EV.Reference(p)


@pytest.mark.parametrize("fuzzy", [0, 1])
def test_corpus_of_false_positives(hard, fuzzy):
    """Words of 2-5 letters over "abc": a quarter and more of the set algebra's candidates fail on the text."""
    p, cases, row, ref = hard
    qs = EV.hard_queries(cases, row, fuzzy)
    EV.assert_hard_coverage(ref.coverage(qs[::len(EV.HARD_PAGES)]))
    EV.compare(qs, p.dev.search_batch(qs), ref)


def _raw(dev, q):
    cqs, keep, shells = dev.prepare([q], into="raw")
    assert shells == [None]
    return cqs[0], keep


def _prepare_fails(dev, cq):
    h = C.c_void_p()
    rc = mg._capi.load().mgx_batch_prepare(dev.device_index._h, (mg._capi.Query * 1)(cq), 1, C.byref(h))
    assert h.value is None
    return rc


def test_refusals():
    INVALID = 2  # MGX_ERR_INVALID_ARGUMENT
    p = Pair(docs=SMALL_DOCS, ngram=2, kanji=0)
    # an index without attached texts (nothing so far asked for them)
    cq, keep = _raw(p.dev, Query(expr=("or", "abab", "cats"), limit=0))
    cq.exact_text = 1
    assert _prepare_fails(p.dev, cq) == INVALID
    # both fields together
    cq, keep = _raw(p.dev, Query(expr=("or", "abab", "cats"), verify_text=True, limit=0))
    assert cq.exact_text == 1 and cq.fuzzy_verify_distance == 0 and cq.n_expr == 3
    cq.fuzzy_verify_distance = 1
    assert _prepare_fails(p.dev, cq) == INVALID
    # a leaf without its text
    cq, keep = _raw(p.dev, Query(expr=("or", "abab", "cats"), fuzzy=1, verify_text=True, limit=0))
    assert cq.exact_text == 0 and cq.fuzzy_verify_distance == 1
    terms = C.cast(cq.terms, C.POINTER(mg._capi.Term))
    assert terms[1].text and terms[1].text_len == 4
    terms[1].text, terms[1].text_len = None, 0
    assert _prepare_fails(p.dev, cq) == INVALID
    # ... and the same queries untouched are served
    got = p.dev.search_batch([Query(expr=("or", "abab", "cats"), verify_text=True, limit=0, descending=False)])
    assert got[0].docs.tolist() == [3, 5]
