"""CPU only: expr_verify_ref.py — the expectation test_gpu_expr_verify.py compares the device with — against the
reference's two known-answer vectors for expression queries under verify_text (tests/golden/expr_verify.json), against
the hand-worked cases of the device test, and the coverage conditions of the generated query sets, so that the device
comparison cannot pass vacuously."""
import numpy as np
import pytest

import expr_verify_ref as EV
import funnel_util as FU
from gpu_util import OracleSide, densify
from pkg import mg

Query = mg.engine.Query


def _side(docs, cross):
    first, texts = densify(docs)
    corpus = mg.Corpus.from_texts(texts)
    return OracleSide(mg.Columns(corpus, first, 2, 0, cross), corpus, first)


def _golden_sides():
    g = EV.golden()
    assert len(g["cases"]) == 2 and (g["index"]["ngram"], g["index"]["kanji"], g["index"]["cross_boundary"]) == (2, 0, False)
    for case in g["cases"]:
        docs = [tuple(d) for d in g["docs"] + case["extra_docs"]]
        yield case, _side(docs, False), Query(expr=EV.tuple_tree(case["tree"]), fuzzy=case["fuzzy"], verify_text=True,
                                             limit=0, descending=False)


def test_helper_reproduces_the_reference_vectors():
    for case, side, q in _golden_sides():
        total, page, _, _ = EV.Reference(side).expected(q)
        assert page.tolist() == case["expect"] and total == len(case["expect"]), (case["id"], page)


def test_tree_rule_differs_from_every_term_rule_on_the_vectors():
    """"Every term must occur" (the rule of the conjunctive path) empties both vectors: no document holds both leaves."""
    for case, side, q in _golden_sides():
        _, cand, kept, every = EV.Reference(side).candidates(q)
        assert kept.tolist() == case["expect"] and every.tolist() == [] and len(cand) >= len(kept), case["id"]
    case, side, q = next(_golden_sides())
    assert EV.Reference(side).candidates(q)[1].tolist() == [3, 4]  # the set algebra's false positive: abzzba


def test_hand_worked_cases_hold_in_the_helper():
    from test_gpu_expr_verify import SMALL, SMALL_DOCS, small_queries
    s = _side(SMALL_DOCS, True)
    s.filters[0] = np.asarray([1, 2, 3, 4, 8], np.uint32)
    ref = EV.Reference(s)
    qs = small_queries(0)
    assert len(SMALL) >= 6
    for (kw, counters, ids), q in zip(SMALL, qs[::2]):
        total, page, _, r = ref.expected(q)
        assert page.tolist() == ids and total == len(ids), (kw, page)
        assert tuple(int(r[k]) for k in FU.COUNTERS) == counters, (kw, [r[k] for k in FU.COUNTERS])


@pytest.fixture(scope="module", params=["bitmap", "lists"])
def big_side(request):
    n = FU.BITMAP_DOCS if request.param == "bitmap" else FU.LISTS_DOCS
    corpus = mg.Corpus.synthetic(n, seed=61 if request.param == "bitmap" else 62)
    s = OracleSide(mg.Columns(corpus, 1, 2, 0, True), corpus)
    FU.register_cpu(s)
    return s


@pytest.mark.parametrize("fuzzy", [0, 1])
def test_funnel_generator_meets_the_coverage_conditions(big_side, fuzzy):
    ref = EV.Reference(big_side)
    qs = EV.funnel_queries(big_side, 0, 0, fuzzy)
    assert len(qs) == 300
    cov = ref.coverage(qs[::len(FU.PAGES)])
    print(cov)
    EV.assert_funnel_coverage(cov, fuzzy)


@pytest.mark.parametrize("fuzzy", [0, 1])
def test_hard_corpus_meets_the_coverage_conditions(fuzzy):
    texts, cases = EV.hard_case()
    assert len(texts) == EV.HARD_DOCS and len(cases) == EV.HARD_TREES
    assert sum(bool(n) for _, n, _ in cases) == 20 and sum(f for _, _, f in cases) == 20
    corpus = mg.Corpus.from_texts(texts)
    s = OracleSide(mg.Columns(corpus, 1, 2, 0, True), corpus)
    s.filters[0] = FU.filter_row_docs(s)
    qs = EV.hard_queries(cases, 0, fuzzy)
    ref = EV.Reference(s)
    cov = ref.coverage(qs[::len(EV.HARD_PAGES)])
    print(cov)
    EV.assert_hard_coverage(cov)
    # scored pages exist and hold something: the tree's positive leaves are scored from the texts
    scored = [ref.expected(q) for q in qs[1::2][:8]]
    assert sum(len(p) > 0 for _, p, _, _ in scored) >= 4


def test_shim_case_file():
    """The case file of tests/cpp/expr_verify_test.cpp: both vectors, the FUZZY tree without verify_text, a delta."""
    lines, summary = EV.shim_case()
    assert summary == dict(runs=4, cut=summary["cut"], delta_runs=1, queries=17) and summary["cut"] >= 4, summary
    assert sum(ln.startswith("expect ") for ln in lines) == 17 and "delta 6" in lines
