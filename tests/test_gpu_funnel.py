"""-m gpu: the four funnel counters (total_candidates, after_intersection, after_not, after_filters) of boolean-expression
and FUZZY queries against the oracle's restatement of ExecuteWithBooleanAst / ExecuteWithFuzzy, beside the page, total
and score parity the rest of the suite asserts. The device produces the counters with kOpCount instructions that every
kernel counts in its own way; a miscount changes these numbers and nothing else.

Shapes are the smallest at which the counting can go wrong: a bitmap index of three tiles with a partial last tile and a
last bitmap word that is not full, a lists-only index of two tiles whose every operand is a sorted list, and a
seven-document table with answers written out by hand. The queries come from funnel_util.py, whose coverage conditions
(test_funnel_queries_cpu.py checks the same without a device) keep the comparison from passing vacuously. Everything
compared is an integer or an fp64 score bit for bit: no tolerance."""
import numpy as np
import pytest

import funnel_util as FU
from gpu_util import Pair
from pkg import mg
from test_gpu_batch_conditions import _routes

pytestmark = pytest.mark.gpu
Query = mg.engine.Query


class Table:
    """A Pair with the filter row and the typed column of funnel_util registered, and the oracle's answers cached."""

    def __init__(self, p):
        self.p = p
        self.row = p.add_filter(FU.filter_row_docs(p))
        self.col = p.add_column(*FU.typed_column(p))
        self._cache = {}

    def family(self, name):
        """(specs, queries, oracle answers) of one query family, computed once and left unchanged."""
        if name not in self._cache:
            specs = {"expr": lambda: FU.expression_specs(self.p, seed=101),
                     "expr-fuzzy": lambda: FU.expression_specs(self.p, seed=101, fuzzy=1),
                     "fuzzy": lambda: FU.fuzzy_specs(self.p, seed=202)}[name]()
            want = FU.expected(self.p, specs, self.row, self.col)
            FU.assert_coverage(FU.coverage(specs, want), "fuzzy" if name == "fuzzy" else "expr")
            self._cache[name] = (specs, [s.query(self.row, self.col) for s in specs], want)
        return self._cache[name]


@pytest.fixture(scope="module")
def bitmap():
    return Table(Pair(corpus=mg.Corpus.synthetic(FU.BITMAP_DOCS, seed=61), dense_threshold=0.0))


@pytest.fixture(scope="module")
def lists():
    return Table(Pair(corpus=mg.Corpus.synthetic(FU.LISTS_DOCS, seed=62), dense_threshold=2.0))


@pytest.mark.parametrize("family", ["expr", "expr-fuzzy"])
@pytest.mark.parametrize("index", ["bitmap", "lists"])
def test_expression_counters_on_every_route(index, family, request, monkeypatch, capfd):
    """60 trees x 5 page shapes (plain, or FUZZY 1 on every leaf): every query's four counters equal the oracle's, under
    the default routing and with MGX_FORCE_BLOCK_KERNEL=1; the trees that push and pop run on the general workgroup
    kernel (tile_eval_kernel) either way, which the route report confirms."""
    t = request.getfixturevalue(index)
    specs, qs, want = t.family(family)
    for env in ({}, {"MGX_FORCE_BLOCK_KERNEL": "1"}):
        got, n = _routes(t.p.dev, qs, monkeypatch, capfd, env)
        assert FU.compare(specs, got, want) == len(specs) == 300, env
        assert n["block"] > 0, (env, n)
        if env:
            assert n["fast"] == n["wave"] == n["cand"] == 0, n
    deep = [i for i, s in enumerate(specs) if not FU.is_flat(s)]
    assert len(deep) >= 250
    got, n = _routes(t.p.dev, [qs[i] for i in deep], monkeypatch, capfd, {})
    assert n["block"] > 0 and n["fast"] == n["wave"] == n["cand"] == 0, n
    assert FU.compare([specs[i] for i in deep], got, [want[i] for i in deep]) == len(deep)


@pytest.mark.parametrize("index", ["bitmap", "lists"])
def test_fuzzy_term_counters(index, request):
    """40 FUZZY term queries (typos, unknown grams, theta clamped to 1, NOT terms, a filter row, a typed condition, docid
    and score pages, with and without verify_text — there after_filters is the count BEFORE the edit-distance filter and
    total the count after it): counters equal the oracle's for every query the oracle does not end with
    empty_term_detected (at most 4 of the 40, which must report empty_term_detected themselves)."""
    t = request.getfixturevalue(index)
    specs, qs, want = t.family("fuzzy")
    got = t.p.dev.search_batch(qs)
    assert FU.compare(specs, got, want) >= len(specs) - 4
    cut = [(g.after_filters, g.total) for s, g in zip(specs, got) if s.verify_text and not g.empty_term_detected]
    assert cut and all(af >= total for af, total in cut)


# (query, (total_candidates, after_intersection, after_not, after_filters), ascending doc ids) on FU.SMALL_DOCS with the
# filter row {1, 2, 3, 4} and a typed column 5, 20, 5, 20, 5, 20, NULL — worked out by hand, document by document
_ROW, _COL = "row", "col"
SMALL = [
    (dict(expr=("or", "basics", "cats"), not_terms=["machine"], filters=[(_ROW, False)]), (5, 5, 3, 1), [3]),
    (dict(expr=("and", "learning", ("not", "deep"))), (2, 2, 2, 2), [1, 4]),
    (dict(expr=("not", "learning"), universe=(2, 5)), (3, 3, 3, 3), [3, 5, 6]),
    (dict(expr=("not", "learning"), filters=[(_ROW, True)]), (4, 4, 4, 3), [5, 6, 7]),
    (dict(expr=("or", "goleng", "cats"), fuzzy=1), (3, 3, 3, 3), [3, 5, 7]),
    (dict(expr=("and", ("or", "basics", "cats"), ("not", "golang")), conditions=[(_COL, "<", 10)]), (4, 4, 4, 3), [1, 3, 5]),
    (dict(expr=("or", "zebra", ("and", "learning", "learning")), not_terms=["techniques"]), (3, 3, 2, 2), [1, 4]),
    (dict(terms=["goleng"], fuzzy=1), (1, 1, 1, 1), [7]),
    (dict(terms=["learnimg", "machine"], fuzzy=1, not_terms=["cats"]), (3, 1, 1, 1), [1]),
    (dict(terms=["lea"], fuzzy=1, filters=[(_ROW, False)]), (4, 4, 4, 4), [1, 2, 3, 4]),
    (dict(terms=["learnimg"], fuzzy=1, verify_text=True), (3, 3, 3, 3), [1, 2, 4]),
    (dict(terms=["basixs"], fuzzy=1, verify_text=True), (3, 3, 3, 3), [1, 6, 7]),
]


def test_seven_document_table_known_answers():
    """The reference's pipeline fixture (tests/server/search_pipeline_test.cpp:916-951) plus four rows: counters and ids
    written out by hand, equal on the device AND in the oracle, as docid pages and as SORT _score."""
    p = Pair(docs=FU.SMALL_DOCS, ngram=2, kanji=0)
    row = p.add_filter([1, 2, 3, 4])
    col = p.add_column([5, 20, 5, 20, 5, 20, 5], [False] * 6 + [True])
    qs = []
    for kw, _, _ in SMALL:
        kw = dict(kw)
        kw["filters"] = [(row, neg) for _, neg in kw.get("filters", [])]
        kw["conditions"] = [(col, FU.OPS.index(op), lit, 0.0, False, False, False) for _, op, lit in kw.get("conditions", [])]
        qs.append(Query(limit=0, descending=False, **kw))
        qs.append(Query(sort_score=True, limit=10, **kw))
    got = p.check(qs)  # page, total, scores and counters against the oracle
    for i, (kw, counters, ids) in enumerate(SMALL):
        for g in got[2 * i: 2 * i + 2]:
            assert tuple(int(getattr(g, k)) for k in FU.COUNTERS) == counters, kw
            assert g.total == len(ids) and sorted(g.docs.tolist()) == ids, kw
