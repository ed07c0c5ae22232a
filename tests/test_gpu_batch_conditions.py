"""-m gpu: FILTER conditions a batch brings along (mgx_query.conditions, Query(conditions=[...])) — evaluated by the
batch's first launch into rows the batch object owns — against the same conditions registered as filter rows
(DeviceIndex.filter_compare), against the comparison written out here in numpy, and, wherever the reference's
per-document path says what a condition means, against oracle/filters.py::doc_matches applied to the oracle's result of
the unfiltered query. Everything is integer set algebra and the already-pinned fp64 scores: no tolerance anywhere."""
import re

import numpy as np
import pytest

from gpu_util import Pair
from oracle import filters as F
from pkg import mg

pytestmark = pytest.mark.gpu
Query = mg.engine.Query
OPS = ("=", "!=", "<", "<=", ">", ">=")
SWITCHES = ("MGX_FORCE_BLOCK_KERNEL", "MGX_FAST_PATH", "MGX_CAND", "MGX_MERGE")
_LINE = re.compile(r"\[mgx\] (score|docid-page|bitmap) group: \d+ queries; fast path (\d+) items .*?wave kernel (\d+) items "
                   r".*?block kernel (\d+) items .*?candidate-driven (\d+) queries")
OUT_OF_RANGE, INVALID_ARGUMENT = 3, 2  # MGX_ERR_*


class Table:
    """An index, the oracle's copy of it, and one typed column per value class with NULLs (the last document among them)."""

    def __init__(self, n_docs, first_doc_id, seed, dense_threshold=0.0):
        self.p = Pair(corpus=mg.Corpus.synthetic(n_docs, seed=seed), first_doc_id=first_doc_id,
                      dense_threshold=dense_threshold)
        self.n, self.first = n_docs, first_doc_id
        rng = np.random.default_rng(seed + 1)
        di = self.p.dev.device_index
        self.cols = {}
        values = {
            "signed": rng.integers(-40, 40, n_docs).astype(np.int64),
            # (both halves of the unsigned range: a signed comparison would order them the other way round)
            "unsigned": (rng.integers(0, 64, n_docs).astype(np.uint64) << np.uint64(58)) + np.uint64(3),
            "double": rng.integers(-160, 160, n_docs) / 4.0,
        }
        for name, v in values.items():
            nul = rng.random(n_docs) < 0.1
            nul[-1] = True
            nul[0] = False
            self.cols[name] = (di.add_filter_column(v, nul), v, nul)
        c = self.p.dev.columns
        sizes = np.diff(c.offsets.astype(np.int64))
        order = [g for g in np.argsort(-sizes, kind="stable") if b" " not in c.gram(g)]
        self.dense = [c.gram(g).decode() for g in order[:12]]
        self.sparse = [c.gram(g).decode() for g in order if 4 < sizes[g] <= 100][:8]  # sorted-list operands
        self._base = {}

    # ---- what a condition means -------------------------------------------------------------------------------------
    def literal(self, name, k=0):
        return {"signed": [-7, 0, 39, -41], "unsigned": [(41 << 58) + 3, 3, (63 << 58) + 3, 5],
                "double": [12.25, -3.5 + 5e-10, 0.0, 100.0]}[name][k]

    def mask(self, name, op, lit, eps=0.0, null_matches=False, never_matches=False):
        """The doc set of mgx_index_filter_compare, by slot."""
        _, v, nul = self.cols[name]
        if name == "double":
            a, b = v, np.float64(lit)
            if op in ("=", "!=") and eps > 0:
                m = np.abs(a - b) < eps if op == "=" else np.abs(a - b) >= eps
            elif op in ("=", "!="):
                same = a.view(np.uint64) == b.view(np.uint64)
                m = same if op == "=" else ~same
            else:
                m = {"<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op]
        else:
            b = np.int64(lit) if name == "signed" else np.uint64(lit)
            m = {"=": v == b, "!=": v != b, "<": v < b, "<=": v <= b, ">": v > b, ">=": v >= b}[op]
        if never_matches:
            m = np.zeros(self.n, bool)
        return np.where(nul, bool(null_matches), m)

    def cond(self, name, op, lit, eps=0.0, null_matches=False, never_matches=False, negate=False):
        return (self.cols[name][0], OPS.index(op), lit, eps, null_matches, never_matches, negate)

    def row(self, name, op, lit, eps=0.0, null_matches=False, never_matches=False, negate=False):
        """The same condition as a registered filter row: a `filters` entry."""
        bid = self.p.dev.device_index.filter_compare(self.cols[name][0], OPS.index(op), lit, eps, null_matches, never_matches)
        return (bid, negate)

    def oracle_says(self, docs, name, op, lit, eps, null_matches, never_matches):
        """doc_matches for every document of `docs` where the reference's per-document path defines the condition (NULL
        passes != only, doubles compare = / != within kFilterValueEpsilon, an unparsable literal matches no stored value),
        else None."""
        if null_matches != (op == "!=") or (name == "double" and op in ("=", "!=") and eps != F.EPSILON):
            return None
        _, v, nul = self.cols[name]
        vtype = {"signed": "int64", "unsigned": "uint64", "double": "double"}[name]
        value = "x" if never_matches else repr(lit)
        parsed = F.parse_filter_value(value)
        return np.asarray([F.doc_matches(None if nul[i] else (vtype, v[i].item()), op, value, parsed)
                           for i in (docs - self.first).tolist()], bool)

    # ---- expected results -------------------------------------------------------------------------------------------
    def base(self, terms, not_terms=()):
        """The oracle's result of the unfiltered query (computed once per term list) and its funnel."""
        key = (tuple(terms), tuple(not_terms))
        if key not in self._base:
            total, docs, _, r = self.p.oracle_query(Query(list(terms), list(not_terms), limit=0, descending=False))
            self._base[key] = (np.asarray(docs, np.int64), r)
        return self._base[key]

    def expect(self, terms, masks, not_terms=()):
        """masks: [(member-by-slot, negate)] -> ascending docids of the filtered result."""
        docs, r = self.base(terms, not_terms)
        keep = np.ones(len(docs), bool)
        for m, negate in masks:
            keep &= ~m[docs - self.first] if negate else m[docs - self.first]
        return docs[keep], r


def _same(a, b, ctx):
    assert a.total == b.total, ctx
    assert a.docs.tolist() == b.docs.tolist(), ctx
    assert np.array_equal(a.scores, b.scores), ctx
    for k in ("total_candidates", "after_intersection", "after_not", "after_filters"):
        assert getattr(a, k) == getattr(b, k), (ctx, k)


def _check_page(t, q, got, want, r, ctx):
    """`got` against the expected filtered docids `want` (ascending) of query q."""
    assert got.total == len(want), ctx
    assert got.after_filters == len(want), ctx
    if not r["empty_term_detected"]:
        for k in ("total_candidates", "after_intersection", "after_not"):
            assert getattr(got, k) == r[k], (ctx, k)
    if q.sort_score:
        assert set(got.docs.tolist()) <= set(want.tolist()) and len(got.docs) == min(q.limit, len(want)), ctx
    else:
        page = want[::-1] if q.descending else want
        assert got.docs.tolist() == (page[: q.limit] if q.limit else page).tolist(), ctx


@pytest.fixture(scope="module")
def big():
    return Table(2 * 16384 + 77, 7, seed=51)  # three tiles, a partial last one, a last word that is not full


@pytest.fixture(scope="module")
def small():
    return Table(63, 1, seed=53)  # less than one word


def _routes(dev, qs, monkeypatch, capfd, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MGX_VERBOSE", "1")
    capfd.readouterr()
    got = dev.search_batch(qs)
    err = capfd.readouterr().err
    for k in SWITCHES + ("MGX_VERBOSE",):
        monkeypatch.delenv(k, raising=False)
    n = {"fast": 0, "wave": 0, "block": 0, "cand": 0}
    for m in _LINE.finditer(err):
        for k, x in zip(("fast", "wave", "block", "cand"), m.groups()[1:]):
            n[k] += int(x)
    return got, n


# ---- equivalence and oracle parity -------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["big", "small"])
@pytest.mark.parametrize("name", ["signed", "unsigned", "double"])
def test_a_condition_equals_its_filter_row_and_the_oracle(name, shape, request):
    """Every operator x null_matches x never_matches x negate (doubles: epsilon 1e-9 and 0) as conditions=[c] and as
    filters=[(filter_compare(c), negate)] in one batch, SORT _score: docids, total, the four funnel counters and the fp64
    scores are identical; total and the docid page equal the comparison written out in numpy; where doc_matches defines the
    condition, that comparison equals doc_matches on every document."""
    t = request.getfixturevalue(shape)
    terms = t.dense[:3] if shape == "big" else t.dense[:1]
    combos = []
    for op in OPS:
        for eps in ((1e-9, 0.0) if name == "double" else (0.0,)):
            for nm in (False, True):
                for never in (False, True):
                    for negate in (False, True):
                        combos.append((op, t.literal(name, len(combos) % 2), eps, nm, never, negate))
    qs = []
    for op, lit, eps, nm, never, negate in combos:
        qs.append(Query(terms, conditions=[t.cond(name, op, lit, eps, nm, never, negate)], sort_score=True, limit=10))
        qs.append(Query(terms, filters=[t.row(name, op, lit, eps, nm, never, negate)], sort_score=True, limit=10))
        qs.append(Query(terms, conditions=[t.cond(name, op, lit, eps, nm, never, negate)], limit=0, descending=False))
    got = t.p.dev.search_batch(qs)
    nonempty = 0
    for i, (op, lit, eps, nm, never, negate) in enumerate(combos):
        ctx = (name, shape) + combos[i]
        _same(got[3 * i], got[3 * i + 1], ctx)
        m = t.mask(name, op, lit, eps, nm, never)
        base = t.base(terms)[0]
        says = t.oracle_says(base, name, op, lit, eps, nm, never)
        if says is not None:  # doc_matches on the oracle's result of the unfiltered query
            assert np.array_equal(m[base - t.first], says), ctx
        want, r = t.expect(terms, [(m, negate)])
        _check_page(t, qs[3 * i], got[3 * i], want, r, ctx)
        _check_page(t, qs[3 * i + 2], got[3 * i + 2], want, r, ctx)  # (NE / null_matches: a set tail bit would show in total)
        nonempty += len(want) > 0
    assert nonempty > len(combos) // 4


# ---- every reader of a filter operand ----------------------------------------------------------------------------------

def _reader_queries(t, terms, **kw):
    """A few conditions of every class, as a condition and as its filter row, around one query shape."""
    picks = [("signed", ">=", 0, 0.0, False, False, False), ("signed", "!=", 0, 0.0, True, False, False),
             ("unsigned", "<", 1, 0.0, False, False, True), ("double", "=", 1, 1e-9, False, False, False),
             ("double", "<=", 0, 0.0, True, False, False), ("unsigned", "=", 0, 0.0, False, True, True)]
    qs, masks = [], []
    for name, op, k, eps, nm, never, negate in picks:
        lit = t.literal(name, k)
        qs.append(Query(terms, conditions=[t.cond(name, op, lit, eps, nm, never, negate)], **kw))
        qs.append(Query(terms, filters=[t.row(name, op, lit, eps, nm, never, negate)], **kw))
        masks.append([(t.mask(name, op, lit, eps, nm, never), negate)])
    return qs, masks


def _check_readers(t, qs, masks, got, not_terms=()):
    for i, m in enumerate(masks):
        _same(got[2 * i], got[2 * i + 1], i)
        want, r = t.expect(qs[2 * i].terms, m, not_terms)
        _check_page(t, qs[2 * i], got[2 * i], want, r, i)


@pytest.mark.parametrize("n_terms", [1, 3, 5])
def test_fast_scored_path(big, n_terms, monkeypatch, capfd):
    qs, masks = _reader_queries(big, big.dense[:n_terms], sort_score=True, limit=10)
    got, n = _routes(big.p.dev, qs, monkeypatch, capfd, {})
    assert n["fast"] > 0, n
    _check_readers(big, qs, masks, got)


@pytest.mark.parametrize("sort_score", [False, True])
def test_general_kernel_expression_not_terms_and_forced_block(big, sort_score, monkeypatch, capfd):
    kw = {"sort_score": True, "limit": 10} if sort_score else {"limit": 10, "descending": False}
    a, b, c = big.dense[:3]
    # NOT terms (the wave / fast kernels take them too) and MGX_FORCE_BLOCK_KERNEL: every query on the general kernel
    qs, masks = _reader_queries(big, [a, b], **kw)
    for q in qs:
        q.not_terms = [c]
    for env in ({}, {"MGX_FORCE_BLOCK_KERNEL": "1"}):
        got, n = _routes(big.p.dev, qs, monkeypatch, capfd, env)
        if env:
            assert n["block"] > 0 and n["fast"] == n["wave"] == n["cand"] == 0, n
        _check_readers(big, qs, masks, got, not_terms=[c])
    # an expression query runs on the general kernel: (a AND b) OR c, conditions against their filter rows and numpy
    eqs, emasks = _reader_queries(big, [a, b, c], **kw)
    for q in eqs:
        q.expr = ("or", ("and", a, b), c)
    got, n = _routes(big.p.dev, eqs, monkeypatch, capfd, {})
    assert n["block"] > 0, n
    base = big.p.oracle_query(Query(expr=eqs[0].expr, limit=0, descending=False))[1].astype(np.int64)
    for i, m in enumerate(emasks):
        _same(got[2 * i], got[2 * i + 1], i)
        keep = m[0][0][base - big.first]
        want = base[~keep if m[0][1] else keep]
        assert got[2 * i].total == len(want), i
        if not sort_score:
            assert got[2 * i].docs.tolist() == want[:10].tolist(), i


@pytest.mark.parametrize("cand", ["1", "0"])
def test_candidate_driven_kernel_on_and_off(big, cand, monkeypatch, capfd):
    assert len(big.sparse) >= 2
    for kw in ({"sort_score": True, "limit": 10}, {"limit": 10, "descending": True}):
        qs, masks = _reader_queries(big, [big.sparse[0], big.dense[0]], **kw)
        got, n = _routes(big.p.dev, qs, monkeypatch, capfd, {"MGX_CAND": cand})
        assert (n["cand"] > 0) == (cand == "1"), n
        _check_readers(big, qs, masks, got)


@pytest.mark.parametrize("kw", [{"limit": 10, "descending": False}, {"limit": 0, "descending": False},
                                {"limit": 10, "descending": True}, {"limit": 0, "descending": True}])
def test_docid_pages(big, small, kw):
    for t in (big, small):
        qs, masks = _reader_queries(t, t.dense[:2], **kw)
        _check_readers(t, qs, masks, t.p.dev.search_batch(qs))


def test_lists_only_index():
    t = Table(16384 + 300, 3, seed=57, dense_threshold=2.0)  # no gram has a bitmap row: every operand a sorted list
    for kw in ({"sort_score": True, "limit": 10}, {"limit": 20, "descending": False}, {"limit": 0, "descending": True}):
        qs, masks = _reader_queries(t, t.dense[:2], **kw)
        _check_readers(t, qs, masks, t.p.dev.search_batch(qs))


def test_facet_counts_with_a_condition(big):
    t = big
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 9, t.n).astype(np.uint32)
    ids[::11] = 0xFFFFFFFF
    col = t.p.dev.device_index.add_filter_column(ids.astype(np.int64), value_ids=ids, n_values=9)
    for name, op, k, negate in (("signed", ">=", 0, False), ("double", "!=", 0, True), ("unsigned", "<=", 0, False)):
        lit = t.literal(name, k)
        nm = op == "!="
        q = Query(t.dense[:2], conditions=[t.cond(name, op, lit, 0.0, nm, False, negate)])
        matched, counts = t.p.dev.facet_counts(q, col, 9)
        want, _ = t.expect(t.dense[:2], [(t.mask(name, op, lit, 0.0, nm), negate)])
        v = ids[want - t.first]
        assert matched == len(want)
        assert counts.tolist() == np.bincount(v[v != 0xFFFFFFFF], minlength=9).tolist()
        q2 = Query(t.dense[:2], filters=[t.row(name, op, lit, 0.0, nm, False, negate)])
        matched2, counts2 = t.p.dev.facet_counts(q2, col, 9)
        assert matched2 == matched and counts2.tolist() == counts.tolist()


# ---- batch structure ---------------------------------------------------------------------------------------------------

def _literals(t, n, start):
    """n distinct (op, literal) pairs on the signed column (values -40..39)."""
    return [(OPS[2 + (start + i) % 4], (start + i) % 97 - 48) for i in range(n)]


def _check_many(t, terms, conds_per_query, got, kw):
    for conds, g in zip(conds_per_query, got):
        masks = [(t.mask(name, op, lit, eps, nm, never), negate) for name, op, lit, eps, nm, never, negate in conds]
        want, r = t.expect(terms, masks)
        _check_page(t, Query(terms, **kw), g, want, r, conds)


def _queries(t, terms, conds_per_query, **kw):
    return [Query(terms, conditions=[t.cond(*c) for c in conds], **kw) for conds in conds_per_query]


def test_many_conditions_columns_and_sharing(big):
    t = big
    terms, kw = t.dense[:2], {"limit": 10, "descending": False}
    # 200 distinct conditions on one column in one batch
    per = [[("signed", op, lit, 0.0, False, False, False)] for op, lit in _literals(t, 200, 0)]
    assert len({c[0][1:3] for c in per}) == 200
    _check_many(t, terms, per, t.p.dev.search_batch(_queries(t, terms, per, **kw)), kw)
    # three columns of different classes in one batch, two and three conditions in one query
    per = [[("signed", ">", -7, 0.0, False, False, False), ("double", "<=", 12.25, 0.0, False, False, False)],
           [("unsigned", ">=", t.literal("unsigned", 0), 0.0, True, False, False)],
           [("double", "=", t.literal("double", 1), 1e-9, False, False, True), ("signed", "!=", 0, 0.0, True, False, False),
            ("unsigned", "<", t.literal("unsigned", 2), 0.0, False, False, False)]]
    _check_many(t, terms, per, t.p.dev.search_batch(_queries(t, terms, per, **kw)), kw)
    # one condition shared by 500 queries (in both polarities: `negate` does not make a condition distinct)
    per = [[("signed", ">=", 3, 0.0, False, False, bool(i % 2))] for i in range(500)]
    _check_many(t, terms, per, t.p.dev.search_batch(_queries(t, terms, per, sort_score=True, limit=5)),
                {"sort_score": True, "limit": 5})
    # filters and conditions in one query
    f1 = t.row("double", ">", 0.0)
    f2 = t.row("signed", "=", -7, negate=True)
    qs = [Query(terms, filters=[f1], conditions=[t.cond("signed", "<", 20)], **kw),
          Query(terms, filters=[f1, f2], conditions=[t.cond("unsigned", ">", 3, negate=True), t.cond("signed", "<", 20)], **kw)]
    got = t.p.dev.search_batch(qs)
    md, ms7, ms20, mu = t.mask("double", ">", 0.0), t.mask("signed", "=", -7), t.mask("signed", "<", 20), t.mask("unsigned", ">", 3)
    for g, masks in zip(got, ([(md, False), (ms20, False)], [(md, False), (ms7, True), (mu, True), (ms20, False)])):
        want, r = t.expect(terms, masks)
        _check_page(t, qs[0], g, want, r, len(masks))


def test_refusals(big):
    t = big
    terms = t.dense[:1]
    col = t.cols["signed"][0]

    def code(q):
        with pytest.raises(mg._capi.MgxError) as e:
            t.p.dev.search_batch([q])
        return e.value.code
    f = t.row("signed", ">", 0)
    assert code(Query(terms, filters=[f] * 33, conditions=[t.cond("signed", ">", 1)] * 32)) == OUT_OF_RANGE
    t.p.dev.search_batch([Query(terms, filters=[f] * 32, conditions=[t.cond("signed", ">", 1)] * 32)])  # 64: accepted
    assert code(Query(terms, conditions=[(10_000, 0, 1)])) == OUT_OF_RANGE
    assert code(Query(terms, conditions=[(col, 6, 1)])) == INVALID_ARGUMENT


# ---- reset and bounded memory ------------------------------------------------------------------------------------------

def test_reset_between_condition_counts(big):
    """One PreparedBatch from 200 conditions to 3 different ones, to none, to 300: rows of an earlier batch never show."""
    t = big
    terms, kw = t.dense[:2], {"limit": 10, "descending": False}
    batch = None
    for per in ([[("signed", op, lit, 0.0, False, False, False)] for op, lit in _literals(t, 200, 0)],
                [[("double", "<", 1.5, 0.0, True, False, False)], [("unsigned", "!=", 3, 0.0, True, False, False)],
                 [("signed", "=", 11, 0.0, False, False, True)]],
                [[]] * 4,
                [[("signed", op, lit, 0.0, bool(i % 2), False, False)] for i, (op, lit) in enumerate(_literals(t, 300, 150))]):
        batch = t.p.dev.prepare(_queries(t, terms, per, **kw), into=batch)
        batch.execute()
        _check_many(t, terms, per, batch.fetch(), kw)
        batch.execute()  # (a second execute of the same batch evaluates its conditions again)
        _check_many(t, terms, per, batch.fetch(), kw)


def test_fresh_literals_do_not_grow_the_index(big):
    t = big
    terms, kw = t.dense[:2], {"sort_score": True, "limit": 10}
    di = t.p.dev.device_index
    before = di.memory_bytes()
    batch = None
    for step in range(40):
        per = [[("double", OPS[2 + i % 4], (step * 32 + i) / 8.0 - 80.0, 0.0, False, False, False)] for i in range(32)]
        batch = t.p.dev.prepare(_queries(t, terms, per, **kw), into=batch)
        batch.execute()
        _check_many(t, terms, per, batch.fetch(), kw)
    assert di.memory_bytes() == before
