"""-m gpu: the tile program (tile_eval_kernel and the host that compiles for it) at every capacity limit it declares, and
one past each: 127 grams per threshold term (the 7-bit bit-sliced counters and their bitwise compare), 40 stack levels
(the LDS operand stack, tile_may_match's bit stack, tile_jump_setup's scratch), 512 expression tokens, 192 distinct
operands, 64 LDS-resident operands, 64 scored terms and the 160 KiB LDS plan, and the operand counts at which a flat
scored query changes kernels. The device answers against the oracle through Pair / OracleSide; everything compared is an
integer or an fp64 score bit for bit: no tolerance. A shape one past a limit is given to Index.prepare alone — a missing
refusal is then a failed assertion, never a launch of a shape the kernel cannot hold — and after every refusal a plain
query on the same index must still equal the oracle.

The corpora and queries come from limits_util.py; test_limits_cpu.py asserts their coverage conditions without a device."""
import re

import numpy as np
import pytest

import funnel_util as FU
import limits_util as LU
from gpu_util import OPS, Pair
from pkg import mg
from test_gpu_batch_conditions import _LINE, SWITCHES, _routes

pytestmark = pytest.mark.gpu
Query = mg.engine.Query
MgxError = mg._capi.MgxError
OUT_OF_RANGE, NOT_IMPLEMENTED = LU.OUT_OF_RANGE, LU.NOT_IMPLEMENTED
LDS_MAX = 160 * 1024
FZ_LDS = 256 * 8 + 16 + 2048 * 2  # kFzLdsBytes: what the fuzzy text filter takes beyond the plan
_GROUP_LDS = re.compile(r"\[mgx\] (\S+) group: .*?block kernel \d+ items \(lds (\d+) B\)")
_MERGE = re.compile(r"list merge (\d+) items")


# ---- indexes: each built once ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def thr_bitmap():
    texts, held = LU.threshold_corpus_bitmap()
    return Pair(corpus=mg.Corpus.from_texts(texts))


@pytest.fixture(scope="module")
def thr_lists():
    texts, held = LU.threshold_corpus_lists()
    return Pair(corpus=mg.Corpus.from_texts(texts), dense_threshold=2.0)


@pytest.fixture(scope="module")
def long_words():
    return Pair(corpus=mg.Corpus.from_texts(LU.long_word_corpus()))


@pytest.fixture(scope="module")
def bitmap():
    return Pair(corpus=mg.Corpus.synthetic(LU.BITMAP_DOCS, seed=61), dense_threshold=0.0)


@pytest.fixture(scope="module")
def lists():
    return Pair(corpus=mg.Corpus.synthetic(LU.LISTS_DOCS, seed=62), dense_threshold=2.0)


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _prepare(dev, qs, monkeypatch, capfd, env=None):
    """Index.prepare alone under MGX_VERBOSE -> (batch, items per route — 'merge' included —, {group: block-kernel LDS
    bytes}). Nothing is launched; a refusal raises MgxError."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MGX_VERBOSE", "1")
    capfd.readouterr()
    try:
        batch = dev.prepare(qs)
    finally:
        err = capfd.readouterr().err
        for k in SWITCHES + ("MGX_VERBOSE",):
            monkeypatch.delenv(k, raising=False)
    n = {"fast": 0, "wave": 0, "block": 0, "cand": 0}
    for m in _LINE.finditer(err):
        for k, x in zip(("fast", "wave", "block", "cand"), m.groups()[1:]):
            n[k] += int(x)
    n["merge"] = sum(int(x) for x in _MERGE.findall(err))
    return batch, n, {g: int(b) for g, b in _GROUP_LDS.findall(err)}


def _compare(p, qs, got):
    """What Pair.check asserts, for results that are already here."""
    for q, g in zip(qs, got):
        total, page, scores, r = p.oracle_query(q)
        ctx = (q.terms[:8], len(q.terms), q.not_terms[:8], len(q.filters), q.limit, q.offset, q.sort_score, q.fuzzy)
        assert g.total == total, (ctx, g.total, total)
        assert g.docs.tolist() == page.tolist(), ctx
        if scores is not None:
            assert np.array_equal(g.scores, scores), (ctx, g.scores, scores)
        assert g.empty_term_detected == r["empty_term_detected"], ctx
        if not r["empty_term_detected"]:
            for k in FU.COUNTERS:
                assert getattr(g, k) == r[k], (ctx, k, getattr(g, k), r[k])


def _run(batch):
    batch.execute()
    return batch.fetch()


def _plain(p):
    """A plain two-term AND out of the index's own two largest grams."""
    c = p.columns
    sizes = np.diff(c.offsets.astype(np.int64))
    top = [c.gram(int(g)).decode() for g in np.argsort(-sizes, kind="stable") if b" " not in c.gram(int(g))][:2]
    return Query(top, limit=17)


def _refused(p, qs, code, needle=""):
    """Index.prepare refuses `qs` with `code` (nothing was launched), and nothing sticks: a plain query still equals the
    oracle. -> the message."""
    with pytest.raises(MgxError) as e:
        p.dev.prepare(qs)
    assert e.value.code == code and needle in str(e.value), e.value
    got = p.check([_plain(p)])
    assert got[0].total > 0
    return str(e.value)


def _largest(p, make, hi, monkeypatch, capfd):
    """The largest k <= hi whose make(k) Index.prepare accepts, going down; every larger one is refused with
    MGX_ERR_NOT_IMPLEMENTED on the host. -> (k, its batch, {group: LDS bytes}, message of the refusal of k + 1)."""
    message = None
    for k in range(hi, 0, -1):
        try:
            batch, _, lds = _prepare(p.dev, [make(k)], monkeypatch, capfd)
        except MgxError as e:
            assert e.code == NOT_IMPLEMENTED, e
            message = str(e)
            continue
        assert message is not None, "make(%d) was accepted: start higher" % hi
        return k, batch, lds, message
    raise AssertionError("no shape accepted")


def _diff(got, want):
    g, w = set(got.tolist()), set(want.tolist())
    return {"missing": sorted(w - g)[:8], "n_missing": len(w - g), "extra": sorted(g - w)[:8], "n_extra": len(g - w)}


# ---- A. threshold counters -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", LU.THRESHOLD_T)
def test_threshold_counters_three_tiles(thr_bitmap, T):
    """mgx_threshold over the first T grams against Index::SearchByThreshold of the oracle at theta = 1, 2, every 2^k - 1,
    2^k, 2^k + 1 below T, T - 1 and T: counts that carry into every bit of the 7-bit counters, thresholds with every bit
    set, documents with theta - 1, theta and theta + 1 grams in one 64-document word, bitmap-form and sorted-list grams
    together (T >= 126), three tiles with a partial last word whose top bit is a match."""
    p = thr_bitmap
    for th in LU.thetas(T):
        want = p.oidx.search_by_threshold(LU.GRAMS[:T], th)
        got = p.dev.search_by_threshold(LU.GRAMS[:T], th)
        assert 0 < len(want) < p.columns.n_docs
        assert np.array_equal(got, want), (T, th, _diff(got, want))


def test_threshold_counters_lists_only(thr_lists):
    """The same on the lists-only index up to T = 64 — every operand a sorted list scattered into LDS, 64 of them the most
    the plan holds; the grams live in the second tile alone, so the union-bound jump skips the first — and the mixed
    queries, in whose first tile exactly theta (or T - 1) of the T lists have a posting: tile_may_match's `cnt >= arg` at
    equality, and a threshold term that requires none of its operands."""
    p = thr_lists
    n = 0
    for T in LU.THRESHOLD_T:
        if T > LU.LISTS_MAX_T:
            continue
        for th in LU.thetas(T):
            want = p.oidx.search_by_threshold(LU.GRAMS[:T], th)
            got = p.dev.search_by_threshold(LU.GRAMS[:T], th)
            assert len(want) > 0 and np.array_equal(got, want), (T, th, _diff(got, want))
            n += 1
    assert n >= 100
    for T, th, grams in LU.mixed_threshold_cases():
        want = p.oidx.search_by_threshold(grams, th)
        got = p.dev.search_by_threshold(grams, th)
        assert (want <= LU.TILE).any() and np.array_equal(got, want), ("mixed", T, th, _diff(got, want))


def test_threshold_of_65_lists_is_refused(thr_lists):
    """One past the 64 LDS-resident operands: refused on the host (MGX_ERR_NOT_IMPLEMENTED), as an expression given to
    Index.prepare first and only then as mgx_threshold."""
    p = thr_lists
    # (64 terms are the most a query takes: the 65th list is a NOT term's)
    _refused(p, [Query(expr=("or",) + tuple(LU.GRAMS[:64]), not_terms=[LU.GRAMS[64]], limit=17)], NOT_IMPLEMENTED,
             "more than 64 sorted-list")
    with pytest.raises(MgxError) as e:
        p.dev.search_by_threshold(LU.GRAMS[:65], 33)
    assert e.value.code == NOT_IMPLEMENTED, e.value
    p.check([_plain(p), Query(expr=("or",) + tuple(LU.GRAMS[:64]), limit=0, descending=False)])


def test_threshold_of_128_grams_is_refused(thr_bitmap):
    """One past the 127 grams the 7-bit counters hold: mgx_threshold refuses before it compiles anything."""
    p = thr_bitmap
    assert all(p.columns.lookup(g) is not None for g in LU.TOKENS[:128])
    with pytest.raises(MgxError) as e:
        p.dev.search_by_threshold(LU.TOKENS[:128], 33)
    assert e.value.code == OUT_OF_RANGE and "more than 127 grams" in str(e.value), e.value
    assert p.check([_plain(p)])[0].total > 0


def test_fuzzy_long_words(long_words):
    """FUZZY 1 and 2 over terms of 8 .. 127 grams (theta = grams - 2 d from the oracle; a typo whose grams the index does not
    know): the same threshold op in a materialised result, a docid page, SORT _score, a second term and an expression
    behind PUSH / POP. Pages, totals, the four funnel counters and the scores equal the oracle's."""
    p = long_words
    specs = LU.long_word_specs(p)
    want = FU.expected(p, specs, 0, 0)
    qs = [s.query(0, 0) for s in specs]
    assert FU.compare(specs, p.dev.search_batch(qs), want) == len(specs) == 108
    _, refused = LU.long_word_terms(p)
    for d in (1, 2):
        _refused(p, [Query([refused], fuzzy=d, limit=17)], OUT_OF_RANGE, "more than 127 grams")
    _refused(p, [Query(expr=("or", refused, "ab"), fuzzy=1, limit=17)], OUT_OF_RANGE, "more than 127 grams")


# ---- B. nesting depth and program length -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", LU.SHAPES)
@pytest.mark.parametrize("index", ["bitmap", "lists"])
def test_chains_at_every_stack_depth(index, shape, request, monkeypatch, capfd):
    """Right-nested AND / OR chains, NOT chains and chains that alternate AND and NOT at stack depth 4, 8, 31, 32, 33, 39
    and 40, each at the five page shapes of funnel_util.PAGES: page, total, scores and counters equal the oracle's. The
    depth is asserted from the shape and from the device's own plan (the general kernel's LDS grows by 2 KiB per level;
    a level's three instructions and
    a new operand's table rows add some tens of bytes). Depth 41 is refused."""
    p = request.getfixturevalue(index)
    core4 = None
    for d in LU.DEPTHS:
        tree = LU.chain(p, shape, d)
        assert LU.stack_depth(tree) == d
        # (on the lists-only build every distinct gram of an AND / OR chain is one more 2 KiB LDS bitmap: not a level)
        resident = len(Query(expr=tree).terms) if index == "lists" and shape != "not" else 0
        batch, n, lds = _prepare(p.dev, [Query(expr=tree, limit=0, descending=False)], monkeypatch, capfd)
        assert n["block"] > 0 and n["fast"] == n["wave"] == n["cand"] == n["merge"] == 0, n
        core = lds["bitmap"] - 2048 * resident
        core4 = core if d == 4 else core4
        assert (core - core4) // 2048 == d - 4, (d, lds, resident, core4)
        qs = LU.tree_queries(tree)
        _compare(p, qs[:1], _run(batch))
        got = p.check(qs)
        assert 0 < got[0].total < p.columns.n_docs
    _refused(p, [Query(expr=LU.chain(p, shape, 41), limit=17)], OUT_OF_RANGE, "deeper than 40")


def test_deep_chain_whose_first_operand_alone_is_in_a_tile(thr_lists):
    """("or", a, <AND chain>) at stack depth 31 .. 40 on the lists-only threshold corpus: `a` lives in the first tile, the
    chain's grams in the second. Whether the first tile is evaluated at all hangs on the BOTTOM entry of tile_may_match's
    bit stack, read back after up to 39 entries were pushed above it and popped again."""
    p = thr_lists
    for d in (31, 32, 33, 39, 40):
        tree = LU.halves_chain(d)
        assert LU.stack_depth(tree) == d
        got = p.check([Query(expr=tree, limit=0, descending=False), Query(expr=tree, limit=17),
                       Query(expr=tree, limit=17, descending=False), Query(expr=tree, sort_score=True, limit=10)])
        assert (got[0].docs <= LU.TILE).sum() > 50 and (got[0].docs > LU.TILE).sum() > 10, d


@pytest.mark.parametrize("index", ["bitmap", "lists"])
def test_programs_of_512_tokens(index, request):
    """An OR of 511 children over 64 distinct sparse grams (64 sorted lists: the most LDS holds) and an AND of 511
    children over three dense grams: 512 tokens, about 1500 instructions. 513 tokens are refused; so is SORT _score over
    the first page of 511 scored leaves (more than 64 scored terms) — its deep page scores at fetch time and runs."""
    p = request.getfixturevalue(index)
    wide_or, wide_and = LU.wide_trees(p)
    for tree in (wide_or, wide_and):
        assert LU.n_tokens(tree) == 512
        got = p.check([Query(expr=tree, **page) for page in FU.PAGES[:3] + FU.PAGES[4:]])
        assert 0 < got[0].total < p.columns.n_docs
    _refused(p, [Query(expr=wide_or + (wide_or[1],), limit=17)], OUT_OF_RANGE, "longer than 512 tokens")
    _refused(p, [Query(expr=wide_or, sort_score=True, limit=10)], NOT_IMPLEMENTED, "more than 64 scored terms")


@pytest.mark.parametrize("index", ["bitmap", "lists"])
def test_deep_wide_plain_and_fuzzy_in_one_batch(index, request):
    """A depth-40 tree, a 511-child OR, a plain two-term AND and a FUZZY query share one group, whose LDS plan is the
    maximum over them: each equals the oracle, in either order, as docid pages and as materialised results. The OR here
    names 24 distinct sorted lists: with the 64 of test_programs_of_512_tokens the group would ask for 64 LDS bitmaps AND
    40 stack rows, 208 KiB, and the batch is refused although each of its queries runs alone (the known limit of
    test_a_wide_and_a_deep_query_in_one_batch)."""
    p = request.getfixturevalue(index)
    v = FU.vocabulary(p)
    for page in (dict(limit=17), dict(limit=0, descending=False)):
        rest = [Query(v["dense"][:2], **page), Query([FU._typo(v["words"][3], np.random.default_rng(5))], fuzzy=1, **page)]
        qs = [Query(expr=LU.chain(p, "and-or", 40), **page), Query(expr=LU.wide_trees(p, distinct=24)[0], **page)] + rest
        got = p.check(qs)
        assert all(r.total > 0 for r in got), [r.total for r in got]
        p.check(qs[::-1])
        _refused(p, [qs[0], Query(expr=LU.wide_trees(p)[0], **page)] + rest, NOT_IMPLEMENTED, "exceeds the 160 KiB LDS")


# ---- C. operand counts and the LDS plan ------------------------------------------------------------------------------------
def _rows_and_column(p, n_rows=40):
    n = p.columns.n_docs
    slots = np.arange(n)
    rows = [p.add_filter((np.nonzero(slots % (i + 7) != 0)[0] + 1).astype(np.uint32)) for i in range(n_rows)]
    rng = np.random.default_rng(9)
    col = p.add_column(rng.integers(-40, 40, n), rng.random(n) < 0.05)
    return rows, col


def test_64_terms_64_not_terms_64_filters(thr_bitmap, monkeypatch):
    """64 positive terms, 64 NOT terms, and 64 filters and conditions together (query_parser.h:270-272), on the default
    routes and on the general kernel; 65 of each are refused."""
    p = thr_bitmap
    rows, col = _rows_and_column(p, 33)
    g = LU.GRAMS
    conds = [(col, OPS.index(">="), -39 + i, 0.0, False, False, False) for i in range(32)]
    page = dict(limit=0, descending=False)
    qs = [Query(g[:64], **page), Query(g[:64], sort_score=True, limit=1000, offset=100),
          Query(g[:1], g[63:127], **page), Query(g[:2], g[63:127], limit=17),
          Query(g[:1], filters=[(r, False) for r in rows[:32]], conditions=conds, **page),
          Query(g[:3], filters=[(r, i == 0) for i, r in enumerate(rows[:32])], conditions=conds, limit=17)]
    for env in ({}, {"MGX_FORCE_BLOCK_KERNEL": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = p.check(qs)
        assert all(r.total > 0 for r in got), [r.total for r in got]
    monkeypatch.delenv("MGX_FORCE_BLOCK_KERNEL")
    _refused(p, [Query(g[:65], **page)], OUT_OF_RANGE, "more than 64 terms")
    _refused(p, [Query(g[:1], g[62:127], **page)], OUT_OF_RANGE, "more than 64 terms")
    _refused(p, [Query(g[:1], filters=[(r, False) for r in rows[:33]], conditions=conds, **page)], OUT_OF_RANGE,
             "more than 64 filters and conditions")


def test_192_distinct_operands(thr_bitmap):
    """An expression whose program names exactly 192 distinct operands — the grams of 50 three-token terms, topped up with
    filter rows and conditions — on the bitmap build (its sorted-list grams among them); 193 are refused."""
    p = thr_bitmap
    rows, col = _rows_and_column(p, 40)
    terms = [" ".join(LU.TOKENS[3 * i:3 * i + 3]) for i in range(50)]
    grams = {g for t in terms for g in mg.engine.generate_query_ngrams(t, 2, 0, True)}
    assert all(p.columns.lookup(g) is not None for g in grams) and 150 < len(grams) < 190

    def query(n_operands, **page):
        extra = n_operands - len(grams)
        conds = [(col, OPS.index(">="), -39 + i, 0.0, False, False, False) for i in range(extra - min(extra, 40))]
        return Query(expr=("or",) + tuple(terms), filters=[(r, False) for r in rows[:min(extra, 40)]], conditions=conds,
                     **page)
    got = p.check([query(192, limit=0, descending=False), query(192, limit=17), query(191, sort_score=True, limit=40, offset=1000)])
    assert all(0 < r.total < p.columns.n_docs for r in got)
    _refused(p, [query(193, limit=17)], NOT_IMPLEMENTED, "more than 192 distinct operands")
    _refused(p, [query(193, sort_score=True, limit=40, offset=1000)], NOT_IMPLEMENTED, "more than 192 distinct operands")


def test_64_list_operands(thr_lists):
    """An expression over exactly 64 sorted lists on the lists-only build: every one resident in LDS. (65:
    test_threshold_of_65_lists_is_refused.)"""
    p = thr_lists
    tree = ("or",) + tuple(("and", LU.GRAMS[2 * i], LU.GRAMS[2 * i + 1]) for i in range(32))
    got = p.check([Query(expr=tree, limit=0, descending=False), Query(expr=tree, limit=17),
                   Query(expr=("and", ("or",) + tuple(LU.GRAMS[:32]), ("or",) + tuple(LU.GRAMS[32:64])), limit=17)])
    assert all(r.total > 0 for r in got)


@pytest.mark.parametrize("index", ["thr_bitmap", "thr_lists"])
def test_most_scored_terms_the_lds_plan_holds(index, request, monkeypatch, capfd):
    """The largest number of scored terms Index.prepare accepts (every scored operand is LDS-resident: 2 KiB and a
    512-byte prefix row each): its plan is within 8 KiB of the 160 KiB of a CU, one more is refused, and it scores bit for
    bit on the general kernel."""
    p = request.getfixturevalue(index)

    def make(k):
        return Query(LU.GRAMS[:k], sort_score=True, limit=10)
    k, batch, lds, message = _largest(p, make, 64, monkeypatch, capfd)
    print("most scored terms on %s: %d, plan %d B; %d: %s" % (index, k, lds["score"], k + 1, message))
    assert LDS_MAX - 8 * 1024 <= lds["score"] <= LDS_MAX and "160 KiB" in message, (k, lds, message)
    _refused(p, [make(k + 1)], NOT_IMPLEMENTED, "160 KiB")
    monkeypatch.setenv("MGX_FORCE_BLOCK_KERNEL", "1")
    got = p.check([make(k), Query(LU.GRAMS[:k], sort_score=True, limit=10, descending=False)])
    monkeypatch.delenv("MGX_FORCE_BLOCK_KERNEL")
    assert got[0].total > 0 and len(got[0].docs) == min(10, got[0].total)
    _compare(p, [make(k)], _run(batch))


def test_largest_fuzzy_verify_shape(thr_lists, monkeypatch, capfd):
    """A FUZZY term with verify_text (kOpVerifyFuzzy) over sorted lists, SORT _score with a page of 600 (a top-k of 1024
    per wave): the largest term Index.prepare accepts has a plan that, with the kFzLdsBytes of the filter, is within 8 KiB
    of 160 KiB; one more token is refused; the accepted shape equals the oracle."""
    p = thr_lists

    def make(k):
        return Query([" ".join(LU.GRAMS[:k])], fuzzy=1, verify_text=True, sort_score=True, limit=600)
    k, batch, lds, message = _largest(p, make, 30, monkeypatch, capfd)
    print("largest fuzzy-verify term: %d tokens, plan %d B + %d B; %d: %s" % (k, lds["score"], FZ_LDS, k + 1, message))
    assert LDS_MAX - 8 * 1024 <= lds["score"] + FZ_LDS <= LDS_MAX and "160 KiB" in message, (k, lds, message)
    _refused(p, [make(k + 1)], NOT_IMPLEMENTED, "160 KiB")
    got = _run(batch)
    _compare(p, [make(k)], got)
    assert 0 < got[0].total <= got[0].after_filters


def test_a_wide_and_a_deep_query_in_one_batch(bitmap, monkeypatch, capfd):
    """A group's LDS plan is the maximum over its queries in every dimension: the widest scored query and a depth-40 tree
    run alone, together their group asks for more than 160 KiB and the batch is refused (a known limit: the group is not
    split). The refusal is MGX_ERR_NOT_IMPLEMENTED on the host; both still run afterwards."""
    p = bitmap
    c = p.columns
    sizes = np.diff(c.offsets.astype(np.int64))
    dense = [c.gram(int(g)).decode() for g in np.argsort(-sizes, kind="stable") if b" " not in c.gram(int(g))][:64]

    def make(k):
        return Query(dense[:k], sort_score=True, limit=10)
    k, _, lds, _ = _largest(p, make, 64, monkeypatch, capfd)
    deep = Query(expr=LU.chain(p, "and-or", 40), sort_score=True, limit=10)
    _, _, lds_deep = _prepare(p.dev, [deep], monkeypatch, capfd)
    assert lds["score"] <= LDS_MAX and lds_deep["score"] <= LDS_MAX and lds_deep["score"] >= 40 * 2048
    message = _refused(p, [make(k), deep], NOT_IMPLEMENTED, "query shape exceeds the 160 KiB LDS of a CU")
    assert _refused(p, [deep, make(k)], NOT_IMPLEMENTED) == message
    p.check([make(k)])
    p.check([deep])
    p.check([make(12), deep])  # (a narrower query beside the deep one fits)


# ---- D. routing boundaries of the flat scoring kernels ---------------------------------------------------------------------
def _routed(p, q, monkeypatch, capfd, env=None):
    """Routes from Index.prepare alone, asserted by the caller BEFORE the batch runs; then the run against the oracle."""
    batch, n, _ = _prepare(p.dev, [q], monkeypatch, capfd, env)
    return batch, n


def test_scored_term_routing_boundaries(bitmap, monkeypatch, capfd):
    """Dense single-gram terms, SORT _score top 10: 3 scored terms on the wave kernel (kWaveScoreSlots; fast path off), 4
    and 5 on the fast path (kFastMaxScore), 6 on the general kernel; 5 scored terms with 8 operands on the fast path
    (kFastMaxOps), with 9 not. Every route is read from the plan before anything runs."""
    p = bitmap
    d = FU.vocabulary(p)["dense"]
    cases = [(Query(d[:3], sort_score=True, limit=10), {"MGX_FAST_PATH": "0"}, "wave"),
             (Query(d[:3], sort_score=True, limit=10), {}, "fast"),
             (Query(d[:4], sort_score=True, limit=10), {}, "fast"),
             (Query(d[:5], sort_score=True, limit=10), {}, "fast"),
             (Query(d[:6], sort_score=True, limit=10), {}, "block"),
             (Query(d[:5], d[10:13], sort_score=True, limit=10), {}, "fast"),
             (Query(d[:5], d[10:14], sort_score=True, limit=10), {}, "block")]
    for q, env, route in cases:
        batch, n = _routed(p, q, monkeypatch, capfd, env)
        others = [k for k in n if k != route]
        assert n[route] > 0 and all(n[k] == 0 for k in others), (len(q.terms), len(q.not_terms), env, route, n)
        got = _run(batch)
        _compare(p, [q], got)
        assert got[0].total > 0, (len(q.terms), len(q.not_terms))
    # the same through search_batch, with the route report of the condition tests
    got, n = _routes(p.dev, [c[0] for c in cases[2:]], monkeypatch, capfd, {})
    assert n["fast"] > 0 and n["block"] > 0 and n["wave"] == n["cand"] == 0, n
    _compare(p, [c[0] for c in cases[2:]], got)


def test_list_merge_routing_boundary(lists, monkeypatch, capfd):
    """Lists-only build, a long driver: 6 staged operands besides the driver run on the list-merge kernel (kMergeMaxOps),
    7 do not."""
    p = lists
    d = FU.vocabulary(p)["dense"]
    for q, merge in ((Query(d[:4], d[10:13], sort_score=True, limit=10), True),
                     (Query(d[:7], sort_score=True, limit=10), True),
                     (Query(d[:4], d[10:14], sort_score=True, limit=10), False),
                     (Query(d[:8], sort_score=True, limit=10), False)):
        batch, n = _routed(p, q, monkeypatch, capfd)
        assert (n["merge"] > 0) == merge and (merge or n["block"] > 0), (len(q.terms), len(q.not_terms), n)
        _compare(p, [q], _run(batch))
