"""-m gpu: every scoring path away from the default BM25 parameters. The reference accepts any k1 >= 0 and 0 <= b <= 1
(config-schema.json, config.cpp), and a sharded table scores with the table's total_docs / avg_doc_length rather than
the shard's own; the device bakes those values into K[dl] tables (bitmap_score_kernel), per-(gram, idf, k1, b, avgdl)
contribution tables (wave kernels), block-max bytes and the integer pruning bound (fast path). Every case here is held
against the oracle bit for bit (totals, pages, fp64 scores, funnel counters) under the default routing and with each
kernel path switched off in turn, and the [mgx] verbose line proves which kernels actually ran."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
from gpu_util import Pair, densify
from oracle import oracle as O
from pkg import mg
from test_gpu_scored_branches import _check_expr, _expected_scored

pytestmark = pytest.mark.gpu
Query = mg.engine.Query

K1 = [0.0, 1e-6, 0.3, 1.2, 2.0, 20.0, 1e4]
B = [0.0, 0.3, 0.75, 1.0]
# every k1 and every b at least once (1.2 only with a non-default b)
PARAMS = [(0.0, 0.75), (1e-6, 0.0), (0.3, 1.0), (1.2, 0.3), (2.0, 0.75), (20.0, 0.0), (1e4, 1.0)]
SWITCHES = ("MGX_FORCE_BLOCK_KERNEL", "MGX_FAST_PATH", "MGX_CAND", "MGX_MERGE")
ROUTES = {"default": {}, "block": {"MGX_FORCE_BLOCK_KERNEL": "1"}, "no-fast": {"MGX_FAST_PATH": "0"},
          "no-cand": {"MGX_CAND": "0"}, "no-merge": {"MGX_MERGE": "0"}}
_LINE = re.compile(r"\[mgx\] score group: \d+ queries; fast path (\d+) items \((\d+) queries, .*?wave kernel (\d+) items "
                   r"\(lds \d+ B, lists (\d+)\), block kernel (\d+) items .*?candidate-driven (\d+) queries, list merge (\d+) "
                   r"items")
KINDS = ("fast", "fast_queries", "wave", "wave_lists", "block", "cand", "merge")


# ---- helpers ---------------------------------------------------------------------------------------------------------

def _groups(params):
    """`params` cut into runs of at most 4 sets with k1 > 0: an index builds block-max bytes for 4 (k1, b, avgdl) sets
    (test_block_max_cap), so each run gets an index of its own and pruning runs for every set of the grid."""
    out, run, pruned = [], [], 0
    for k1, b in params:
        if k1 > 0 and pruned == 4:
            out.append(run)
            run, pruned = [], 0
        run.append((k1, b))
        pruned += k1 > 0
    return out + [run]


def _want(p, q):
    cache = p.__dict__.setdefault("want_cache", {})
    key = (tuple(q.terms), tuple(q.not_terms), q.limit, q.offset, q.descending, q.k1, q.b, p.N, p.avgdl)
    if key not in cache:
        cache[key] = p.oracle_query(q)
    return cache[key]


def _compare(p, qs, got):
    for q, g in zip(qs, got):
        total, page, scores, r = _want(p, q)
        ctx = (q.terms, q.not_terms, q.limit, q.offset, q.descending, q.k1, q.b, p.N, p.avgdl)
        assert g.total == total, ctx
        assert g.docs.tolist() == page.tolist(), (ctx, g.docs[:8], page[:8])
        assert np.array_equal(g.scores, scores), (ctx, g.scores[:8], scores[:8])
        if not r["empty_term_detected"]:
            for k in ("total_candidates", "after_intersection", "after_not", "after_filters"):
                assert getattr(g, k) == r[k], (ctx, k)


def _run(p, qs, route, monkeypatch, capfd):
    """One batch under `route`, checked against the oracle: (results, the items each kernel took by the verbose line).
    A route that switches a kernel off must not show it."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MGX_VERBOSE", "1")
    capfd.readouterr()
    got = p.dev.search_batch(qs)
    err = capfd.readouterr().err
    for k in SWITCHES + ("MGX_VERBOSE",):
        monkeypatch.delenv(k, raising=False)
    n = dict.fromkeys(KINDS, 0)
    for m in _LINE.finditer(err):
        fast, fast_queries, wave, lists, block, cand, merge = (int(x) for x in m.groups())
        n["fast"] += fast
        n["fast_queries"] += fast_queries
        n["wave"] += wave - lists
        n["wave_lists"] += lists
        n["block"] += block
        n["cand"] += cand
        n["merge"] += merge
    assert sum(n.values()) > 0, err[-2000:]
    if route == "block":
        assert n["block"] > 0 and n["block"] == sum(n[k] for k in KINDS if k != "fast_queries"), n
    elif route == "no-fast":
        assert n["fast"] == 0, n
    elif route == "no-cand":
        assert n["cand"] == 0, n
    elif route == "no-merge":
        assert n["merge"] == 0, n
    _compare(p, qs, got)
    return got, n


def _grams(p):
    c = p.dev.columns
    sizes = np.diff(c.offsets.astype(np.int64))
    g = sorted((i for i in range(c.n_grams) if b" " not in c.gram(i)), key=lambda i: -sizes[i])
    return c, sizes, g


def _dense_queries(p, k1, b, seed):
    c, sizes, g = _grams(p)
    grams = [c.gram(i).decode() for i in g[:48]]
    rng = np.random.default_rng(seed)
    qs = []
    for n_terms in (2, 3, 4, 5):
        for it in range(3):
            terms = [str(t) for t in rng.choice(grams[:16] if it else grams, size=n_terms, replace=False)]
            limit, offset = ((1, 0), (10, 3), (100, 0))[it]
            qs.append(Query(terms, sort_score=True, limit=limit, offset=offset, k1=k1, b=b))
    qs.append(Query(qs[1].terms, sort_score=True, limit=37, offset=5, descending=False, k1=k1, b=b))
    qs.append(Query(qs[4].terms, sort_score=True, limit=10, descending=False, k1=k1, b=b))
    return qs


@pytest.fixture(scope="module")
def corpus300k():
    # 19 tiles of dense grams (later tiles prune against a k-th best score) and sparse grams (candidate-driven queries);
    # each test builds its indexes over it, with the statistics and dense_threshold it needs
    return mg.Corpus.synthetic(300_000, seed=7)


# ---- the grid: dense scored terms on many tiles ----------------------------------------------------------------------

def test_dense_terms_every_parameter_every_route(corpus300k, monkeypatch, capfd):
    for group in _groups(PARAMS):
        p = Pair(corpus=corpus300k)
        for k1, b in group:
            qs = _dense_queries(p, k1, b, 100 + PARAMS.index((k1, b)))
            for route in ROUTES:
                _, n = _run(p, qs, route, monkeypatch, capfd)
                if route in ("default", "no-cand", "no-merge"):
                    # one (k1, b, avgdl) per batch: the fast path takes every query
                    assert n["fast_queries"] == len(qs), (k1, b, route, n)
                elif route == "no-fast":
                    assert n["wave"] > 0, (k1, b, n)


@pytest.mark.parametrize("stats", ["avgdl-below-1", "avgdl-x10", "avgdl-div10", "N-below-df", "N-zero"])
def test_dense_terms_under_other_statistics(corpus300k, stats, monkeypatch, capfd):
    own = Pair(corpus=corpus300k)
    c, sizes, g = _grams(own)
    own_n, own_avg = c.bm25_doc_count, c.avg_doc_length()
    N, avg = {"avgdl-below-1": (own_n, 0.4), "avgdl-x10": (own_n, own_avg * 10.0),
              "avgdl-div10": (own_n, own_avg / 10.0), "N-below-df": (int(sizes[g[20]]) // 2, own_avg),
              "N-zero": (0, own_avg)}[stats]
    del own
    p = Pair(corpus=corpus300k, total_docs=N, avg_doc_length=avg)
    j = ["avgdl-below-1", "avgdl-x10", "avgdl-div10", "N-below-df", "N-zero"].index(stats)
    for i in range(3):
        k1, b = PARAMS[(3 * j + i) % len(PARAMS)]
        qs = _dense_queries(p, k1, b, 200 + 3 * j + i)
        for route in ROUTES:
            got, n = _run(p, qs, route, monkeypatch, capfd)
            if route == "default":
                assert n["fast_queries"] == len(qs), (stats, k1, b, n)
            if N == 0:  # every idf is 0: every score +0.0, the docid decides (DESC: the largest first)
                for q, r in zip(qs[:3], got[:3]):
                    assert not r.scores.any() and r.docs.tolist() == sorted(r.docs.tolist(), reverse=True), q.terms


def test_ties_at_the_page_boundary(monkeypatch, capfd):
    """Thousands of docs share every score and the page boundary falls inside a tie class; at k1 = 1e-6 the classes
    differ in the last bits only, which is where the pruning bound's margins are thin."""
    rng = np.random.default_rng(77)
    words = ["alpha", "beta", "gamma", "delta", "kappa", "sigma", "omega"]
    protos = [" ".join(str(w) for w in rng.choice(words, size=int(rng.integers(1, 7)))) for _ in range(40)]
    texts = [protos[int(i)] for i in rng.integers(0, len(protos), size=300_000)]
    corpus = mg.Corpus.from_texts(texts)
    for group in _groups(PARAMS + [(1e-6, 1.0), (1e4, 0.0)]):
        p = Pair(corpus=corpus)
        for k1, b in group:
            qs = []
            for terms in (["al"], ["ma", "ga"], ["ta", "be", "et"], ["om", "eg", "ga"]):
                for limit, offset in ((10, 0), (37, 5), (100, 11), (1, 0)):
                    qs.append(Query(terms, sort_score=True, limit=limit, offset=offset, k1=k1, b=b))
            qs.append(Query(["ma", "ga"], sort_score=True, limit=10, descending=False, k1=k1, b=b))
            assert _run(p, qs, "default", monkeypatch, capfd)[1]["fast_queries"] == len(qs), (k1, b)
            assert _run(p, qs, "no-fast", monkeypatch, capfd)[1]["wave"] > 0, (k1, b)


@pytest.mark.parametrize("dense", [0.0, 4.0], ids=["dense-bitmaps", "lists-only"])
def test_saturated_tf_and_long_docs(dense, monkeypatch, capfd):
    """tf past the 4-bit nibble (15) and the tf byte (255), docs longer than the byte column (255 code points) and than
    the contribution tables, at b = 0 and 1 and at large k1."""
    docs = []
    for i in range(1, 40_001):
        docs.append((i, "ab" * (i % 27 + 1) + " cd " + ("ef " * (i % 4)) + "x" * ((i % 9) * 45)))
    docs[16] = (17, "ab" * 300 + " cd")
    docs[1233] = (1234, "cd " + "ab" * 255)
    docs[1999] = (2000, "ab" * 254 + " cd cd")
    docs[2998] = (2999, "cd" * 400 + "ab")
    first, texts = densify(docs)
    corpus = mg.Corpus.from_texts(texts)
    for group in _groups(PARAMS + [(20.0, 1.0), (1e4, 0.0), (2.0, 0.0)]):
        p = Pair(corpus=corpus, first_doc_id=first, dense_threshold=dense)
        for k1, b in group:
            qs = [Query(["ab", "cd"], sort_score=True, limit=25, k1=k1, b=b),
                  Query(["ab"], sort_score=True, limit=100, descending=False, k1=k1, b=b),
                  Query(["cd", "ef", "ab"], sort_score=True, limit=10, offset=5, k1=k1, b=b),
                  Query(["ab"], sort_score=True, limit=5, k1=k1, b=b)]
            for route in ROUTES:
                _, n = _run(p, qs, route, monkeypatch, capfd)
                if route == "default":  # bitmap-form grams: the fast path; sorted lists only: never
                    assert n["fast_queries"] == (len(qs) if dense == 0.0 else 0), (k1, b, n)
                if route == "no-fast":
                    assert n["wave"] + n["wave_lists"] + n["merge"] + n["cand"] > 0, (k1, b, n)


def test_selective_queries_and_lists(corpus300k, monkeypatch, capfd):
    """A sparse gram drives (cand_kernel); with MGX_CAND=0 the same queries take the wave kernel over a sorted list;
    on a lists-only index (dense_threshold 2.0) long drivers take the list merge, and at 0.18 bitmaps and lists mix."""
    p = Pair(corpus=corpus300k)
    c, sizes, g = _grams(p)
    rng = np.random.default_rng(12)
    sparse = [c.gram(i).decode() for i in g if 50 < sizes[i] < c.n_docs // 300]
    dense = [c.gram(i).decode() for i in g[:40]]
    seen = dict.fromkeys(KINDS, 0)
    for form, group in [(f, gr) for f in (0.0, 0.18, 2.0) for gr in _groups(PARAMS)]:
        p = Pair(corpus=corpus300k, dense_threshold=form)
        for k1, b in group:
            qs = []
            for j in range(10):
                terms = [sparse[int(rng.integers(0, len(sparse)))]] + [str(t) for t in rng.choice(dense, size=1 + j % 3,
                                                                                                 replace=False)]
                qs.append(Query(terms, sort_score=True, limit=int((1, 10, 100)[j % 3]), offset=j % 2 * 3,
                                descending=j != 9, k1=k1, b=b))
            for j in range(6):  # dense only: the merge kernel on the lists-only index
                qs.append(Query([str(t) for t in rng.choice(dense[:20], size=2 + j % 2, replace=False)], sort_score=True,
                                limit=(10, 100)[j % 2], k1=k1, b=b))
            for route in ROUTES:
                _, n = _run(p, qs, route, monkeypatch, capfd)
                for k in KINDS:
                    seen[k] += n[k]
                if route == "default" and form == 0.0:
                    assert n["cand"] > 0, (k1, b, n)
                if route == "default" and form == 2.0:
                    assert n["merge"] > 0, (k1, b, n)
                if route == "no-cand" and form == 0.0:
                    assert n["wave_lists"] > 0, (k1, b, n)
    assert all(seen[k] > 0 for k in KINDS), seen


def test_text_level_terms_expressions_and_fuzzy(corpus300k):
    """Whole-word terms (tf from the text), SORT _score over boolean expressions and over FUZZY results."""
    p = Pair(corpus=corpus300k)
    c, sizes, g = _grams(p)
    grams = [c.gram(i).decode() for i in g[:100]]
    words = sorted({w for i in range(0, 300_000, 211) for w in p.corpus.text(i).decode().split(" ") if 3 <= len(w) <= 8})
    rng = np.random.default_rng(41)
    for i, (k1, b) in enumerate(PARAMS):
        qs = [Query([words[int(rng.integers(0, len(words)))], grams[int(rng.integers(0, 30))]], sort_score=True,
                    limit=int(rng.choice([1, 10, 50])), descending=j != 3, k1=k1, b=b) for j in range(6)]
        _compare(p, qs, p.dev.search_batch(qs))
        ex = []
        for j in range(4):
            a, bb, cc = (words[int(rng.integers(0, len(words)))] if rng.random() < 0.4 else grams[int(rng.integers(0, 60))]
                         for _ in range(3))
            e = (("and", ("or", a, bb), cc), ("or", a, ("and", bb, cc)), ("and", a, ("not", bb)), ("or", a, bb, cc))[j]
            ex.append(Query(expr=e, sort_score=True, limit=10, descending=j != 2, k1=k1, b=b))
        _check_expr(p, ex)
        fq = [Query([words[int(rng.integers(0, len(words)))]], fuzzy=1, sort_score=True, limit=10, k1=k1, b=b)
              for _ in range(3)]
        for q, r in zip(fq, p.dev.search_batch(fq)):
            res = O.execute_fuzzy(p.oidx, p.ostore, q.terms, 1, ngram_size=2, kanji_ngram_size=0,
                                  cross_boundary=True)["results"]
            page, scores = _expected_scored(p, res, q.terms, q)
            assert r.total == len(res) and r.docs.tolist() == page.tolist(), (q.terms, k1, b)
            assert np.array_equal(r.scores, scores), (q.terms, k1, b)


def test_deep_pages(corpus300k, monkeypatch, capfd):
    """offset + limit past 1024 and unbounded pages: every match scored (score_candidates_mixed_kernel), device sort;
    a bounded page in the same batch takes the fast path."""
    p = Pair(corpus=corpus300k)
    c, sizes, g = _grams(p)
    top = [c.gram(i).decode() for i in g[:8]]
    for k1, b in PARAMS:
        qs = [Query([top[0], top[1]], sort_score=True, limit=100, offset=3000, k1=k1, b=b),
              Query([top[2], top[3], top[4]], sort_score=True, limit=1000, offset=25, descending=False, k1=k1, b=b),
              Query([top[5], top[7]], sort_score=True, limit=0, k1=k1, b=b),
              Query([top[0], top[6]], sort_score=True, limit=10, k1=k1, b=b)]
        assert _run(p, qs, "default", monkeypatch, capfd)[1]["fast_queries"] == 1, (k1, b)
        _run(p, qs, "block", monkeypatch, capfd)


def test_score_documents_over_the_grid():
    """BM25Scorer::ScoreDocuments on the device (tf columns and text scan) over the whole k1 x b grid and the
    statistics overrides."""
    rng = np.random.default_rng(9)
    words = ["ab", "abab", "cd", "xy", "abcd", "zz"]
    texts = [" ".join(str(w) for w in rng.choice(words, size=int(rng.integers(1, 12)))) for _ in range(5000)]
    texts[7], texts[8], texts[9] = "ab" * 20 + " cd", "ab" * 300 + " cd", "cd " + "x" * 300
    p = Pair(docs=list(enumerate(texts, start=1)))
    cand = np.asarray(list(range(1, 5001, 3)) + [8, 9, 10, 9_000_000], dtype=np.uint32)
    for terms in (["ab", "cd"], ["abab", "cd"]):
        dfs = [sum(1 for t in texts if term in t) for term in terms]
        for N, avg in ((p.N, p.avgdl), (p.N, 0.3), (p.N, p.avgdl * 10), (p.N, p.avgdl / 10), (min(dfs) // 2, p.avgdl),
                       (0, p.avgdl)):
            for k1 in K1:
                for b in B:
                    want = O.score_documents(p.ostore, cand, terms, dfs, N, avg, k1, b)
                    got = p.dev.score_documents(cand, terms, dfs, N, avg, k1, b)
                    assert np.array_equal(got, want), (terms, N, avg, k1, b)


# ---- several parameter sets on one index -----------------------------------------------------------------------------

def test_mixed_parameters_in_one_batch(corpus300k, monkeypatch, capfd):
    """Queries cycle through three (k1, b) sets, the same terms under two and three of them: the fast path takes one set, the
    others run on the wave / general kernels, and every query is exact."""
    p = Pair(corpus=corpus300k)
    sets = [(2.0, 0.3), (0.3, 1.0), (20.0, 0.3)]  # (the third differs from the first in k1 alone)
    base = _dense_queries(p, 0, 0, 300)
    qs = []
    for i, q in enumerate(base * 2):
        k1, b = sets[i % 3]
        qs.append(Query(q.terms, sort_score=True, limit=q.limit, offset=q.offset, descending=q.descending, k1=k1, b=b))
    _, n = _run(p, qs, "default", monkeypatch, capfd)
    # every query fits the fast path, but it takes the first set only: the other two run on the wave / general kernels
    first = [q for q in qs if (q.k1, q.b) == sets[0]]
    assert n["fast_queries"] == len(first) and n["wave"] + n["block"] > 0, n
    _, one = _run(p, first, "default", monkeypatch, capfd)
    assert one["fast_queries"] == len(first) and one["wave"] + one["block"] == 0, one
    _run(p, qs, "no-fast", monkeypatch, capfd)


def test_cache_keys(corpus300k, monkeypatch, capfd):
    """A, then B (only b differs), C (only avg_doc_length), D (only total_docs: only the idf changes), then A again,
    all on one index with the same terms: no table of one set may serve another. The statistics change the way a
    sharded table's do: through Index.total_docs / avg_doc_length (and the oracle's N / avgdl)."""
    p = Pair(corpus=corpus300k)
    own_n, own_avg = p.N, p.avgdl
    for (k1, b, N, avg) in [(2.0, 0.3, own_n, own_avg), (2.0, 0.9, own_n, own_avg), (2.0, 0.3, own_n, own_avg * 3),
                            (2.0, 0.3, own_n // 3, own_avg), (2.0, 0.3, own_n, own_avg)]:
        p.dev.total_docs = p.N = N
        p.dev.avg_doc_length = p.avgdl = avg
        qs = _dense_queries(p, k1, b, 400)
        assert _run(p, qs, "default", monkeypatch, capfd)[1]["fast_queries"] == len(qs), (k1, b, N, avg)
        assert _run(p, qs, "no-fast", monkeypatch, capfd)[1]["wave"] > 0, (k1, b, N, avg)


def test_block_max_cap(corpus300k, monkeypatch, capfd):
    """Block-max bytes are built for the first 4 parameter sets of an index (its memory grows by far more than one
    2 KiB K[dl] table per set), then no more; the 5th set and later run unpruned, still exact."""
    p = Pair(corpus=corpus300k)
    for i, k1 in enumerate([0.3, 0.7, 1.5, 2.5, 4.0, 9.0, 30.0]):
        before = p.dev.device_index.memory_bytes()
        qs = _dense_queries(p, k1, 0.5, 500 + i)
        assert _run(p, qs, "default", monkeypatch, capfd)[1]["fast_queries"] == len(qs)
        grew = p.dev.device_index.memory_bytes() - before
        if i < 4:
            assert grew > 64 * 1024, (i, grew)
        else:
            assert grew <= 4096, (i, grew)


def test_norm_table_cap(monkeypatch, capfd):
    """An index keeps 64 K[dl] tables: past them the fast path is off (0 fast items) and the queries run elsewhere,
    exact."""
    p = Pair(corpus=mg.Corpus.synthetic(40_000, seed=3))
    c, sizes, g = _grams(p)
    terms = [c.gram(i).decode() for i in g[:3]]
    for i in range(70):
        k1, b = 0.05 + 0.1 * i, (0.0, 0.3, 0.75, 1.0)[i % 4]
        qs = [Query(terms[:2], sort_score=True, limit=10, k1=k1, b=b),
              Query(terms, sort_score=True, limit=3, descending=False, k1=k1, b=b)]
        _, n = _run(p, qs, "default", monkeypatch, capfd)
        if i < 64:
            assert n["fast_queries"] == len(qs), (i, n)
        else:
            assert n["fast"] == 0 and n["wave"] + n["block"] > 0, (i, n)


def test_contribution_table_pool_fills(monkeypatch, capfd):
    """The wave kernels' contribution tables live in a pool of 2 * dense grams + 4096 tables per index; once it is
    full a query falls back to the general kernel. Every batch exact, before and after."""
    rng = np.random.default_rng(4)
    texts = ["".join(str(x) for x in rng.choice(list("abcde"), size=int(rng.integers(3, 40)))) for _ in range(6000)]
    p = Pair(docs=list(enumerate(texts, start=1)))
    c, sizes, g = _grams(p)
    grams = [c.gram(i).decode() for i in g]
    assert len(grams) == 25
    per_batch = 20
    wave_only, fell_back = 0, 0
    for batch in range(10):
        qs = []
        for s in range(per_batch):
            k1 = 0.01 + 0.01 * (batch * per_batch + s)
            qs += [Query([gr], sort_score=True, limit=10, k1=k1, b=0.6) for gr in grams]
        _, n = _run(p, qs, "no-fast", monkeypatch, capfd)
        if n["block"] == 0:
            wave_only += 1
        else:
            fell_back += 1
    assert wave_only > 0 and fell_back > 0, (wave_only, fell_back)


# ---- the reference's own non-default vectors on the fused path -------------------------------------------------------

@pytest.mark.parametrize("ngram", [5, 2], ids=["tf-column", "text-level"])
def test_golden_vectors_as_sort_score_batches(ngram, monkeypatch, capfd):
    bm = {v["id"]: v for v in G.load("bm25.json")["score_properties"]}
    for vid in ("k1_zero_is_pure_idf", "higher_tf_scores_higher"):
        v = bm[vid]
        p = Pair(docs=[(d, t) for d, t in v["docs"]], ngram=ngram, total_docs=v["N"], avg_doc_length=v["avgdl"])
        qs = [Query(v["terms"], sort_score=True, limit=10, k1=v["k1"], b=v["b"]),
              Query(v["terms"], sort_score=True, limit=10, descending=False, k1=v["k1"], b=v["b"])]
        for route in ("default", "block"):
            got, n = _run(p, qs, route, monkeypatch, capfd)  # ("block": only the general kernel ran)
            if route == "default" and ngram == 5:  # "hello" is one 5-gram: a dense tf column
                assert n["fast_queries"] == len(qs), (vid, n)
            by_doc = dict(zip(got[0].docs.tolist(), got[0].scores.tolist()))
            score = [by_doc[c] for c in v["candidates"]]
            assert eval(v["assert"], {"score": score, "abs": abs, "idf": O.compute_idf}), (vid, score)


def test_without_pruning_in_a_fresh_process():
    """MGX_NO_PRUNE is read once per process: the dense grid once more with block-max pruning off."""
    from pkg import ROOT
    env = dict(os.environ, MGX_NO_PRUNE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "dense_terms_every_parameter"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout, r.stdout[-2000:]
