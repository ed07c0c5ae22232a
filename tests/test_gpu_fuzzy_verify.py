"""-m gpu: FUZZY with verify_text — the edit-distance post-filter over the resident texts (kOpVerifyFuzzy) — through
engine.py. ExecuteWithFuzzy (src/server/search_pipeline.cpp:1659-1744) applies PostFilterByFuzzyText (:1746-1755) after
NOT terms and filters: a candidate stays when every normalized term is in its text (text.find) or fuzzily contained
(ContainsFuzzyMatch); RetainCandidatesMatchingText (:386-402) keeps a candidate without stored text. The oracle's
orc_execute_fuzzy(verify_text=1) leaves out the text.find short-circuit, so expectations are built from its primitives:
the unverified candidates and counters of execute_fuzzy(verify_text=False), then the rule of :1749-1753 restated here."""
import json
import os

import numpy as np
import pytest

from gpu_util import Pair
from oracle import oracle as O
from pkg import mg

pytestmark = pytest.mark.gpu
Query = mg.engine.Query


def _text(p, doc):
    first = p.dev.columns.first_doc_id
    t = p.corpus.text(doc - first)
    return None if t is None else bytes(t)


def _verified(p, candidates, terms, d):
    """PostFilterByFuzzyText, search_pipeline.cpp:1749-1753: every term found exactly or within d edits (no text: kept)."""
    keep = []
    for doc in candidates.tolist():
        text = _text(p, doc)
        if text is None or all(t in text or O.contains_fuzzy_match(text, t, d) for t in terms):
            keep.append(doc)
    return np.asarray(keep, dtype=np.uint32)


def _df(p, term):
    return O.execute(p.oidx, p.ostore, [term], compute_df=True, ngram_size=p.dev.ngram_size,
                     kanji_ngram_size=p.dev.kanji_ngram_size, cross_boundary=p.dev.cross_boundary)["term_df"][0]


def _expected(p, q):
    terms = [O.normalize_text(t) for t in q.terms]
    nots = [O.normalize_text(t) for t in q.not_terms]
    filters = [(p.filters[bid], neg) for bid, neg in q.filters]
    r = O.execute_fuzzy(p.oidx, p.ostore, terms, q.fuzzy, nots, filters, ngram_size=p.dev.ngram_size,
                        kanji_ngram_size=p.dev.kanji_ngram_size, cross_boundary=p.dev.cross_boundary,
                        verify_text=False)
    assert not r["exact_text_applied"], terms  # (the hybrid-fragment rule of :1733-1741 is another issue)
    res = _verified(p, r["results"], [t.encode("utf-8") for t in terms], q.fuzzy)
    scores = None
    if q.sort_score:
        dfs = [_df(p, t) for t in terms]
        sc = O.score_documents(p.ostore, res, terms, dfs, p.N, p.avgdl, q.k1, q.b)
        page = O.sort_by_score(res, sc, q.descending, q.limit, q.offset)
        lookup = dict(zip(res.tolist(), sc.tolist()))
        scores = np.asarray([lookup[x] for x in page.tolist()])
    else:
        page = res[::-1] if q.descending else res
        if q.limit:
            page = page[: q.limit]
    return r, res, page, scores


def _check(p, qs):
    got = p.dev.search_batch(qs)
    kept = dropped = 0
    for q, g in zip(qs, got):
        r, res, page, scores = _expected(p, q)
        ctx = (q.terms, q.fuzzy, q.not_terms, q.filters, q.sort_score, q.limit, q.offset, q.descending)
        assert g.total == len(res), ctx
        assert g.docs.tolist() == page.tolist(), (ctx, g.docs[:20], page[:20])
        if scores is not None:
            assert np.array_equal(g.scores, scores), (ctx, g.scores, scores)  # fp64, the reference's order: bit-exact
        for k in ("total_candidates", "after_intersection", "after_not", "after_filters"):
            assert getattr(g, k) == r[k], (ctx, k, getattr(g, k), r[k])
        kept += len(res)
        dropped += r["after_filters"] - len(res)
    return got, kept, dropped


def test_fuzzy_pipeline_vectors_verified():
    """tests/server/search_pipeline_test.cpp:2034-2078 (tests/golden/fuzzy.json) with verify_text on the device."""
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "fuzzy.json")))["pipeline"]
    for case in g["cases"]:
        docs = g["docs"] + case.get("extra_docs", [])
        kanji = case.get("query_kanji", g["index"]["kanji"])
        p = Pair(docs=[tuple(d) for d in docs], ngram=g["index"]["ngram"], kanji=kanji, cross=g["index"]["cross_boundary"])
        q = Query(case["terms"], fuzzy=case["distance"], verify_text=case["verify_text"], limit=0, descending=False)
        r = p.dev.search_batch([q])[0]
        got = r.docs.tolist()
        if "expect" in case:
            assert got == case["expect"], (case["id"], got)
        else:
            assert len(got) >= case["min_results"] and set(case["expect_contains"]) <= set(got), (case["id"], got)
        _check(p, [q])


def test_exact_substring_short_circuit():
    """"data" FUZZY 1: the candidates are the union of da/at/ta; "data" is a substring of the texts of 1 and 2 (no word of
    them is within one edit of it), "date" is one substitution away."""
    p = Pair(docs=[(1, "the databases are big"), (2, "a dataset"), (3, "date of birth"), (4, "tall tales")], ngram=2)
    q = Query(["data"], fuzzy=1, verify_text=True, limit=0, descending=False)
    g = p.dev.search_batch([q, Query(["data"], fuzzy=1, limit=0, descending=False)])
    assert g[0].docs.tolist() == [1, 2, 3]
    assert g[0].after_filters == g[1].total == 4 and g[0].total == 3
    _check(p, [q])


def _edit(rng, w, n):
    w = list(w)
    for _ in range(n):
        k = int(rng.integers(0, 4))
        if k == 0 and w:
            w[int(rng.integers(0, len(w)))] = chr(ord("a") + int(rng.integers(0, 26)))
        elif k == 1:
            w.insert(int(rng.integers(0, len(w) + 1)), chr(ord("a") + int(rng.integers(0, 26))))
        elif k == 2 and len(w) > 2:
            del w[int(rng.integers(0, len(w)))]
        elif len(w) > 1:
            i = int(rng.integers(0, len(w) - 1))
            w[i], w[i + 1] = w[i + 1], w[i]
    return "".join(w)


def _random_queries(p, rng, words, n, not_pool, edit_fn):
    fb = p.add_filter(np.arange(1, p.dev.columns.n_docs + 1, 3))
    shapes = [dict(limit=0, descending=False), dict(limit=50, descending=True),
              dict(sort_score=True, limit=10), dict(sort_score=True, offset=20, limit=100)]
    qs = []
    for i in range(n):
        d = 1 + i % 2
        terms = [edit_fn(rng, words[int(rng.integers(0, len(words)))], int(rng.integers(1, 3)))
                 for _ in range(1 + int(rng.integers(0, 2)))]
        nots = [not_pool[int(rng.integers(0, len(not_pool)))]] if rng.random() < 0.3 else []
        filters = [(fb, bool(rng.random() < 0.5))] if rng.random() < 0.3 else []
        qs.append(Query(terms, not_terms=nots, filters=filters, fuzzy=d, verify_text=True, **shapes[(i // 2) % 4]))
    return qs


def test_random_parity_multi_tile():
    p = Pair(corpus=mg.Corpus.synthetic(150_000, seed=23))
    rng = np.random.default_rng(24)
    words = sorted({w for i in range(0, 150_000, 89) for w in p.corpus.text(i).decode().split(" ") if 3 <= len(w) <= 9})
    qs = _random_queries(p, rng, words, 96, ["th", "er", "an", "zq"], _edit)
    qs = [q for q in qs if all(len(O.normalize_text(t)) >= 2 for t in q.terms)]
    _, kept, dropped = _check(p, qs)
    assert kept > 1000 and dropped > 1000, (kept, dropped)


KANJI = "東京都大阪府市区町村日本語学校先生電車駅前"
KANA = "のはにをがでとも"


def _cjk_corpus(n, seed):
    rng = np.random.default_rng(seed)
    texts = []
    for i in range(n):
        parts = []
        for _ in range(int(rng.integers(1, 4))):
            r = rng.random()
            if r < 0.5:  # an unspaced CJK run: one "word" of the window rule
                parts.append("".join(rng.choice(list(KANJI + KANA), int(rng.integers(4, 30)))))
            elif r < 0.8:
                parts.append("".join(rng.choice(list("abcdefgh"), int(rng.integers(2, 8)))))
            else:  # mixed-script word
                parts.append("".join(rng.choice(list("abcd" + KANJI[:6]), int(rng.integers(3, 10)))))
        sep = str(rng.choice([" ", "　", "\t"]))
        texts.append(sep.join(parts))
    return texts


def _edit_cjk(rng, w, n):
    al = list(KANJI + KANA) if any(ord(c) > 127 for c in w) else list("abcdefgh")
    w = list(w)
    for _ in range(n):
        k = int(rng.integers(0, 3))
        if k == 0 and w:
            w[int(rng.integers(0, len(w)))] = str(rng.choice(al))
        elif k == 1:
            w.insert(int(rng.integers(0, len(w) + 1)), str(rng.choice(al)))
        elif len(w) > 2:
            del w[int(rng.integers(0, len(w)))]
    return "".join(w)


def test_random_parity_cjk_windows():
    """Unspaced CJK runs (code-point windows, long words), kanji n-gram size 1: FUZZY terms cut from the runs."""
    texts = _cjk_corpus(40_000, 31)
    p = Pair(docs=list(enumerate(texts, start=1)), ngram=2, kanji=1, cross=False)
    rng = np.random.default_rng(32)
    pieces = []
    for i in range(0, len(texts), 53):
        for part in texts[i].replace("　", " ").replace("\t", " ").split(" "):
            if part and all(ord(c) > 127 for c in part) and len(part) >= 4:
                a = int(rng.integers(0, len(part) - 3))
                pieces.append(part[a:a + int(rng.integers(3, 6))])
            elif part and all(ord(c) < 128 for c in part) and len(part) >= 3:
                pieces.append(part)
    qs = _random_queries(p, rng, sorted(set(pieces)), 96, ["ab", "東京"], _edit_cjk)
    keep = []
    for q in qs:  # the hybrid-fragment exact-text rule is out of scope: only terms every code point of which is covered
        terms = [O.normalize_text(t) for t in q.terms]
        r = O.execute_fuzzy(p.oidx, p.ostore, terms, q.fuzzy, ngram_size=2, kanji_ngram_size=1, cross_boundary=False)
        if not r["exact_text_applied"]:
            keep.append(q)
    assert len(keep) > 30
    _, kept, dropped = _check(p, keep)
    assert kept > 200 and dropped > 200, (kept, dropped)
