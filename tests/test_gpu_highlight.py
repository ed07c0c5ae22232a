"""-m gpu: HIGHLIGHT on the device (highlight_kernel) through the C ABI (mgx_batch_set_highlight /
mgx_batch_fetch_highlight / mgx_highlight_render) and engine.py (Query(highlight=...), SearchResult.snippets).

Every returned snippet must equal highlight_ref.generate(text_of(doc), terms, options) — the line-cited restatement of
the reference's Highlighter that tests/test_highlight_cpu.py pins on the reference's own vectors — for that page's doc,
with the texts of the corpus the test built. Pages, totals, funnel counters and scores of a batch must not depend on
whether it is highlighted."""
import collections
import ctypes as C
import random

import numpy as np
import pytest

import highlight_ref as R
from pkg import mg

pytestmark = pytest.mark.gpu
Query, Highlight = mg.engine.Query, mg.engine.Highlight
_capi = mg._capi

NON_DEFAULT = dict(open_tag="【", close_tag="】", snippet_length=9, max_fragments=2)


def _ascii_index():
    corpus = mg.Corpus.synthetic(20_000, seed=7)
    return mg.Index(corpus=corpus, first_doc_id=1, ngram_size=2, kanji_ngram_size=0, device=0)


def _cjk_index():
    rng = random.Random(11)
    kanji = "東京都大阪市名古屋福岡札幌神戸横浜川崎"
    kana = "あいうえおタワービル"
    words = ["".join(rng.choice(kanji) for _ in range(rng.randint(2, 4))) for _ in range(60)]
    texts = []
    for _ in range(6000):
        parts = []
        for _ in range(rng.randint(3, 40)):
            r = rng.random()
            parts.append(rng.choice(words) if r < 0.7 else "".join(rng.choice(kana) for _ in range(rng.randint(1, 5)))
                         if r < 0.9 else rng.choice(["abc", "tower ", "\U00020000", " "]))
        texts.append("".join(parts))
    corpus = mg.Corpus.from_texts(texts)
    return mg.Index(corpus=corpus, first_doc_id=5, ngram_size=2, kanji_ngram_size=0, device=0), words


def _text_of(idx, doc):
    return bytes(idx.corpus.text(doc - idx.columns.first_doc_id))


def _norm(idx, term):
    return mg.engine.normalize_text(term, idx.normalize_nfkc, idx.normalize_width, idx.normalize_lower).encode("utf-8")


def _expected_terms(idx, q):
    """all_search_terms of the reference (plain: the terms; expression: the leaves not under a NOT; FUZZY: the terms as
    given) through BuildHighlightTerms."""
    names = []
    if q.expr is not None:
        def leaves(e, under_not):
            if isinstance(e, str):
                if not under_not:
                    names.append(e)
                return
            for c in e[1:]:
                leaves(c, under_not or e[0] == "not")
        leaves(q.expr, False)
    else:
        names = list(q.terms)
    return R.build_highlight_terms([t.encode("utf-8") for t in names], normalize=lambda b: _norm(idx, b.decode("utf-8")))


def _plain(q):
    """The same query without highlight."""
    c = Query.__new__(Query)
    c.__dict__.update(q.__dict__)
    c.highlight = None
    return c


def _check_batch(idx, queries):
    got = idx.search_batch(queries)
    base = idx.search_batch([_plain(q) for q in queries])
    n_snippets = 0
    for q, r, b in zip(queries, got, base):
        # the page itself does not depend on highlight
        assert r.total == b.total and r.docs.tolist() == b.docs.tolist() and np.array_equal(r.scores, b.scores)
        assert (r.total_candidates, r.after_intersection, r.after_not, r.after_filters) == \
            (b.total_candidates, b.after_intersection, b.after_not, b.after_filters)
        if q.highlight is None:
            assert r.snippets == []
            continue
        h = q.highlight
        terms = _expected_terms(idx, q)
        assert len(r.snippets) == len(r.docs)
        for doc, snippet in zip(r.docs.tolist(), r.snippets):
            want = R.generate(_text_of(idx, doc), terms, h.snippet_length, h.max_fragments, h.open_tag.encode("utf-8"),
                              h.close_tag.encode("utf-8"))
            assert snippet == want, (q.terms, q.expr, doc, snippet, want)
            n_snippets += 1
    return got, n_snippets


def _mixed_batch(words, rare_pair, hl):
    """The shapes of the issue's list; words[0..] are frequent words of the corpus, rare_pair never co-occurs."""
    w = words
    return [
        Query([w[0], w[1]], sort_score=True, limit=10, highlight=hl()),                      # AND + SORT _score top-10
        Query([w[2]], sort_score=False, limit=20, offset=5, descending=False, highlight=hl()),  # docid page ASC
        Query([w[3]], sort_score=False, limit=20, offset=5, descending=True, highlight=hl()),   # docid page DESC
        Query([w[4]], sort_score=True, limit=10, highlight=None),                            # off, between two on
        Query(expr=("and", w[0], ("not", w[1])), sort_score=True, limit=10, highlight=hl()),  # expression with NOT
        Query([w[5][:-1] + "q"], fuzzy=1, sort_score=False, limit=15, highlight=hl()),         # FUZZY
        Query([w[1], w[2]], sort_score=True, limit=10, verify_text=True, highlight=hl()),    # exact_text
        Query(list(rare_pair), sort_score=True, limit=10, highlight=hl()),                   # empty page
        Query(expr=("not", w[0]), sort_score=False, limit=12, highlight=hl()),               # no positive term: prefix path
        Query([w[0] + " " + w[1]], sort_score=True, limit=10, offset=3, highlight=hl()),      # a phrase: pieces are added
    ]


def _frequent_words(idx, n_docs):
    cnt = collections.Counter()
    docs_of = collections.defaultdict(set)
    for i in range(n_docs):
        for wd in bytes(idx.corpus.text(i)).decode("utf-8").split():
            if len(wd) >= 3:
                cnt[wd] += 1
                docs_of[wd].add(i)
    words = [wd for wd, _ in cnt.most_common(40)]
    rare = [wd for wd, c in cnt.items() if c == 1 and len(wd) >= 5]
    pair = next((a, b) for a in rare for b in rare if a != b and not (docs_of[a] & docs_of[b]))
    return words, pair


@pytest.mark.parametrize("options", [None, NON_DEFAULT], ids=["default", "non_default"])
def test_ascii_corpus(options):
    idx = _ascii_index()
    words, pair = _frequent_words(idx, 20_000)
    hl = (lambda: True) if options is None else (lambda: Highlight(**options))
    got, n = _check_batch(idx, _mixed_batch(words, pair, hl))
    assert n >= 80
    assert len(got[7].docs) == 0 and got[7].snippets == []
    assert all(b"<em>" not in s and "【".encode() not in s for s in got[8].snippets) and len(got[8].snippets) == 12


@pytest.mark.parametrize("options", [None, NON_DEFAULT], ids=["default", "non_default"])
def test_cjk_corpus(options):
    idx, words = _cjk_index()
    hl = (lambda: True) if options is None else (lambda: Highlight(**options))
    queries = [
        Query([words[0]], sort_score=True, limit=10, highlight=hl()),
        Query([words[1], words[2]], sort_score=False, limit=30, descending=False, highlight=hl()),
        Query([words[3]], sort_score=False, limit=30, descending=True, highlight=None),
        Query(expr=("or", words[4], ("and", words[5], ("not", words[6]))), sort_score=True, limit=10, highlight=hl()),
        Query([words[7][:2], words[7]], sort_score=True, limit=10, highlight=hl()),   # one term a prefix of the other
        Query(["タワー"], sort_score=False, limit=25, highlight=hl()),
        Query(["tower"], sort_score=True, limit=10, verify_text=True, highlight=hl()),
        Query(expr=("not", words[0]), sort_score=False, limit=8, highlight=hl()),
    ]
    _, n = _check_batch(idx, queries)
    assert n >= 80


def test_extreme_options():
    """snippet_length 1, max_fragments 1 and 100, a snippet longer than every text, a 256-byte tag."""
    idx = _ascii_index()
    words, _ = _frequent_words(idx, 20_000)
    queries = [
        Query([words[0]], sort_score=True, limit=10, highlight=Highlight(snippet_length=1, max_fragments=1)),
        Query([words[0][:2]], sort_score=False, limit=40, highlight=Highlight(snippet_length=3, max_fragments=100)),
        Query([words[1]], sort_score=True, limit=10, highlight=Highlight(snippet_length=10000, max_fragments=1)),
        Query([words[2]], sort_score=True, limit=10, highlight=Highlight(open_tag="x" * 256, close_tag="", snippet_length=7)),
    ]
    _, n = _check_batch(idx, queries)
    assert n >= 50


# ---- the C ABI's refusals -------------------------------------------------------------------------------------------

def _request(enabled=1, snippet_length=100, max_fragments=3, terms=(b"ab",)):
    arr = (C.c_char_p * max(len(terms), 1))(*terms)
    lens = (C.c_uint32 * max(len(terms), 1))(*[len(t) for t in terms])
    return _capi.HighlightRequest(enabled, snippet_length, max_fragments, len(terms), arr, lens), (arr, lens)


def _set(batch, reqs, max_text=0):
    L = _capi.load()
    arr = (_capi.HighlightRequest * len(reqs))(*[r for r, _ in reqs])
    rc = L.mgx_batch_set_highlight(batch._h, arr, len(reqs), max_text)
    return rc, L.mgx_last_error().decode()


def test_refusals():
    L = _capi.load()
    idx = _ascii_index()
    words, _ = _frequent_words(idx, 2_000)
    w = words[0][:2]  # one n-gram: needs no text
    # without attached texts
    assert not idx._text_attached
    b = idx.prepare([Query([w], sort_score=True, limit=10)])
    rc, msg = _set(b, [_request()])
    assert rc == 2 and "mgx_index_attach_text" in msg
    idx.ensure_text()
    # limit 0, offset + limit above the fused top-k page bound, a docid page above it
    for q in (Query([w], sort_score=True, limit=0), Query([w], sort_score=True, limit=1000, offset=25),
              Query([w], sort_score=False, limit=0), Query([w], sort_score=False, limit=1025)):
        b = idx.prepare([q])
        rc, msg = _set(b, [_request()])
        assert rc == 3 and ("limit" in msg), (rc, msg)
    b = idx.prepare([Query([w], sort_score=True, limit=1000, offset=24)])
    assert _set(b, [_request()])[0] == 0
    # option ranges
    for bad in (dict(snippet_length=0), dict(snippet_length=10001), dict(max_fragments=0), dict(max_fragments=101),
                dict(terms=tuple(b"t%03d" % i for i in range(257)))):
        b = idx.prepare([Query([w], sort_score=True, limit=10)])
        assert _set(b, [_request(**bad)])[0] == 3, bad
    # one request per query; only before the first execute; only once
    b = idx.prepare([Query([w], sort_score=True, limit=10)])
    assert _set(b, [_request(), _request()])[0] == 2
    b.execute()
    b.fetch()
    assert _set(b, [_request()])[0] == 2
    b = idx.prepare([Query([w], sort_score=True, limit=10)])
    assert _set(b, [_request()])[0] == 0 and _set(b, [_request()])[0] == 2
    # the arena's worst case above its cap: the message names the option to lower
    qs = [Query([w], sort_score=True, limit=1024) for _ in range(64)]
    b = idx.prepare(qs)
    rc, msg = _set(b, [_request(snippet_length=10000, max_fragments=100) for _ in qs], max_text=1 << 20)
    assert rc == 3 and "snippet_length" in msg and "MGX_HIGHLIGHT_ARENA_CAP" in msg
    # a sharded table: the exchange entry points refuse a highlighted batch before they touch anything
    b = idx.prepare([Query([w], sort_score=True, limit=10, highlight=True)])
    b.execute()
    dummy = (C.c_uint64 * 64)()
    assert L.mgx_batch_merge_shards(b._h, 1, dummy, 0, C.cast(dummy, C.c_void_p), 0, None) == 4
    assert "sharded" in L.mgx_last_error().decode()
    stride = C.c_uint32(0)
    assert L.mgx_batch_export_topk(b._h, None, None, C.byref(stride), None) == 4  # a host's own transport
    blob, nbytes, off32 = C.c_void_p(), C.c_uint64(), C.c_uint64()
    assert L.mgx_batch_export_buffer(b._h, C.byref(blob), C.byref(nbytes), C.byref(off32)) == 4
    fn = _capi.GATHER_FN(lambda *a: 7)
    assert L.mgx_batch_execute_gather(b._h, 2, fn, None, None) == 4
    r = b.fetch()[0]
    assert len(r.snippets) == len(r.docs) == 10
    # fetch_highlight before fetch
    b.execute()
    hv = _capi.HighlightView()
    assert L.mgx_batch_fetch_highlight(b._h, C.byref(hv)) == 2


def test_reset_drops_the_requests_and_reuses_the_batch():
    idx = _ascii_index()
    words, _ = _frequent_words(idx, 2_000)
    on = [Query([words[0]], sort_score=True, limit=10, highlight=True)]
    off = [Query([words[1]], sort_score=True, limit=10)]
    b = idx.prepare(on)
    b.execute()
    first = b.fetch()[0]
    assert len(first.snippets) == 10
    idx.prepare(off, into=b)
    b.execute()
    assert b.fetch()[0].snippets == []
    idx.prepare(on, into=b)
    b.execute()
    b.execute()  # a batch may be executed again
    again = b.fetch()[0]
    assert again.snippets == first.snippets and again.docs.tolist() == first.docs.tolist()
