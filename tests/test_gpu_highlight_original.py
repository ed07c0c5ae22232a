"""-m gpu: HIGHLIGHT from original texts on the device (highlight_original_kernel) through the C ABI
(mgx_index_attach_original_text, mgx_batch_set_highlight / _fetch_highlight, mgx_highlight_render) and engine.py
(Index.attach_original_text, SearchResult.snippets).

Every snippet of a page entry whose document has an original must equal highlight_original_ref.generate_original — the
line-cited restatement of Highlighter::GenerateOriginal that tests/test_highlight_original_cpu.py pins on the reference's
own vectors — and carry MGX_HL_ORIGINAL; every other entry must equal highlight_ref.generate over the normalized text, as
before, and not carry it. The normalizers are synthetic per-segment tables, so expansions, contractions and deletions all
occur; no Unicode work happens on the device, which sees texts, kinds and maps only."""
import ctypes as C
import random

import numpy as np
import pytest

import highlight_original_ref as O
import highlight_ref as R
from pkg import mg

pytestmark = pytest.mark.gpu
Query, Highlight = mg.engine.Query, mg.engine.Highlight
_capi = mg._capi

SENTINEL = "zzqq"  # one document holds it: NOT <sentinel> matches all the others
PAGE = 64          # a docid page has no offset (search_handler.cpp:469-470): a filter bitmap per PAGE documents cuts the pages
WIDE = {2: "é", 3: "京", 4: "\U00020000"}
TERMS = [t.encode() for t in ["ab", "bc", "a", "cab", "b c", "京", "é京", "q", "xé", "x京", "x\U00020000", "xxxq"]]


class Doc:
    def __init__(self, segments, kind=None, extra=""):
        """segments: [(original piece, its normalized piece)]; kind None: what build_map says. extra: appended to the
        whole-text normal form only (a normalizer that composes across segments: unmappable)."""
        self.segments = [(a.encode(), b.encode()) for a, b in segments]
        self.original = b"".join(a for a, _ in self.segments)
        self.normalized = b"".join(b for _, b in self.segments) + extra.encode()
        self.kind, self.pairs = O.build_map(self.original, self.normalized, self.segments)
        if kind == O.ORIG_NONE:
            self.kind, self.pairs, self.original = O.ORIG_NONE, None, None

    def want(self, terms, h):
        args = (h.snippet_length, h.max_fragments, h.open_tag.encode(), h.close_tag.encode())
        if self.kind == O.ORIG_NONE:
            return R.generate(self.normalized, terms, *args)
        return O.generate_original(self.original, self.normalized, self.segments, terms, *args)


def _random_doc(rng, i):
    src, dst = "ABCÉ京\U0001F600 ", "abc é京"
    segments = []
    for _ in range(rng.randint(1, 70)):
        r = rng.random()
        if r < 0.5:
            c = rng.choice(src)
            segments.append((c, {"A": "a", "B": "b", "C": "c", "É": "é"}.get(c, c) if c in dst + "ABCÉ" else rng.choice(dst)))
        elif r < 0.7:
            segments.append((rng.choice(src), "".join(rng.choice("abc") for _ in range(rng.randint(2, 4)))))
        elif r < 0.9:
            segments.append(("".join(rng.choice(src) for _ in range(rng.randint(2, 3))), rng.choice(dst)))
        else:
            segments.append((rng.choice(src), ""))
    if i % 6 == 0:  # pure 1 -> 1: identity
        segments = [(a[0], b[0] if b else "a") for a, b in segments]
    if i % 5 == 1:  # ends with a match, at the original's last code point
        segments += [("A", "a"), ("Q", "q")]
    return Doc(segments, kind=O.ORIG_NONE if i % 7 == 3 else None, extra="z" if i % 9 == 4 else "")


def _sized_docs():
    """Texts of 1, 63, 64, 65, 128 and 129 bytes (and their neighbours, so that both the original and the normalized text
    take each size), with a 2-, 3- or 4-byte character that starts at byte 62, 63 or 64 and a term over it; the normalized
    text is as long as the original, one byte shorter (a contraction in front) or one longer (an expansion in front), so
    the character lies across byte 63/64 of the one, of the other, or of both."""
    docs, seen = [], set()
    for size in (1, 2, 62, 63, 64, 65, 66, 127, 128, 129, 130):
        for w, ch in WIDE.items():
            for start in (62, 63, 64):
                for front in ("same", "contract", "expand"):
                    rest = size - start - w
                    if rest >= 0:
                        body = ["X"] * start + [ch] + (["X"] * (rest - 1) + ["Q"] if rest else [])
                    else:
                        body = ["X"] * (size - 1) + ["Q"]
                    segs = [(c, c.lower() if c in "XQ" else c) for c in body]
                    if front == "contract" and len(segs) > 2:
                        segs[:2] = [("XX", "x")]
                    elif front == "expand" and len(segs) > 1:
                        segs[0] = ("X", "xx")
                    d = Doc(segs)
                    if (d.original, d.normalized) not in seen:
                        seen.add((d.original, d.normalized))
                        docs.append(d)
    return docs


def _hand_docs():
    return [
        # a match that starts and ends inside expanded segments: "X" -> "cab", "Y" -> "abc"; the term "ab" ... "bc"
        Doc([("X", "cab"), ("Y", "bc "), ("A", "a")]),
        # two terms, one shared start after the translation, the later range longer: "a" -> (0, 1), "bc" -> (0, 2)
        Doc([("X", "ab"), ("C", "c"), (" ", " "), ("Z", "q")]),
        # two matches inside one expanded segment: equal ranges
        Doc([("X", "abab"), ("!", "")]),
        Doc([("!", ""), ("?", "")]),           # a normalized text without a code point
        Doc([("A", "a")]), Doc([("Q", "q")]),  # one byte
        Doc([("A", "a"), ("B", "b")], extra="zz"),  # unmappable
        Doc([("a", "a"), ("b", "b"), (" ", " "), ("c", "c")], kind=O.ORIG_NONE),
        Doc([("Ａ", "a"), ("Ｂ", "b"), ("　", " "), ("É", "é"), ("京", "京"), ("Ｑ", "q")]),  # identity, all wider
    ]


class Table:
    def __init__(self, docs, first_doc_id=1):
        self.docs = list(docs) + [Doc([(c, c) for c in SENTINEL], kind=O.ORIG_NONE)]
        self.first = first_doc_id
        self.idx = mg.Index(corpus=mg.Corpus.from_texts([d.normalized for d in self.docs]), first_doc_id=first_doc_id,
                            ngram_size=2, kanji_ngram_size=0, device=0, normalize_nfkc=False, normalize_lower=False)
        self.attach()
        ids = np.arange(first_doc_id, first_doc_id + len(self.docs), dtype=np.uint32)
        self.chunks = [self.idx.device_index.add_filter_bitmap(ids[o:o + PAGE]) for o in range(0, len(ids), PAGE)]

    def attach(self):
        self.idx.attach_original_text([d.original for d in self.docs], [d.kind for d in self.docs],
                                      [d.pairs if d.kind == O.ORIG_MAPPED else None for d in self.docs])

    def doc(self, doc_id):
        return self.docs[doc_id - self.first]


@pytest.fixture(scope="module")
def table():
    rng = random.Random(4242)
    return Table(_hand_docs() + _sized_docs() + [_random_doc(rng, i) for i in range(150)])


def _run(idx, queries, hls, max_text=0, merge_with=None):
    """Prepare, attach explicit highlight requests ((Highlight, [term bytes]) or None per query), execute (merging with
    the same queries on another index if asked), fetch: the results and every page entry's record flags."""
    L = _capi.load()
    b = idx.prepare(queries)
    reqs = (_capi.HighlightRequest * len(queries))()
    keep = []
    for i, h in enumerate(hls):
        if h is None:
            continue
        terms = list(h[1])
        arr = (C.c_char_p * max(len(terms), 1))(*terms)
        lens = (C.c_uint32 * max(len(terms), 1))(*[len(t) for t in terms])
        keep.append((arr, lens))
        reqs[i] = _capi.HighlightRequest(1, h[0].snippet_length, h[0].max_fragments, len(terms), arr, lens)
    _capi.check(L.mgx_batch_set_highlight(b._h, reqs, len(queries), max_text))
    b._highlights = list(hls)
    if merge_with is not None:
        _capi.check(L.mgx_batch_defer_highlight(b._h, 1))
        other = merge_with.prepare(queries)
        b.execute()
        other.execute()
        _capi.check(L.mgx_batch_merge_local(b._h, (C.c_void_p * 1)(other._h.value), 1, None))
    else:
        b.execute()
    res = b.fetch()
    if merge_with is not None:
        other.fetch()
    hv = _capi.HighlightView()
    _capi.check(L.mgx_batch_fetch_highlight(b._h, C.byref(hv)))
    flags, at = [], 0
    for r in res:
        flags.append([int(hv.entries[at + j].flags) for j in range(len(r.docs))])
        at += len(r.docs)
    assert at == hv.n_entries
    return res, flags


def _check_pages(table_of, res, flags, hls):
    """table_of(doc id) -> Doc. Returns how many entries were built from an original / from a normalized text."""
    n_orig = n_norm = 0
    for r, fl, h in zip(res, flags, hls):
        assert len(r.snippets) == len(r.docs) == len(fl)
        for doc_id, snippet, f in zip(r.docs.tolist(), r.snippets, fl):
            d = table_of(doc_id)
            want = d.want(h[1], h[0])
            assert snippet == want, (doc_id, d.kind, d.original, d.normalized, d.pairs, h[1], vars(h[0]), snippet, want)
            assert bool(f & _capi.HL_ORIGINAL) == (d.kind != O.ORIG_NONE), (doc_id, d.kind, f)
            assert not f & 4
            n_orig += d.kind != O.ORIG_NONE
            n_norm += d.kind == O.ORIG_NONE
    return n_orig, n_norm


def _all_pages(chunks):
    """One docid page per filter bitmap: together every document but the sentinel, ASC and DESC in turn."""
    return [Query(expr=("not", SENTINEL), filters=[(c, False)], sort_score=False, limit=PAGE, descending=bool(k % 2))
            for k, c in enumerate(chunks)]


OPTIONS = {
    "default": (Highlight(), TERMS),
    "L1_F1": (Highlight(snippet_length=1, max_fragments=1, open_tag="[", close_tag="]"), TERMS),
    "L10000_F100": (Highlight(snippet_length=10000, max_fragments=100), TERMS),
    "L7_F100": (Highlight(snippet_length=7, max_fragments=100, open_tag="【", close_tag="】"), TERMS),
    "L2_F1": (Highlight(snippet_length=2, max_fragments=1), TERMS),       # the early stop, a pending range held
    "L4_F3_dense": (Highlight(snippet_length=4, max_fragments=3), TERMS + [b"x", b" "]),
    "no_terms": (Highlight(snippet_length=10), []),
    "empty_terms_only": (Highlight(snippet_length=10), [b"", b""]),
}


@pytest.mark.parametrize("name", list(OPTIONS))
def test_docid_pages_over_every_document(table, name):
    h = OPTIONS[name]
    queries = _all_pages(table.chunks)
    res, flags = _run(table.idx, queries, [h] * len(queries))
    seen = sorted(d for r in res for d in r.docs.tolist())
    assert seen == list(range(1, len(table.docs)))  # every document but the sentinel, once (the empty text included)
    n_orig, n_norm = _check_pages(table.doc, res, flags, [h] * len(queries))
    assert n_orig >= 200 and n_norm >= 15


def test_the_corpus_holds_the_shapes_the_issue_lists(table):
    """What the pages above compared, counted on the checker's side."""
    docs = table.docs[:-1]
    kinds = [d.kind for d in docs]
    for k in (O.ORIG_NONE, O.ORIG_IDENTITY, O.ORIG_MAPPED, O.ORIG_UNMAPPABLE):
        assert kinds.count(k) >= 5, k
    sizes_o = {len(d.original) for d in docs if d.original is not None}
    sizes_n = {len(d.normalized) for d in docs if d.kind != O.ORIG_NONE}
    assert {1, 63, 64, 65, 128, 129} <= sizes_o and {1, 63, 64, 65, 128, 129} <= sizes_n

    def straddles(b):
        return len(b) > 64 and (b[64] & 0xC0) == 0x80
    for w, ch in WIDE.items():
        assert any(straddles(d.original) and ch.encode() in d.original[60:68] for d in docs if d.original)
        assert any(straddles(d.normalized) and ch.encode() in d.normalized[60:68] for d in docs if d.kind == O.ORIG_MAPPED)
    shared = inside = at_end = early = 0
    for d in docs:
        if d.kind in (O.ORIG_NONE, O.ORIG_UNMAPPABLE):
            continue
        m = O.segment_map(d.segments)
        matches = R.find_match_positions(d.normalized, TERMS)
        ranges = O.translated_matches(d.normalized, d.segments, TERMS)
        kept = O.remove_overlapping_match_positions(ranges)
        shared += any(a[0] == b[0] and b[1] > a[1] for a, b in zip(ranges, ranges[1:]))
        inside += any(s > 0 and m[s] == m[s - 1] and e < len(m) and m[e - 1] == m[e] for s, e in matches)
        at_end += bool(kept) and kept[-1][1] == R.count_code_points(d.original)
        # L = 2, F = 1: the first window closes while a later range is held
        early += len(R.merge_windows([(s - 1 if s > 1 else 0, e + 1) for s, e in kept])) > 1 and len(kept) > 2
    assert shared >= 3 and inside >= 3 and at_end >= 10 and early >= 20, (shared, inside, at_end, early)


def test_score_pages_through_the_engine(table):
    """SORT _score pages, requested the ordinary way: Query(highlight=...), the engine builds the term lists."""
    hs = [Highlight(), Highlight(snippet_length=5, max_fragments=2, open_tag="<b>", close_tag="</b>")]
    queries = [Query(["ab"], sort_score=True, limit=64, highlight=hs[0]),
               Query(["bc", "ca"], sort_score=True, limit=40, offset=3, highlight=hs[1]),
               Query(["xx"], sort_score=True, limit=64),
               Query(["xq"], sort_score=False, limit=50, offset=2, descending=True, highlight=hs[1])]  # a docid page, DESC
    res = table.idx.search_batch(queries)
    assert res[2].snippets == [] and len(res[2].docs) > 0
    n = 0
    for q, r, terms in ((queries[0], res[0], [b"ab"]), (queries[1], res[1], [b"bc", b"ca"]), (queries[3], res[3], [b"xq"])):
        assert len(r.docs) >= 20 and len(r.snippets) == len(r.docs)
        for doc_id, snippet in zip(r.docs.tolist(), r.snippets):
            assert snippet == table.doc(doc_id).want(terms, q.highlight), doc_id
            n += table.doc(doc_id).kind in (O.ORIG_IDENTITY, O.ORIG_MAPPED)
    assert n >= 30


def test_a_table_with_a_delta_on_the_merged_page():
    """The main index and a delta (mgx_batch_merge_local re-runs the highlight step): a document's original comes from the
    index that holds the live document — the main index only, the delta only, or a document updated into the delta
    without an original, whose old original in the main index must not be used."""
    L = _capi.load()
    rng = random.Random(99)
    main_docs = [d for d in (_random_doc(rng, i) for i in range(400)) if d.kind in (O.ORIG_IDENTITY, O.ORIG_MAPPED)][:90]
    main = Table(main_docs, first_doc_id=1)
    assert len(main_docs) == 90
    updated_plain, updated_orig = [5, 17, 40], [7, 18, 64]
    delta_docs, ids = [], []
    for t in updated_plain:  # updated without an original
        delta_docs.append(Doc([("a", "a"), ("b", "b"), (" ", " "), ("q", "q"), (chr(ord("a") + t % 3), chr(ord("a") + t % 3))],
                              kind=O.ORIG_NONE))
        ids.append(t)
    for t in updated_orig:   # updated with a new original
        delta_docs.append(Doc([("X", "cab"), ("Y", "bc "), ("Q", "q")] * (1 + t % 3)))
        ids.append(t)
    for j in range(30):      # new documents, with and without originals
        delta_docs.append(_random_doc(rng, j))
        ids.append(1000 + 3 * j)
    order = np.argsort(ids, kind="stable")
    delta_docs, ids = [delta_docs[k] for k in order], np.asarray(ids, np.uint32)[order]
    delta = Table(delta_docs, first_doc_id=1)
    sentinel_id = 5000
    table_ids = np.concatenate([ids, [sentinel_id]]).astype(np.uint32)
    _capi.check(L.mgx_index_set_doc_map(delta.idx.device_index._h, table_ids.ctypes.data, len(table_ids)))
    live = [d for d in range(1, len(main.docs) + 1) if d not in updated_plain + updated_orig]
    bitmap = main.idx.device_index.add_filter_bitmap(live)
    _capi.check(L.mgx_index_set_live_bitmap(C.c_void_p(main.idx.device_index._h.value), C.c_uint32(bitmap), C.c_int(1)))
    by_id = {int(t): d for t, d in zip(ids, delta_docs)}

    def table_of(doc_id):
        return by_id[doc_id] if doc_id in by_id else main.doc(doc_id)
    longest = max(main.idx.device_index.max_original_text_bytes(), delta.idx.device_index.max_original_text_bytes(),
                  max(len(d.normalized) for d in main.docs + delta.docs))
    h = (Highlight(snippet_length=12, max_fragments=2), TERMS)
    queries = [Query(expr=("not", SENTINEL), sort_score=False, limit=2 * PAGE, descending=False),  # (120 documents)
               Query(expr=("not", SENTINEL), sort_score=False, limit=PAGE, descending=True),
               Query(["ab"], sort_score=True, limit=PAGE)]
    hls = [h] * len(queries)
    res, flags = _run(main.idx, queries, hls, max_text=longest, merge_with=delta.idx)
    everything = sorted(live[:-1] + [int(t) for t in ids])  # (live[-1] is the main index's sentinel)
    assert res[0].docs.tolist() == everything and res[1].docs.tolist() == everything[::-1][:PAGE]
    n_orig, n_norm = _check_pages(table_of, res, flags, hls)
    assert n_orig >= 100 and n_norm >= 6
    assert len(res[-1].docs) >= 20 and any(d >= 1000 for d in res[-1].docs.tolist())


# ---- the C ABI: refusals, memory ------------------------------------------------------------------------------------

def _attach(idx, originals, kinds, maps):
    try:
        idx.device_index.attach_original_text(originals, kinds, maps)
    except Exception as e:  # noqa: BLE001
        return str(e)
    return None


def test_attach_refusals_name_the_slot():
    L = _capi.load()
    idx = mg.Index(corpus=mg.Corpus.from_texts(["ab", "abc", "é"]), first_doc_id=1, ngram_size=2, kanji_ngram_size=0, device=0)
    ok = (["AB", "ABC", "É"], [1, 1, 1], None)
    msg = _attach(idx, *ok)
    assert msg and "mgx_index_attach_text" in msg  # the normalized texts come first
    idx.ensure_text()
    assert _attach(idx, *ok) is None
    cases = [
        ((["AB", b"A\xffC", "É"], [1, 1, 1], None), ["slot 1", "UTF-8"]),
        ((["AB", b"AB\xe4\xba", "É"], [1, 3, 1], None), ["slot 1", "UTF-8"]),       # a truncated character, unmappable kind
        ((["AB", "ABCD", "É"], [1, 1, 1], None), ["slot 1", "identity", "4 code points", "3"]),
        ((["AB", "AC", "É"], [1, 2, 1], [None, [(0, 1), (1, 2)], None]), ["slot 1", "2 pairs", "3 code points"]),
        ((["AB", "AC", "É"], [1, 2, 1], [None, [(0, 1), (1, 1), (1, 2)], None]), ["slot 1", "pair 1", "start < end"]),
        ((["AB", "AC", "É"], [1, 2, 1], [None, [(0, 1), (1, 3), (1, 2)], None]), ["slot 1", "pair 1", "start < end"]),
        ((["AB", "AC", "É"], [1, 2, 1], [None, [(1, 2), (0, 2), (1, 2)], None]), ["slot 1", "pair 1", "decrease"]),
        ((["AB", "AC", "É"], [1, 2, 1], [None, [(0, 2), (1, 2), (1, 1 + 1)], None]), None),
        ((["AB", "ACD", "É"], [1, 2, 1], [None, [(0, 3), (1, 3), (1, 2)], None]), ["slot 1", "pair 2", "decrease"]),
        ((["AB", "ABC", "É"], [1, 4, 1], None), ["slot 1", "kind 4"]),
        ((["AB", "ABC", "É"], [1, 1, 0], [None, None, [(0, 1)]]), ["slot 2", "MGX_ORIG_MAPPED"]),
    ]
    for args, want in cases:
        msg = _attach(idx, *args)
        if want is None:
            assert msg is None, (args, msg)
            continue
        assert msg is not None, args
        for piece in ["mgx_index_attach_original_text"] + want:
            assert piece in msg, (args, msg)
    # null arguments
    assert L.mgx_index_attach_original_text(idx.device_index._h, None, None, None, None, None) == 2
    n = C.c_uint32(7)
    assert L.mgx_index_max_original_text_bytes(None, C.byref(n)) == 2 and n.value == 0


def test_memory_bytes_grow_by_the_maps():
    texts = ["ab cd", "abc", "q", "abab"]
    idx = mg.Index(corpus=mg.Corpus.from_texts(texts), first_doc_id=1, ngram_size=2, kanji_ngram_size=0, device=0)
    idx.ensure_text()
    dev = idx.device_index
    assert dev.max_original_text_bytes() == 0
    before = dev.memory_bytes()
    originals = ["AB CD", "XC", "Q", "ＡＢＡＢ"]
    dev.attach_original_text(originals, [1, 3, 1, 1], None)  # no document is mapped: no map
    without = dev.memory_bytes()
    assert without > before
    maps = [None, [(0, 1), (0, 1), (1, 2)], None, None]
    dev.attach_original_text(originals, [1, 2, 1, 1], maps)
    assert dev.memory_bytes() - without == 8 * 3  # 8 bytes per normalized code point of the mapped document
    assert dev.max_original_text_bytes() == len("ＡＢＡＢ".encode())
    r = idx.search_batch([Query(["ab"], sort_score=False, limit=10, descending=False, highlight=True)])[0]
    assert r.docs.tolist() == [1, 2, 4]
    assert r.snippets == [b"<em>AB</em> CD", b"<em>X</em>C", "<em>ＡＢ</em><em>ＡＢ</em>".encode()]
    # new normalized texts drop the originals (they were checked against the old ones)
    dev.attach_text(idx.corpus)
    assert dev.max_original_text_bytes() == 0 and dev.memory_bytes() == before
    r = idx.search_batch([Query(["ab"], sort_score=False, limit=10, descending=False, highlight=True)])[0]
    assert r.snippets == [b"<em>ab</em> cd", b"<em>ab</em>c", b"<em>ab</em><em>ab</em>"]
