"""-m gpu: the device column builder (mgx_columns_build_device, mygram-db_amd/csrc/mgx_build.hip). The bar: every array
and scalar of its view equals the host builder's for the same inputs, padding included — and, so that the device builder is
measured against the reference's restatement and not only against its sibling, the oracle's own check of the columns
(tests/test_host_cpu.py's, restated here): posting lists as Index::AddDocument leaves them, tf as CountTermOccurrences
counts, doc_len as CountCodePoints, the BM25 statistics of the document store."""
import numpy as np
import pytest

import golden_util as G
from gpu_util import Pair, OracleSide, densify
from oracle import oracle as O
from pkg import mg

pytestmark = pytest.mark.gpu
Query = mg.engine.Query

# (ngram, kanji, cross_boundary)
CONFIGS = [(2, 0, True), (1, 0, True), (3, 0, True), (2, 1, True), (2, 1, False), (1, 2, False), (3, 3, True)]

VIEW_ARRAYS = ("key_bytes", "key_off", "offsets", "docids", "tf", "doc_len", "tf_overflow_pos", "tf_overflow_val")
VIEW_SCALARS = ("n_grams", "n_postings", "first_doc_id", "n_docs", "bm25_doc_count", "bm25_total_len")


def _padded(cols, name, dtype):
    """docids / tf with the 4 entries of padding the host builder leaves behind them."""
    return mg.engine._np_view(getattr(cols.view, name), cols.n_postings + 4, dtype)


def assert_same_columns(host, dev):
    for k in VIEW_SCALARS:
        assert getattr(host, k) == getattr(dev, k), k
    assert int(host.view.n_tf_overflow) == int(dev.view.n_tf_overflow)
    for k in VIEW_ARRAYS:
        a, b = getattr(host, k), getattr(dev, k)
        assert a.dtype == b.dtype and np.array_equal(a, b), k
    assert np.array_equal(_padded(host, "docids", np.uint32), _padded(dev, "docids", np.uint32))
    assert np.array_equal(_padded(host, "tf", np.uint8), _padded(dev, "tf", np.uint8))
    for g in range(host.n_grams):
        assert dev.lookup(host.gram(g)) == g
    assert dev.lookup("\x01\x02") is None and dev.lookup("q\x01z") is None


def check_against_oracle(cols, texts, first_doc_id, ngram, kanji, cross, tf=True, tf_step=1):
    """tests/test_host_cpu.py::_check_columns_against_oracle over columns that exist already. tf=False: the texts hold
    invalid UTF-8 — a gram whose code points were separated by skipped bytes is a window of the document but no byte
    string of it, so CountTermOccurrences (a byte search) is not the tf of such texts for either builder."""
    oidx = O.Index(ngram, kanji, cross)
    store = O.DocumentStore()
    for i, t in enumerate(texts):
        oidx.add_document(first_doc_id + i, t)
        store.add(first_doc_id + i, t)
    assert cols.n_grams == oidx.gram_count()
    keys = [cols.gram(g) for g in range(cols.n_grams)]
    assert keys == sorted(keys)
    ovf = dict(zip(cols.tf_overflow_pos.tolist(), cols.tf_overflow_val.tolist()))
    assert cols.tf_overflow_pos.tolist() == sorted(ovf)
    for g, key in enumerate(keys):
        lo, hi = int(cols.offsets[g]), int(cols.offsets[g + 1])
        assert cols.docids[lo:hi].tolist() == oidx.search_and([key]).tolist(), key
        if tf:
            for p in range(lo, hi, tf_step):
                text = texts[int(cols.docids[p]) - first_doc_id]
                want = O.count_term_occurrences(text, key)
                assert cols.tf[p] == min(255, want), (key, p)
                assert (ovf.get(p) == want) if want >= 255 else (p not in ovf), (key, want)
    for i, t in enumerate(texts):
        assert cols.doc_len[i] == O.count_code_points(t)
    assert (cols.bm25_doc_count, cols.bm25_total_len) == store.bm25_stats()


def same(texts, first, ngram, kanji, cross, tf=True, tf_step=1, corpus=None):
    corpus = corpus if corpus is not None else mg.Corpus.from_texts(texts)
    host = mg.Columns(corpus, first, ngram, kanji, cross, n_threads=3)
    dev = mg.Columns(corpus, first, ngram, kanji, cross, device=0)
    assert_same_columns(host, dev)
    check_against_oracle(dev, texts, first, ngram, kanji, cross, tf=tf, tf_step=tf_step)
    return dev


MIXED = ["東京都", "東京は日本の首都です", "aあ東京b", "カタカナとひらがな", "abc東京def", "", "京", "a", "ab", "東a京b都c", "ｱｲｳ abc 漢字かな交じり文 xyz"]


def _sized(n):
    """n short documents over a small alphabet, some empty, some shorter than any n-gram."""
    rng = np.random.default_rng(n)
    alphabet = ["a", "b", "c", " ", "東", "京", "あ", "é", "\U00020000"]
    out = []
    for i in range(n):
        k = int(rng.integers(0, 12)) if i % 7 else 0
        out.append("".join(alphabet[int(rng.integers(0, len(alphabet)))] for _ in range(k)))
    return out


# name -> (texts, the texts are valid UTF-8)
SMALL = {
    "no documents": ([], True),
    "all empty": (["", "", ""], True),
    "shorter than n": (["a", "", "ab", "東", "b"], True),
    "one document": (["hello world 東京都 hello"], True),
    "mixed scripts": (MIXED, True),
    "63": (_sized(63), True),
    "64": (_sized(64), True),
    "65": (_sized(65), True),
    "257": (_sized(257), True),
    "1-4 byte code points": (["a\u00e9\u20ac\U0001F600", "\U0010FFFF\U0010FFFFa\U0010FFFF", "a\x00b\x00\x00c", "\x00",
                              "\u07ff\u0800\uffff\U00010000", "\ud7ff\ue000 x", "z\u007f\u0080z"], True),
    "greedy tf": (["aaaaa", "abababa", "aaaaaaa", "aaa", "aaaa", "aa bb aa", "東東東東東", "東京東京東京東"], True),
    "invalid utf-8": ([b"a\x80b", b"\x80\x80", b"ab\xc0\x80cd", b"x\xed\xa0\x80y", b"p\xf5\x80\x80\x80q", b"\xff\xfeab", b"ab\xe6\x9d",
                       b"\xb1\xe4\xba\xac", b"ab\xf0\x9f\x98", b"\x80\x80 tail", b"\xe6", b"\x9d\xb1", b"ok \xe6\x9d\xb1\xe4\xba\xac ok",
                       b"\xc2", b"\xa9 c", b"\xf4\x90\x80\x80", b"\xe0\x80\x80", b"\xe0\xa0\x80"], False),
}


@pytest.mark.parametrize("ngram,kanji,cross", CONFIGS)
def test_device_columns_equal_host_columns_and_the_oracle(ngram, kanji, cross):
    for name, (texts, valid) in SMALL.items():
        try:
            same(texts, 1, ngram, kanji, cross, tf=valid)
        except AssertionError as e:
            raise AssertionError("corpus %r: %s" % (name, e)) from e


def test_a_sequence_cut_off_by_the_end_of_its_document_is_not_completed_by_the_next():
    # "東" is e6 9d b1: the first document ends after e6, the second begins with 9d b1. A decode that read past the
    # document's end would see one ideograph; the reference sees three invalid bytes.
    texts = [b"ab\xe6", b"\x9d\xb1cd", b"\xf0\x9f", b"\x98\x80", b"ef"]
    for ngram, kanji, cross in CONFIGS:
        dev = same(texts, 1, ngram, kanji, cross, tf=False)
        assert dev.doc_len.tolist() == [2, 2, 0, 0, 2]
        assert dev.lookup("東") is None and dev.lookup("\U0001F600") is None


def test_texts_without_padding_and_offsets_that_do_not_begin_at_zero():
    # the ABI promises no padding behind the texts: the last document ends with a cut-off sequence at the very end of
    # the buffer, and doc 0 does not begin at byte 0
    raw = b"SKIPPED" + b"abc" + "東京".encode() + b"xy\xe6\x9d"
    off = np.asarray([7, 10, 16, 20], dtype=np.uint64)
    data = np.frombuffer(raw, dtype=np.uint8).copy()
    assert len(data) == int(off[-1])
    corpus = mg.Corpus(data, off)
    texts = [raw[7:10], raw[10:16], raw[16:20]]
    for ngram, kanji, cross in CONFIGS:
        dev = same(texts, 5, ngram, kanji, cross, tf=False, corpus=corpus)
        assert dev.doc_len.tolist() == [3, 2, 2]


@pytest.mark.parametrize("config", [None] + CONFIGS, ids=lambda c: "own" if c is None else "%d-%d-%s" % c)
def test_every_golden_corpus(config):
    """config None: each corpus under the n-gram sizes of its own golden case."""
    seen = set()
    for case in G.index_cases():
        docs = G.expand_docs(case["docs"])
        ic = case["index"]
        ngram, kanji, cross = config if config is not None else (ic["ngram"], ic.get("kanji", 0), True)
        first, texts = densify(docs)
        key = (first, tuple(texts), ngram, kanji)
        if key in seen:
            continue
        seen.add(key)
        same(texts, first, ngram, kanji, cross, tf_step=1 if len(texts) <= 3000 else 17)


def test_tf_saturates_the_byte_column_and_overflows_in_ascending_order():
    texts = ["a" * (2 * k) for k in (254, 255, 256, 299)] + ["aaaa", "b" * 600 + "a" * 512, ""]
    dev = same(texts, 1, 2, 0, True)
    g = dev.lookup("aa")
    lo = int(dev.offsets[g])
    assert dev.tf[lo:lo + 6].tolist() == [254, 255, 255, 255, 2, 255]
    assert dev.tf_overflow_val.tolist() == [255, 256, 299, 256, 300]  # "aa" of docs 2, 3, 4, 6; "bb" of doc 6
    assert np.all(np.diff(dev.tf_overflow_pos.astype(np.int64)) > 0)
    for ngram, kanji, cross in ((1, 0, True), (3, 0, True)):
        same(texts, 1, ngram, kanji, cross)


def test_one_document_of_70000_code_points_among_300_short_ones():
    rng = np.random.default_rng(9)
    short = _sized(300)
    words = ["abc", "abd", "東京", "都", " ", "xy", "あい"]
    long_doc = "".join(words[int(i)] for i in rng.integers(0, len(words), 40000))[:70000]
    assert len(long_doc) == 70000
    texts = short[:150] + [long_doc] + short[150:]
    for ngram, kanji, cross in ((2, 1, False), (3, 3, True)):
        dev = same(texts, 1, ngram, kanji, cross)
        assert dev.doc_len[150] == 70000
        assert len(dev.tf_overflow_val) > 1 and int(dev.tf_overflow_val.max()) > 255


@pytest.mark.parametrize("first", [1, 1000, 2**32 - 400])
def test_first_doc_id(first):
    texts = _sized(300)
    dev = same(texts, first, 2, 0, True)
    assert int(dev.docids.max()) <= first + 299 and int(dev.docids.min()) >= first


def test_two_device_builds_of_one_corpus_are_equal():
    corpus = mg.Corpus.synthetic(5000, seed=3)
    a = mg.Columns(corpus, 1, 2, 0, True, device=0)
    b = mg.Columns(corpus, 1, 2, 0, True, device=0)
    assert_same_columns(a, b)
    assert_same_columns(mg.Columns(corpus, 1, 2, 0, True), a)


def test_many_threads_build_at_once():
    import threading
    corpora = [mg.Corpus.from_texts(_sized(200 + 13 * i)) for i in range(6)]
    got, errs = [None] * 6, []

    def work(i):
        try:
            got[i] = mg.Columns(corpora[i], 1 + i, 2, 1, True, device=0)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(6)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(6):
        assert_same_columns(mg.Columns(corpora[i], 1 + i, 2, 1, True), got[i])


def test_a_bad_device_ordinal_is_an_invalid_argument():
    corpus = mg.Corpus.from_texts(["abc"])
    for dev in (-1, mg._capi.load().mgx_device_count()):
        with pytest.raises(mg._capi.MgxError) as e:
            mg.Columns(corpus, 1, 2, 0, True, device=dev)
        assert e.value.code == 2 and "bad device" in str(e.value)


class DevicePair(Pair):
    """gpu_util.Pair whose device index is made from device-built columns."""

    def __init__(self, corpus, first_doc_id=1, ngram=2, kanji=0, cross=True):
        self.dev = mg.Index(corpus=corpus, first_doc_id=first_doc_id, ngram_size=ngram, kanji_ngram_size=kanji,
                            cross_boundary=cross, build_device=0)
        OracleSide.__init__(self, self.dev.columns, corpus, first_doc_id)


def test_an_index_over_device_built_columns_serves_as_before():
    corpus = mg.Corpus.synthetic(5000, seed=3)
    p = DevicePair(corpus)
    assert_same_columns(mg.Columns(corpus, 1, 2, 0, True), p.dev.columns)
    c = p.dev.columns
    sizes = np.diff(c.offsets.astype(np.int64))
    grams = [c.gram(g).decode() for g in np.argsort(-sizes)[:50] if b" " not in c.gram(g)]
    rng = np.random.default_rng(4)
    qs = []
    for i in range(40):
        terms = [grams[int(rng.integers(0, len(grams)))] for _ in range(int(rng.integers(1, 4)))]
        nots = [grams[int(rng.integers(0, len(grams)))]] if i % 4 == 0 else []
        qs.append(Query(terms, not_terms=nots, sort_score=i % 2 == 0, descending=i % 3 != 0, limit=10))
    got = p.check(qs)
    assert sum(1 for r in got if r.total > 0) >= 20  # (the queries are not vacuous)
