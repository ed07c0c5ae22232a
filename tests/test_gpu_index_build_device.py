"""-m gpu: mgx_index_build_device (a serving index from normalized texts in one call, the postings never on the host) and
mgx_index_read_postings. The bar: the dictionary equals the host builder's columns in everything but docids / tf; the
index equals, array by array as far as the ABI lets a caller read device memory (posting lists, tf bytes, texts, text
offsets, memory_bytes, max_text_bytes), the one mgx_index_create + mgx_index_attach_text make of the host builder's
columns; and it serves as the oracle answers over the host columns."""
import ctypes as C
import threading

import numpy as np
import pytest

from gpu_util import OracleSide, Pair
from pkg import mg
from test_gpu_columns_device import CONFIGS, SMALL, _sized

pytestmark = pytest.mark.gpu
Query = mg.engine.Query
K = mg._capi
INVALID, OUT_OF_RANGE, NOT_IMPLEMENTED = 2, 3, 4

DICT_ARRAYS = ("key_bytes", "key_off", "offsets", "doc_len", "tf_overflow_pos", "tf_overflow_val")
DICT_SCALARS = ("n_grams", "n_postings", "first_doc_id", "n_docs", "bm25_doc_count", "bm25_total_len")


def assert_same_dictionary(host, dic):
    for k in DICT_SCALARS:
        assert getattr(host, k) == getattr(dic, k), k
    assert int(host.view.n_tf_overflow) == int(dic.view.n_tf_overflow)
    for k in DICT_ARRAYS:
        a, b = getattr(host, k), getattr(dic, k)
        assert a.dtype == b.dtype and np.array_equal(a, b), k
    assert not dic.view.docids and not dic.view.tf  # the postings are not on the host
    if host.n_postings:
        assert dic.docids is None and dic.tf is None
    for g in range(host.n_grams):
        assert dic.lookup(host.gram(g)) == g
    assert dic.lookup("\x01\x02") is None


def read_texts(index, n_docs):
    """mgx_index_copy_text -> (rc, text bytes, n_docs + 1 offsets); (rc, None, None) when the index refuses."""
    L = K.load()
    L.mgx_index_copy_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
    total = C.c_uint64()
    rc = L.mgx_index_copy_text(index._h, None, 0, None, C.byref(total))
    if rc != 0:
        return rc, None, None
    data = np.zeros(int(total.value) + 1, dtype=np.uint8)
    off = np.zeros(n_docs + 1, dtype=np.uint64)
    K.check(L.mgx_index_copy_text(index._h, data.ctypes.data, total.value, off.ctypes.data, C.byref(total)))
    return 0, data[:int(total.value)], off


def max_text_bytes(index):
    n = C.c_uint32()
    K.check(K.load().mgx_index_max_text_bytes(index._h, C.byref(n)))
    return int(n.value)


def same_index(corpus, first, ngram, kanji, cross, dense_threshold=0.0, attach=True, gram_step=1):
    """Builds the index both ways and compares them. Returns (host columns, dictionary, resident index), or None when both
    paths refuse with the same code."""
    host = mg.Columns(corpus, first, ngram, kanji, cross, n_threads=3)
    try:
        ref = mg.DeviceIndex(host, 0, dense_threshold)
    except K.MgxError as e:
        with pytest.raises(K.MgxError) as got:
            mg.DeviceIndex.build_resident(corpus, first, ngram, kanji, cross, 0, dense_threshold, attach_text=attach)
        assert got.value.code == e.code, (got.value, e)
        return None
    if attach:
        ref.attach_text(corpus)
    dic, res = mg.DeviceIndex.build_resident(corpus, first, ngram, kanji, cross, 0, dense_threshold, attach_text=attach)
    assert_same_dictionary(host, dic)
    for g in range(0, host.n_grams, gram_step):
        lo, hi = int(host.offsets[g]), int(host.offsets[g + 1])
        d, t = res.read_postings(g)
        assert np.array_equal(d, host.docids[lo:hi]) and np.array_equal(t, host.tf[lo:hi]), host.gram(g)
        d2, t2 = ref.read_postings(g)
        assert np.array_equal(d, d2) and np.array_equal(t, t2), host.gram(g)
    assert res.memory_bytes() == ref.memory_bytes()
    rc, data, off = read_texts(res, corpus.n_docs)
    rc2, data2, off2 = read_texts(ref, corpus.n_docs)
    assert rc == rc2
    if attach:
        base = int(corpus.text_off[0])
        assert rc == 0 and int(off[0]) == 0
        assert np.array_equal(off, corpus.text_off - corpus.text_off[0]) and np.array_equal(off, off2)
        assert np.array_equal(data, corpus.text_bytes[base:int(corpus.text_off[-1])]) and np.array_equal(data, data2)
        assert max_text_bytes(res) == max_text_bytes(ref) == int(np.diff(corpus.text_off.astype(np.int64)).max())
    else:
        assert rc == INVALID and "holds no texts" in K.load().mgx_last_error().decode()  # as an index without texts
        assert max_text_bytes(res) == max_text_bytes(ref) == 0
    return host, dic, res


@pytest.mark.parametrize("ngram,kanji,cross", CONFIGS)
def test_the_resident_index_equals_the_index_of_the_host_columns(ngram, kanji, cross):
    for name, (texts, _) in SMALL.items():
        try:
            out = same_index(mg.Corpus.from_texts(texts), 1, ngram, kanji, cross)
            assert (out is None) == (len(texts) == 0)  # no documents: both paths refuse alike
            same_index(mg.Corpus.from_texts(texts), 1, ngram, kanji, cross, attach=False)
        except AssertionError as e:
            raise AssertionError("corpus %r: %s" % (name, e)) from e


@pytest.mark.parametrize("first", [1, 1000, 2**32 - 400])
def test_first_doc_id(first):
    host, dic, res = same_index(mg.Corpus.from_texts(_sized(300)), first, 2, 0, True)
    d, _ = res.read_postings(int(np.argmax(np.diff(host.offsets.astype(np.int64)))))
    assert int(d.min()) >= first and int(d.max()) <= first + 299


def test_tf_saturation_and_the_overflow_lists():
    texts = ["a" * (2 * k) for k in (254, 255, 256, 299)] + ["aaaa", "b" * 600 + "a" * 512, ""]
    for ngram in (2, 1, 3):
        host, dic, res = same_index(mg.Corpus.from_texts(texts), 1, ngram, 0, True)
        assert (len(dic.tf_overflow_val) > 0) == (ngram < 3)  # ("aaa" fits 199 times into the longest run)
    host, dic, res = same_index(mg.Corpus.from_texts(texts), 1, 2, 0, True)
    _, t = res.read_postings(dic.lookup("aa"))
    assert t.tolist() == [254, 255, 255, 255, 2, 255]
    assert dic.tf_overflow_val.tolist() == [255, 256, 299, 256, 300]


def test_texts_that_do_not_begin_at_offset_zero_and_end_without_padding():
    raw = b"SKIPPED" + b"abc" + "東京".encode() + b"xy\xe6\x9d"
    off = np.asarray([7, 10, 16, 20], dtype=np.uint64)
    data = np.frombuffer(raw, dtype=np.uint8).copy()
    assert len(data) == int(off[-1])
    for ngram, kanji, cross in CONFIGS:
        host, dic, res = same_index(mg.Corpus(data, off), 5, ngram, kanji, cross)
        assert dic.doc_len.tolist() == [3, 2, 2]


class ResidentPair(Pair):
    """gpu_util.Pair whose device index comes from mgx_index_build_device (texts attached by the call); the oracle side is
    made of HOST-built columns."""

    def __init__(self, corpus, host_columns, first_doc_id=1, ngram=2, kanji=0, cross=True, dense_threshold=0.0):
        self.dev = mg.Index(corpus=corpus, first_doc_id=first_doc_id, ngram_size=ngram, kanji_ngram_size=kanji,
                            cross_boundary=cross, dense_threshold=dense_threshold, build_device=0, resident=True)
        assert self.dev._text_attached and self.dev.columns.docids is None
        OracleSide.__init__(self, host_columns, corpus, first_doc_id)


TWO_TILES = 16384 + 77


def two_tile_queries(host, corpus, seed=11):
    """About 40 seeded queries: 1-3 terms, some NOT terms, SORT _score and docid pages in both directions, limit 10, one
    limit 0, docid pages beyond 16384, six with a multi-gram word (text-level BM25) as a term."""
    rng = np.random.default_rng(seed)
    sizes = np.diff(host.offsets.astype(np.int64))
    grams = [host.gram(g).decode() for g in np.argsort(-sizes)[:50] if b" " not in host.gram(g)]
    words = []
    for i in range(0, 400, 7):
        for w in corpus.text(i).split():
            if len(w) >= 4 and w.decode() not in words:
                words.append(w.decode())
    words = words[:6]
    qs = []
    for i in range(32):
        terms = [grams[int(rng.integers(0, len(grams)))] for _ in range(int(rng.integers(1, 4)))]
        nots = [grams[int(rng.integers(0, len(grams)))]] if i % 4 == 0 else []
        qs.append(Query(terms, not_terms=nots, sort_score=i % 2 == 0, descending=i % 3 != 0, limit=10))
    for j, w in enumerate(words):
        terms = [w] + ([grams[j]] if j % 2 else [])
        qs.append(Query(terms, sort_score=True, descending=j % 3 != 0, limit=10))
    qs.append(Query([grams[0]], limit=0))
    # a docid page beyond 16384: the first descending page of the widest gram lies in the second tile; and a page bound
    # past 16384 entries, which no gram of this corpus fills
    qs.append(Query([grams[0]], limit=10, descending=True))
    qs.append(Query([grams[0]], limit=16384 + 6, descending=False))
    qs.append(Query([grams[1]], descending=True, limit=10, offset=3))
    return qs, len(words)


@pytest.fixture(scope="module")
def two_tiles():
    corpus = mg.Corpus.synthetic(TWO_TILES, seed=7)
    return corpus, mg.Columns(corpus, 1, 2, 0, True)


@pytest.mark.parametrize("dense_threshold", [0.0, 2.0], ids=["bitmaps", "lists only"])
def test_two_tiles_the_last_partial(two_tiles, dense_threshold):
    corpus, host = two_tiles
    assert same_index(corpus, 1, 2, 0, True, dense_threshold=dense_threshold, gram_step=3) is not None
    p = ResidentPair(corpus, host, dense_threshold=dense_threshold)
    qs, n_words = two_tile_queries(host, corpus)
    assert len(qs) >= 40 and n_words >= 5
    got = p.check(qs)
    assert sum(1 for r in got if r.total > 0) >= len(qs) // 2  # (the queries are not vacuous)
    assert len(got[-3].docs) == 10 and int(got[-3].docs.min()) > 16384  # the page does lie in the second tile
    assert len(got[-2].docs) == got[-2].total > 8192


def test_one_document_of_70000_code_points_among_300_short_ones():
    rng = np.random.default_rng(9)
    short = _sized(300)
    words = ["abc", "abd", "東京", "都", " ", "xy", "あい"]
    long_doc = "".join(words[int(i)] for i in rng.integers(0, len(words), 40000))[:70000]
    assert len(long_doc) == 70000
    corpus = mg.Corpus.from_texts(short[:150] + [long_doc] + short[150:])
    host, dic, res = same_index(corpus, 1, 2, 1, False)
    assert dic.doc_len[150] == 70000
    assert len(dic.tf_overflow_val) > 1 and int(dic.tf_overflow_val.max()) > 255
    assert max_text_bytes(res) == len(long_doc.encode())
    p = ResidentPair(corpus, host, ngram=2, kanji=1, cross=False)
    got = p.check([Query(["ab"], sort_score=True, limit=10), Query(["都"], sort_score=True, limit=10),
                   Query(["abc"], sort_score=True, limit=10), Query(["xy", "ab"], sort_score=True, descending=False, limit=10)])
    assert 151 in got[0].docs.tolist() and got[0].total > 1


def _raw_call(params, desc, tb, to, first, n_docs):
    L = K.load()
    ch, ih = C.c_void_p(0x1234), C.c_void_p(0x5678)
    rc = L.mgx_index_build_device(C.byref(params), C.byref(desc), tb, to, first, n_docs, C.byref(ch), C.byref(ih))
    return rc, L.mgx_last_error().decode(), ch, ih


def test_refusals_leave_nothing_behind_and_a_good_build_serves_afterwards():
    L = K.load()
    corpus = mg.Corpus.synthetic(500, seed=3)
    tb, to = corpus.text_bytes.ctypes.data, corpus.text_off.ctypes.data

    def params(ngram=2, size=None):
        return K.BuildParams(C.sizeof(K.BuildParams) if size is None else size, K.ABI_VERSION, ngram, 0, 1, 0)

    def desc(device=0, size=None):
        return K.IndexBuildDesc(C.sizeof(K.IndexBuildDesc) if size is None else size, K.ABI_VERSION, device, 0, 0.0, 1, 0)

    bad_off = corpus.text_off.copy()
    bad_off[3] = bad_off[2] - 1
    cases = [(params(ngram=4), desc(), to, NOT_IMPLEMENTED, "3 code points"),
             (params(), desc(device=L.mgx_device_count()), to, INVALID, "bad device"),
             (params(), desc(device=-1), to, INVALID, "bad device"),
             (params(), desc(), bad_off.ctypes.data, INVALID, "text_off descends"),
             (params(), desc(size=8), to, INVALID, "bad struct_size/version"),
             (params(size=4), desc(), to, INVALID, "bad struct_size/version")]
    for p, d, o, code, text in cases:
        rc, msg, ch, ih = _raw_call(p, d, tb, o, 1, corpus.n_docs)
        assert rc == code and text in msg, (rc, msg)
        assert ch.value is None and ih.value is None
    host = mg.Columns(corpus, 1, 2, 0, True)
    pair = ResidentPair(corpus, host)
    sizes = np.diff(host.offsets.astype(np.int64))
    top = [host.gram(g).decode() for g in np.argsort(-sizes)[:6] if b" " not in host.gram(g)]
    got = pair.check([Query([top[0]], sort_score=True, limit=10), Query([top[1], top[2]], limit=10)])
    assert got[0].total > 0

    # mgx_index_create over the dictionary-only view: null posting arrays
    with pytest.raises(K.MgxError) as e:
        mg.DeviceIndex(pair.dev.columns)
    assert e.value.code == INVALID and "null posting arrays" in str(e.value)

    # read_postings: unknown gram; short buffer (*n holds the count)
    idx = pair.dev.device_index
    n = C.c_uint64(7)
    assert L.mgx_index_read_postings(idx._h, host.n_grams, None, None, 0, C.byref(n)) == OUT_OF_RANGE and n.value == 0
    g = int(np.argmax(sizes))
    buf = np.zeros(int(sizes[g]), dtype=np.uint32)
    tf = np.zeros(int(sizes[g]), dtype=np.uint8)
    rc = L.mgx_index_read_postings(idx._h, g, buf.ctypes.data, tf.ctypes.data, int(sizes[g]) - 1, C.byref(n))
    assert rc == OUT_OF_RANGE and n.value == sizes[g] and not buf.any()
    assert L.mgx_index_read_postings(idx._h, g, buf.ctypes.data, None, int(sizes[g]), C.byref(n)) == 0  # doc ids alone
    assert np.array_equal(buf, host.docids[int(host.offsets[g]):int(host.offsets[g + 1])]) and not tf.any()
    # an index made without tf returns doc ids only
    plain = mg.DeviceIndex(host, with_scoring=False)
    d, t = plain.read_postings(g)
    assert np.array_equal(d, buf) and not t.any()


def test_many_threads_build_at_once():
    corpora = [mg.Corpus.from_texts(_sized(200 + 13 * i)) for i in range(6)]
    got, errs = [None] * 6, []

    def work(i):
        try:
            got[i] = mg.DeviceIndex.build_resident(corpora[i], 1 + i, 2, 1, True, 0, 0.0, attach_text=True)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(6)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(6):
        host = mg.Columns(corpora[i], 1 + i, 2, 1, True)
        ref = mg.DeviceIndex(host, 0)
        ref.attach_text(corpora[i])
        dic, res = got[i]
        assert_same_dictionary(host, dic)
        for g in range(host.n_grams):
            lo, hi = int(host.offsets[g]), int(host.offsets[g + 1])
            d, t = res.read_postings(g)
            assert np.array_equal(d, host.docids[lo:hi]) and np.array_equal(t, host.tf[lo:hi])
        assert res.memory_bytes() == ref.memory_bytes()
        _, data, off = read_texts(res, corpora[i].n_docs)
        _, data2, off2 = read_texts(ref, corpora[i].n_docs)
        assert np.array_equal(data, data2) and np.array_equal(off, off2)
