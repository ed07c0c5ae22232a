"""Host-side mirror of the reference's operator interface over the C ABI of libmygram_gpu.so.

Names follow the reference (src/index/index.h, src/index/bm25_scorer.h, src/query/result_sorter.h,
src/server/search_pipeline.h) so the parity tests read like the reference's own tests. Everything that computes on
postings goes through the C ABI to the HIP kernels; what stays on the host is what the reference also does per query
on the host before touching posting lists: normalisation, n-gram generation, dictionary lookup, term ordering and
the empty/unknown-term rules.
"""
import ctypes as C
import math

import numpy as np

from . import _capi
from ._capi import check, load


# --------------------------------------------------------------------------------------------------------------------
# host-side string rules (src/utils/string_utils.cpp)
# --------------------------------------------------------------------------------------------------------------------

def _is_cjk_ideograph(cp):  # string_utils.cpp:441-448 — kana is NOT an ideograph here
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or
            0x2A700 <= cp <= 0x2B73F or 0x2B740 <= cp <= 0x2B81F or 0xF900 <= cp <= 0xFAFF)


def _generate_ngrams(text, n):  # string_utils.cpp:382-423
    if n <= 0 or len(text) < n:
        return []
    return [text[i:i + n] for i in range(len(text) - n + 1)]


def _generate_hybrid_ngrams(text, ascii_n, kanji_n, cross_boundary):  # string_utils.cpp:452-509
    out = []
    if ascii_n <= 0 or kanji_n <= 0:
        return out
    for i, ch in enumerate(text):
        cjk = _is_cjk_ideograph(ord(ch))
        n = kanji_n if cjk else ascii_n
        if i + n > len(text):
            continue
        if not cross_boundary and any(_is_cjk_ideograph(ord(c)) != cjk for c in text[i + 1:i + n]):
            continue
        out.append(text[i:i + n])
    return out


def generate_query_ngrams(normalized, ngram_size, kanji_ngram_size, cross_boundary=True):
    """GenerateQueryNgrams, string_utils.cpp:639-653 (returns str grams, in text order)."""
    if kanji_ngram_size > 0:
        return _generate_hybrid_ngrams(normalized, ngram_size if ngram_size > 0 else 2, kanji_ngram_size,
                                       cross_boundary)
    if ngram_size == 0:
        return _generate_hybrid_ngrams(normalized, 2, 1, True)
    return _generate_ngrams(normalized, ngram_size)


def normalize_text(text, nfkc=True, width="keep", lower=True):
    """mygram::utils::NormalizeText (string_utils.cpp:295-380) — the C++ host layer's implementation, so that the shim
    and this module normalise identically: ICU NFKC -> width -> lower when libmygram_shim.so was built with ICU
    (`normalize_uses_icu()`), otherwise the reference's non-ICU branch (ASCII lower-casing)."""
    from . import _shim_capi
    return _shim_capi.normalize_text(text, nfkc, width, lower)


def normalize_uses_icu():
    from . import _shim_capi
    return _shim_capi.normalize_uses_icu()


def _is_cjk_ideograph_pipeline(cp):
    """IsCjkIdeograph of src/server/search_pipeline.cpp:70-78."""
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F or
            0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF)


def has_uncovered_hybrid_fragment(normalized, ngram_size, kanji_ngram_size, cross_boundary):
    """HasUncoveredHybridFragment (src/server/search_pipeline.cpp:80-136): a term that mixes CJK ideographs with other
    code points and has a code point no query n-gram covers; such a query is post-filtered by exact text (:858-866)."""
    if not normalized or kanji_ngram_size <= 0:
        return False
    ascii_n = ngram_size if ngram_size > 0 else 2
    cps = [ord(c) for c in normalized]
    if len(cps) < 2:
        return False
    flags = [_is_cjk_ideograph_pipeline(c) for c in cps]
    if all(flags) or not any(flags):
        return False
    covered = [False] * len(cps)
    for i, start_is_cjk in enumerate(flags):
        n = kanji_ngram_size if start_is_cjk else ascii_n
        if n <= 0 or i + n > len(cps):
            continue
        if not cross_boundary and any(flags[i + j] != start_is_cjk for j in range(1, n)):
            continue
        for j in range(n):
            covered[i + j] = True
    return not all(covered)


def compute_idf(total_docs, doc_freq):
    """BM25Scorer::ComputeIDF, src/index/bm25_scorer.cpp:14-25 (host side: once per term per query)."""
    if total_docs == 0:
        return 0.0
    df = min(doc_freq, total_docs)
    return math.log((float(total_docs) - float(df) + 0.5) / (float(df) + 0.5) + 1.0)


def _np_view(ptr, count, dtype):
    if not ptr or count == 0:
        return np.zeros(0, dtype=dtype)
    nbytes = int(count) * np.dtype(dtype).itemsize
    buf = (C.c_uint8 * nbytes).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=int(count))


# --------------------------------------------------------------------------------------------------------------------
# corpus / columns / device index
# --------------------------------------------------------------------------------------------------------------------

class Corpus:
    """Normalized document texts as (text_bytes u8, text_off u64[n+1])."""

    def __init__(self, text_bytes, text_off, _owner=None):
        self.text_bytes, self.text_off, self._owner = text_bytes, text_off, _owner
        self.n_docs = len(text_off) - 1

    @classmethod
    def from_texts(cls, texts):
        bs = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in texts]
        off = np.zeros(len(bs) + 1, dtype=np.uint64)
        if bs:
            off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
        data = np.frombuffer(b"".join(bs) + b"\0" * 16, dtype=np.uint8).copy()
        return cls(data, off)

    @classmethod
    def synthetic(cls, n_docs, seed=42, global_first=0, n_threads=0):
        """The deterministic ASCII corpus of include/mygram_tools.h."""
        L = load()
        h = C.c_void_p()
        rc = L.mgxt_corpus_generate(seed, global_first, n_docs, n_threads, C.byref(h))
        if rc != 0:
            raise RuntimeError("mgxt_corpus_generate rc=%d" % rc)
        tb, to, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        L.mgxt_corpus_view(h, C.byref(tb), C.byref(to), C.byref(n))
        off = _np_view(to.value, n.value + 1, np.uint64)
        data = _np_view(tb.value, int(off[-1]) + 16, np.uint8)

        class _Owner:
            def __init__(self, handle):
                self.handle = handle

            def __del__(self):
                load().mgxt_corpus_destroy(self.handle)

        return cls(data, off, _Owner(h))

    def text(self, i):
        return bytes(self.text_bytes[int(self.text_off[i]):int(self.text_off[i + 1])])


class Columns:
    """mgx_columns: gram dictionary + CSR postings + tf + doc_len, built by libmygram_gpu: on the host, or with
    `device=k` on HIP device k (mgx_columns_build_device: the same arrays)."""

    def __init__(self, corpus, first_doc_id=1, ngram_size=2, kanji_ngram_size=0, cross_boundary=True, n_threads=0,
                 device=None):
        L = load()
        self.ngram_size, self.kanji_ngram_size, self.cross_boundary = ngram_size, kanji_ngram_size, cross_boundary
        bp = _capi.BuildParams(C.sizeof(_capi.BuildParams), _capi.ABI_VERSION, ngram_size, kanji_ngram_size,
                               int(cross_boundary), n_threads)
        h = C.c_void_p()
        if device is None:
            check(L.mgx_columns_build(C.byref(bp), corpus.text_bytes.ctypes.data, corpus.text_off.ctypes.data,
                                      first_doc_id, corpus.n_docs, C.byref(h)))
        else:
            check(L.mgx_columns_build_device(C.byref(bp), corpus.text_bytes.ctypes.data, corpus.text_off.ctypes.data,
                                             first_doc_id, corpus.n_docs, int(device), C.byref(h)))
        self._adopt(h)

    @classmethod
    def from_mgix(cls, data, first_doc_id=0, n_docs=0):
        """The reference's index dump (MGIX v1..v4, Index::SaveToStream) -> columns: doc ids only (tf / doc_len stay
        empty — BM25 needs the texts). n_docs=0: the doc range is the span of the ids in the dump."""
        L = load()
        raw = bytes(data)
        h, info = C.c_void_p(), _capi.MgixInfo()
        check(L.mgx_columns_from_mgix(raw, len(raw), first_doc_id, n_docs, C.byref(h), C.byref(info)))
        self = cls.__new__(cls)
        self.ngram_size, self.kanji_ngram_size = int(info.ngram_size), int(info.kanji_ngram_size)
        self.cross_boundary = bool(info.cross_boundary_ngrams)
        self.mgix = {"version": int(info.version), "normalize_nfkc": bool(info.normalize_nfkc),
                     "normalize_width": info.normalize_width.decode(), "normalize_lower": bool(info.normalize_lower),
                     "n_terms": int(info.n_terms)}
        self._adopt(h)
        return self

    def _adopt(self, h):
        L = load()
        self._h = h
        v = _capi.ColumnsView()
        check(L.mgx_columns_view_get(h, C.byref(v)))
        self.view = v
        self.n_grams = int(v.n_grams)
        self.n_postings = int(v.n_postings)
        self.first_doc_id = int(v.first_doc_id)
        self.n_docs = int(v.n_docs)
        self.bm25_doc_count = int(v.bm25_doc_count)
        self.bm25_total_len = int(v.bm25_total_len)
        self.key_off = _np_view(v.key_off, self.n_grams + 1, np.uint32)
        self.key_bytes = _np_view(v.key_bytes, int(self.key_off[-1]) if self.n_grams else 0, np.uint8)
        self.offsets = _np_view(v.offsets, self.n_grams + 1, np.uint64)
        # the dictionary of mgx_index_build_device holds no postings: its view's docids / tf are NULL
        self.docids = _np_view(v.docids, self.n_postings, np.uint32) if v.docids or not self.n_postings else None
        self.tf = _np_view(v.tf, self.n_postings, np.uint8) if v.docids or not self.n_postings else None
        self.doc_len = _np_view(v.doc_len, self.n_docs, np.uint32)
        self.tf_overflow_pos = _np_view(v.tf_overflow_pos, int(v.n_tf_overflow), np.uint64)
        self.tf_overflow_val = _np_view(v.tf_overflow_val, int(v.n_tf_overflow), np.uint32)

    def __del__(self):
        if getattr(self, "_h", None):
            load().mgx_columns_destroy(self._h)
            self._h = None

    def lookup(self, gram):
        """gram (str/bytes) -> gram id, or None when the gram is not in the index."""
        g = gram.encode("utf-8") if isinstance(gram, str) else bytes(gram)
        gid, found = C.c_uint32(), C.c_int()
        check(load().mgx_columns_lookup(self._h, g, len(g), C.byref(gid), C.byref(found)))
        return int(gid.value) if found.value else None

    def gram(self, gid):
        return bytes(self.key_bytes[int(self.key_off[gid]):int(self.key_off[gid + 1])])

    def avg_doc_length(self):  # BM25Stats::avg_doc_length, server_types.h:182-187
        return self.bm25_total_len / self.bm25_doc_count if self.bm25_doc_count else 0.0


class DeviceIndex:
    """mgx_index: one doc-range shard resident in HBM."""

    def __init__(self, columns, device=0, dense_threshold=0.0, with_scoring=True):
        L = load()
        v = columns.view
        d = _capi.IndexDesc(C.sizeof(_capi.IndexDesc), _capi.ABI_VERSION, device, 0, v.first_doc_id, v.n_docs,
                            v.n_grams, v.offsets, v.docids, v.tf if with_scoring else None,
                            v.doc_len if with_scoring else None, dense_threshold,
                            v.tf_overflow_pos if with_scoring else None, v.tf_overflow_val if with_scoring else None,
                            v.n_tf_overflow if with_scoring else 0)
        h = C.c_void_p()
        check(L.mgx_index_create(C.byref(d), C.byref(h)))
        self._adopt(h, device)

    @classmethod
    def build_resident(cls, corpus, first_doc_id=1, ngram_size=2, kanji_ngram_size=0, cross_boundary=True, device=0,
                       dense_threshold=0.0, attach_text=True, tile_shift=0):
        """mgx_index_build_device: (dictionary-only Columns, DeviceIndex) from normalized texts in one call; the postings
        never come to the host."""
        L = load()
        bp = _capi.BuildParams(C.sizeof(_capi.BuildParams), _capi.ABI_VERSION, ngram_size, kanji_ngram_size,
                               int(cross_boundary), 0)
        d = _capi.IndexBuildDesc(C.sizeof(_capi.IndexBuildDesc), _capi.ABI_VERSION, int(device), tile_shift,
                                 dense_threshold, int(bool(attach_text)), 0)
        ch, ih = C.c_void_p(), C.c_void_p()
        check(L.mgx_index_build_device(C.byref(bp), C.byref(d), corpus.text_bytes.ctypes.data, corpus.text_off.ctypes.data,
                                       first_doc_id, corpus.n_docs, C.byref(ch), C.byref(ih)))
        cols = Columns.__new__(Columns)
        cols.ngram_size, cols.kanji_ngram_size, cols.cross_boundary = ngram_size, kanji_ngram_size, cross_boundary
        cols._adopt(ch)
        self = cls.__new__(cls)
        self._adopt(ih, device)
        return cols, self

    def _adopt(self, h, device):
        self._h = h
        self.device = device
        self.facet_values = {}  # column id -> n_values of the columns added with value ids (the lengths of their counts)
        # handles of the batches prepared on this index and not yet destroyed. A batch keeps its index alive, but when
        # both end up in one unreachable reference cycle (a caught exception's traceback holds the frame that holds the
        # batch) the collector runs their __del__ in no particular order, and mgx_batch_destroy reads its index: the one
        # that goes first takes the batches with it. A plain dict, shared with every PreparedBatch.
        self._live_batches = {}

    def __del__(self):
        if getattr(self, "_h", None):
            L = load()
            live = getattr(self, "_live_batches", {})
            for h in list(live):
                L.mgx_batch_destroy(C.c_void_p(h))
            live.clear()
            L.mgx_index_destroy(self._h)
            self._h = None

    def memory_bytes(self):
        n = C.c_uint64()
        check(load().mgx_index_memory_bytes(self._h, C.byref(n)))
        return int(n.value)

    def read_postings(self, gram_id):
        """mgx_index_read_postings: (docids u32, tf u8) of one gram as device memory holds them."""
        L = load()
        n = C.c_uint64()
        check(L.mgx_index_read_postings(self._h, gram_id, None, None, 0, C.byref(n)))
        docids, tf = np.zeros(int(n.value), dtype=np.uint32), np.zeros(int(n.value), dtype=np.uint8)
        if n.value:
            check(L.mgx_index_read_postings(self._h, gram_id, docids.ctypes.data, tf.ctypes.data, n.value, C.byref(n)))
        return docids, tf

    def set_batch_order(self, fifo=True):
        """mgx_index_set_batch_order: batches in flight run first-in-first-out (default) or time-slice the device."""
        check(load().mgx_index_set_batch_order(self._h, 0 if fifo else 1))

    def attach_text(self, corpus):
        """Normalized doc text into HBM (text-level BM25 terms: tf/df by text scan)."""
        check(load().mgx_index_attach_text(self._h, corpus.text_bytes.ctypes.data, corpus.text_off.ctypes.data))

    def attach_original_text(self, originals, kinds, maps=None):
        """mgx_index_attach_original_text, after attach_text: the documents' texts as the user wrote them, by doc slot.
        originals[i]: bytes / str (ignored for kind 0); kinds[i]: _capi.ORIG_*; maps[i]: the (cp_start, cp_end) pairs of
        an ORIG_MAPPED document, one per code point of its normalized text (None otherwise). HIGHLIGHT then builds a
        page entry's snippet from the original of a document that has one."""
        enc = [b"" if o is None else (o.encode("utf-8") if isinstance(o, str) else bytes(o)) for o in originals]
        blob = np.frombuffer(b"".join(enc) + b"\0", dtype=np.uint8)
        off = np.zeros(len(enc) + 1, dtype=np.uint64)
        np.cumsum([len(o) for o in enc], out=off[1:])
        kind = np.ascontiguousarray(kinds, dtype=np.uint8)
        maps = list(maps) if maps is not None else [None] * len(enc)
        if not len(kind) == len(enc) == len(maps):
            raise ValueError("originals, kinds and maps are by doc slot: one entry per document each")
        pairs = [np.asarray(m if m is not None else [], dtype=np.uint32).reshape(-1, 2) for m in maps]
        map_off = np.zeros(len(enc) + 1, dtype=np.uint64)
        np.cumsum([len(m) for m in pairs], out=map_off[1:])
        flat = np.ascontiguousarray(np.concatenate(pairs + [np.zeros((1, 2), np.uint32)]))
        check(load().mgx_index_attach_original_text(self._h, blob.ctypes.data, off.ctypes.data, kind.ctypes.data,
                                                    flat.ctypes.data, map_off.ctypes.data))

    def max_original_text_bytes(self):
        n = C.c_uint32()
        check(load().mgx_index_max_original_text_bytes(self._h, C.byref(n)))
        return int(n.value)

    def add_filter_bitmap(self, docids):
        a = np.ascontiguousarray(docids, dtype=np.uint32)
        out = C.c_uint32()
        check(load().mgx_index_add_filter_bitmap(self._h, a.ctypes.data, len(a), C.byref(out)))
        return int(out.value)

    def add_filter_column(self, values, is_null=None, value_ids=None, n_values=0):
        """mgx_index_add_filter_column: a typed filter column by doc slot. `values`: int64 (signed class), uint64
        (unsigned class / string ranks) or float64 array."""
        v = np.ascontiguousarray(values)
        cls = {"i": 0, "u": 1, "f": 2}[v.dtype.kind]
        v = v.astype({0: np.int64, 1: np.uint64, 2: np.float64}[cls])
        keep = [v]
        nul = None
        if is_null is not None:
            nul = np.ascontiguousarray(is_null, dtype=np.uint8)
            keep.append(nul)
        ids = None
        if value_ids is not None:
            ids = np.ascontiguousarray(value_ids, dtype=np.uint32)
            keep.append(ids)
        d = _capi.FilterColumnDesc(C.sizeof(_capi.FilterColumnDesc), _capi.ABI_VERSION, cls, int(n_values), v.ctypes.data,
                                   nul.ctypes.data if nul is not None else None, ids.ctypes.data if ids is not None else None)
        out = C.c_uint32()
        check(load().mgx_index_add_filter_column(self._h, C.byref(d), C.byref(out)))
        if ids is not None:
            self.facet_values[int(out.value)] = int(n_values)
        return int(out.value)

    def set_primary_keys(self, keys):
        """mgx_index_set_primary_keys: the documents' primary keys by doc slot (bytes or str; None: the document has no
        key and sorts by its doc id). Query(sort_primary_key=True) then pages by them. Calling it again replaces them."""
        enc = [None if k is None else (k if isinstance(k, bytes) else str(k).encode("utf-8")) for k in keys]
        blob = np.frombuffer(b"".join(k or b"" for k in enc) or b"\0", dtype=np.uint8)
        off = np.zeros(len(enc) + 1, dtype=np.uint64)
        np.cumsum([len(k or b"") for k in enc], out=off[1:])
        has = np.asarray([k is not None for k in enc], dtype=np.uint8)
        check(load().mgx_index_set_primary_keys(self._h, blob.ctypes.data, off.ctypes.data,
                                                None if has.all() else has.ctypes.data))

    def attach_primary_key_bytes(self, keys):
        """mgx_index_attach_primary_key_bytes: the documents' raw primary keys by doc slot (bytes or str; None: the
        document has no key), kept resident for Query(documents=...). Calling it again replaces them."""
        enc = [None if k is None else (k if isinstance(k, bytes) else str(k).encode("utf-8")) for k in keys]
        blob = np.frombuffer(b"".join(k or b"" for k in enc) or b"\0", dtype=np.uint8)
        off = np.zeros(len(enc) + 1, dtype=np.uint64)
        np.cumsum([len(k or b"") for k in enc], out=off[1:])
        has = np.asarray([k is not None for k in enc], dtype=np.uint8)
        check(load().mgx_index_attach_primary_key_bytes(self._h, blob.ctypes.data, off.ctypes.data,
                                                        None if has.all() else has.ctypes.data))

    def max_primary_key_bytes(self):
        n = C.c_uint32()
        check(load().mgx_index_max_primary_key_bytes(self._h, C.byref(n)))
        return int(n.value)

    def set_primary_key_shortcut(self, enable=True):
        """mgx_index_set_primary_key_shortcut: off on a main index while a delta index merges with it."""
        check(load().mgx_index_set_primary_key_shortcut(self._h, int(bool(enable))))

    @staticmethod
    def literal_bits(literal):
        """A condition's literal (a python int or float in the column's class) as the ABI's 64-bit pattern."""
        if isinstance(literal, float):
            return int(np.float64(literal).view(np.uint64))
        return int(literal) & 0xFFFFFFFFFFFFFFFF

    def filter_compare(self, column_id, op, literal, eq_epsilon=0.0, null_matches=False, never_matches=False):
        """mgx_index_filter_compare -> filter bitmap id. op: 0 = , 1 != , 2 < , 3 <= , 4 > , 5 >= ; literal: a python int or
        float in the column's class."""
        bits = self.literal_bits(literal)
        out = C.c_uint32()
        check(load().mgx_index_filter_compare(self._h, column_id, op, bits, float(eq_epsilon), int(null_matches),
                                              int(never_matches), C.byref(out)))
        return int(out.value)


# --------------------------------------------------------------------------------------------------------------------
# queries
# --------------------------------------------------------------------------------------------------------------------

class Highlight:
    """query::HighlightOptions (src/query/query_parser.h:158-163): SEARCH ... HIGHLIGHT [TAG <open> <close>]
    [SNIPPET_LEN n] [MAX_FRAGMENTS n]."""

    def __init__(self, open_tag="<em>", close_tag="</em>", snippet_length=100, max_fragments=3):
        self.open_tag, self.close_tag = open_tag, close_tag
        self.snippet_length, self.max_fragments = snippet_length, max_fragments


def build_highlight_terms(normalized_terms):
    """search_pipeline::BuildHighlightTerms (search_pipeline.cpp:712-745) without the synonym branch, over terms that
    are normalized already: skip empty terms, add the whitespace-separated pieces, sort bytewise and dedupe."""
    out = set()
    for t in normalized_terms:
        b = t.encode("utf-8") if isinstance(t, str) else bytes(t)
        if not b:
            continue
        out.add(b)
        for piece in b.split():  # bytes.split(): ' ', \t, \n, \v, \f, \r — what `stream >> piece` skips
            out.add(piece)
    return sorted(out)


class Query:
    """The parts of query::Query (src/query/query_parser.h:207-243) the hot path consumes."""

    def __init__(self, terms=(), not_terms=(), filters=(), sort_score=False, limit=100, offset=0, descending=True,
                 k1=1.2, b=0.75, fuzzy=0, expr=None, universe=None, verify_text=False, highlight=None, conditions=(),
                 sort_column=None, sort_key_bias=0, sort_ranks=False, facet_columns=None, sort_primary_key=False, documents=None):
        """`expr`: boolean tree over term strings instead of the plain AND of `terms` (query::QueryNode):
        "term" | ("and", e, ...) | ("or", e, ...) | ("not", e). `universe` = (first_doc_id, count) of the NOT universe
        (DocumentStore::GetAllDocIds); None = every slot of the index."""
        self.terms, self.not_terms, self.filters = list(terms), list(not_terms), list(filters)
        # conditions: FILTER conditions the batch evaluates itself (mgx_condition), each (column_id, op, literal,
        # eq_epsilon=0.0, null_matches=False, never_matches=False, negate=False) with op and literal as in
        # DeviceIndex.filter_compare — no filter row is registered for them
        self.conditions = list(conditions)
        # sort_column: SORT <filter column> (the id DeviceIndex.add_filter_column returned), `descending` its direction,
        # any limit / offset. sort_ranks: the column holds ranks in a sorted string dictionary; sort_key_bias is then 0
        # when the dictionary holds "" and 1 otherwise (MGX_SORT_COLUMN_RANK)
        if sort_column is not None and sort_score:
            raise ValueError("sort_score and sort_column are two orders: set one of them")
        self.sort_column, self.sort_key_bias, self.sort_ranks = sort_column, sort_key_bias, sort_ranks
        # sort_primary_key: the reference's order without a SORT clause (MGX_SORT_PRIMARY_KEY) over the keys given to
        # DeviceIndex.set_primary_keys, `descending` its direction, any limit / offset
        if sort_primary_key and (sort_score or sort_column is not None):
            raise ValueError("sort_primary_key, sort_score and sort_column are three orders: set one of them")
        self.sort_primary_key = bool(sort_primary_key)
        self.sort_score, self.limit, self.offset, self.descending = sort_score, limit, offset, descending
        self.k1, self.b, self.fuzzy = k1, b, fuzzy
        # verify_text: the caller's memory.verify_text decision (ShouldApplyVerifyText, search_pipeline.cpp:42-66);
        # queries with an uncovered mixed-script fragment are post-filtered by exact text regardless (:858-866)
        self.verify_text = verify_text
        self.expr, self.universe = expr, universe
        # highlight: None / False = off; True = default options; or a Highlight. SearchResult.snippets then holds one
        # snippet per returned doc (GenerateHighlightSnippets on the page, search_handler.cpp:473-482)
        self.highlight = Highlight() if highlight is True else (highlight or None)
        # facet_columns: FACET in a batch (mgx_batch_set_facets): ids DeviceIndex.add_filter_column returned for columns
        # with value ids, at most 8, repeats allowed. SearchResult.facets then holds one count array per column over the
        # query's whole result set; the query returns no page: it runs in doc-id order with limit 0, whatever was given
        self.facet_columns = [int(c) for c in facet_columns] if facet_columns else None
        if self.facet_columns:
            if sort_score or sort_column is not None or sort_primary_key or self.highlight is not None:
                raise ValueError("a faceted query returns counts, not a page: no sort order and no highlight")
            self.limit, self.offset = 0, 0
        # documents: page documents (mgx_batch_set_documents): None = off; a list of ids DeviceIndex.add_filter_column
        # returned (or _capi.DOC_NO_COLUMN), at most 32, repeats allowed, [] = keys only. SearchResult.documents then holds
        # one PageDocument (or None: not found) per returned doc, gathered on the device behind the page
        self.documents = [int(c) for c in documents] if documents is not None else None
        if self.documents is not None and self.facet_columns:
            raise ValueError("a faceted query returns counts, not a page: no documents")
        if expr is not None and not self.terms:
            seen = []

            def walk(e):
                if isinstance(e, str):
                    if e not in seen:
                        seen.append(e)
                else:
                    for c in e[1:]:
                        walk(c)
            walk(expr)
            self.terms = seen


def _set_sort_column(cq, q):
    """q.sort_column -> cq.sort / sort_column / sort_key_bias (offset and reverse are set as for SORT _score)."""
    if q.sort_primary_key:
        cq.sort = _capi.SORT_PRIMARY_KEY
        cq.sort_column = int(q.sort_column or 0)  # (0 unless a test sets them: the library refuses anything else)
        cq.sort_key_bias = int(q.sort_key_bias)
        return
    if q.sort_column is None:
        return
    cq.sort = _capi.SORT_COLUMN_RANK if q.sort_ranks else _capi.SORT_COLUMN
    cq.sort_column = int(q.sort_column)
    cq.sort_key_bias = int(q.sort_key_bias)


def _set_conditions(cq, q, keep):
    """q.conditions -> cq.conditions / n_conditions (mgx_condition array, kept alive in `keep`)."""
    if not q.conditions:
        return
    cc = (_capi.Condition * len(q.conditions))()
    for j, cond in enumerate(q.conditions):
        column_id, op, literal = cond[:3]
        eps, null_matches, never_matches, negate = (tuple(cond[3:]) + (0.0, False, False, False)[len(cond) - 3:])[:4]
        cc[j] = _capi.Condition(int(column_id), int(op), DeviceIndex.literal_bits(literal), float(eps), int(bool(null_matches)),
                                int(bool(never_matches)), int(bool(negate)), 0)
    keep.append(cc)
    cq.conditions = C.cast(cc, C.c_void_p)
    cq.n_conditions = len(q.conditions)


class TermInfo:
    """search_pipeline::SearchTermInfo (src/server/search_pipeline.h:44-55)."""
    __slots__ = ("term", "normalized", "grams", "gram_ids", "estimated_size", "df", "threshold", "fuzzy_ids",
                 "fuzzy_empty")


class PageDocument:
    """One page entry's row (mgx_document_entry): `key` = the primary key's bytes or None, `values` = the requested
    columns' stored 8 bytes as np.uint64, bit c of `null_mask` = values[c] is NULL, `mapped` = the row came from the
    index that names its documents through a doc map (a delta)."""
    __slots__ = ("key", "values", "null_mask", "mapped")

    def __init__(self, key, values, null_mask, mapped):
        self.key, self.values, self.null_mask, self.mapped = key, values, null_mask, mapped


class SearchResult:
    __slots__ = ("total", "docs", "scores", "total_candidates", "after_intersection", "after_not", "after_filters",
                 "empty_term_detected", "term_order", "snippets", "facets", "documents")

    def __init__(self):
        self.total = 0
        self.docs = np.zeros(0, np.uint32)
        self.scores = np.zeros(0, np.float64)
        self.total_candidates = self.after_intersection = self.after_not = self.after_filters = 0
        self.empty_term_detected = False
        self.term_order = []
        self.snippets = []  # bytes per returned doc, when the query asked for highlight
        self.facets = []  # np.uint64 counts per value id, one array per requested facet column
        self.documents = []  # PageDocument (or None) per returned doc, when the query asked for documents


def _take_u32(ptr, n):
    out = np.ctypeslib.as_array(ptr, shape=(max(int(n), 1),))[: int(n)].copy() if n else np.zeros(0, np.uint32)
    load().mgx_free(ptr)
    return out.astype(np.uint32)


def _render_snippet(entry, opts):
    """mgx_highlight_render: tags and "..." around one page entry's record."""
    open_tag = opts.open_tag.encode("utf-8") if isinstance(opts.open_tag, str) else bytes(opts.open_tag)
    close_tag = opts.close_tag.encode("utf-8") if isinstance(opts.close_tag, str) else bytes(opts.close_tag)
    cap = entry.n_bytes + entry.n_spans * (len(open_tag) + len(close_tag)) + 3 * (entry.n_windows + 1)
    buf = C.create_string_buffer(max(cap, 1))
    n = C.c_size_t(0)
    check(load().mgx_highlight_render(C.byref(entry), open_tag, len(open_tag), close_tag, len(close_tag), buf, cap,
                                      C.byref(n)))
    assert n.value <= cap
    return buf.raw[:n.value]


def _page_document(e):
    """mgx_document_entry -> PageDocument, or None for a doc id no index of the batch holds."""
    if not e.flags & _capi.DOC_FOUND:
        return None
    key = C.string_at(e.key, e.key_len) if e.flags & _capi.DOC_HAS_KEY else None
    values = (np.ctypeslib.as_array(e.values, shape=(e.n_columns,)).copy() if e.n_columns else np.zeros(0, np.uint64))
    return PageDocument(key, values, int(e.null_mask), bool(e.flags & _capi.DOC_MAPPED))


class PreparedBatch:
    """mgx_batch: a compiled, device-resident batch of queries that can be executed repeatedly."""

    def __init__(self, index, cqueries, keep, shells, orders, highlights=None, facets=None, documents=None):
        self.index, self._keep, self._shells, self._orders = index, keep, shells, orders
        self.n = len(cqueries)
        self._h = None
        if self.n:
            h = C.c_void_p()
            arr = (_capi.Query * self.n)(*cqueries)
            check(load().mgx_batch_prepare(index.device_index._h, arr, self.n, C.byref(h)))
            self._adopt(h)
        self._set_highlight(highlights)
        self._set_facets(facets)
        self._set_documents(documents)

    def _set_documents(self, documents, max_key_bytes=0):
        """mgx_batch_set_documents: documents[i] = None or the column ids of device query i."""
        self._documents = documents if documents and any(d is not None for d in documents) else None
        if not self._documents or not self._h:
            return
        reqs = (_capi.DocumentRequest * self.n)()
        for i, d in enumerate(self._documents):
            if d is None:
                continue
            ids = (C.c_uint32 * max(len(d), 1))(*d)
            self._keep.append(ids)
            reqs[i] = _capi.DocumentRequest(1, len(d), ids)
        check(load().mgx_batch_set_documents(self._h, reqs, self.n, max_key_bytes))

    def _set_facets(self, facets):
        """mgx_batch_set_facets: facets[i] = None or the column ids of device query i."""
        self._facets = facets if facets and any(f for f in facets) else None
        if not self._facets or not self._h:
            return
        reqs = (_capi.FacetRequest * self.n)()
        for i, f in enumerate(self._facets):
            if not f:
                continue
            ids = (C.c_uint32 * len(f))(*f)
            self._keep.append(ids)
            reqs[i] = _capi.FacetRequest(len(f), 0, ids)
        check(load().mgx_batch_set_facets(self._h, reqs, self.n))

    def _set_highlight(self, highlights):
        """mgx_batch_set_highlight: highlights[i] = None or (Highlight, term list as bytes) of device query i."""
        self._highlights = highlights if highlights and any(h is not None for h in highlights) else None
        if not self._highlights or not self._h:
            return
        reqs = (_capi.HighlightRequest * self.n)()
        for i, h in enumerate(self._highlights):
            if h is None:
                continue
            opts, terms = h
            arr = (C.c_char_p * max(len(terms), 1))(*terms)
            lens = (C.c_uint32 * max(len(terms), 1))(*[len(t) for t in terms])
            self._keep.extend([arr, lens])
            reqs[i] = _capi.HighlightRequest(1, opts.snippet_length, opts.max_fragments, len(terms), arr, lens)
        check(load().mgx_batch_set_highlight(self._h, reqs, self.n, 0))

    def _adopt(self, h):
        """Takes the handle of a batch just prepared and enters it in its index's list of live batches."""
        self._h = h
        self._live = self.index.device_index._live_batches
        self._live[h.value] = True

    def __del__(self):
        if getattr(self, "_h", None):
            if self._live.pop(self._h.value, None):  # (else the index went first and took the batch with it)
                load().mgx_batch_destroy(self._h)
            self._h = None

    def reset(self, cqueries, keep, shells, orders, highlights=None, facets=None, documents=None):
        """mgx_batch_reset: the same batch object (device arenas, pinned result block) for a new set of queries."""
        self._keep, self._shells, self._orders = keep, shells, orders
        self.n = len(cqueries)
        self._exchange = self._df_view = None  # (views of the old contents' device memory)
        arr = (_capi.Query * max(self.n, 1))(*cqueries)
        if self._h is None:
            h = C.c_void_p()
            check(load().mgx_batch_prepare(self.index.device_index._h, arr, self.n, C.byref(h)))
            self._adopt(h)
        else:
            check(load().mgx_batch_reset(self._h, arr, self.n))
        self._set_highlight(highlights)
        self._set_facets(facets)
        self._set_documents(documents)

    def execute(self, stream=None):
        if self._h:
            check(load().mgx_batch_execute(self._h, stream))

    def execute_sharded(self, comm, stream=None):
        """mgx_batch_execute_sharded: execute on a shard of a table — the seeds' best keys of every rank are all-gathered
        (RCCL) and raise each query's pruning bound before the rest of the batch runs; follow with exchange()."""
        if self._h:
            check(load().mgx_batch_execute_sharded(self._h, comm._h, stream))

    def execute_gather(self, world, gather, stream=None):
        """mgx_batch_execute_gather: the same with the caller's all-gather, gather(mine_ptr, all_ptr, nbytes) -> None
        (device pointers; rank r's block goes to all_ptr + r * nbytes)."""
        if not self._h:
            return
        failure = []

        def _cb(_user, mine, all_, nbytes, _stream):
            try:
                gather(mine, all_, nbytes)
                return 0
            except BaseException as e:  # noqa: BLE001 (re-raised below: no exception may cross the C frame)
                failure.append(e)
                return 7
        fn = _capi.GATHER_FN(_cb)
        rc = load().mgx_batch_execute_gather(self._h, world, fn, None, stream)
        if failure:
            raise failure[0]
        check(rc)

    def fetch(self):
        """-> list[SearchResult] in the order the queries were given (host-resolved queries included)."""
        v = _capi.ResultView()
        hv = _capi.HighlightView()
        if self._h:
            check(load().mgx_batch_fetch(self._h, C.byref(v)))
            if self._highlights:
                check(load().mgx_batch_fetch_highlight(self._h, C.byref(hv)))
        counts_of = {}  # device query -> its count arrays, in request order
        if self._h and self._facets:
            fv = _capi.FacetView()
            check(load().mgx_batch_fetch_facets(self._h, C.byref(fv)))
            for j in range(fv.n_entries):
                e = fv.entries[j]
                counts_of.setdefault(e.query, []).append(
                    np.ctypeslib.as_array(e.counts, shape=(e.n_values,)).copy() if e.n_values else np.zeros(0, np.uint64))
        dv = _capi.DocumentView()
        if self._h and self._documents:
            check(load().mgx_batch_fetch_documents(self._h, C.byref(dv)))
        out = []
        k = 0
        for qi, shell in enumerate(self._shells):
            if shell is not None:  # resolved on the host (empty / unknown term): never reached the device
                out.append(shell)
                continue
            r = v.queries[k]
            k += 1
            s = SearchResult()
            s.term_order = self._orders[qi]
            s.total = int(r.total)
            s.total_candidates, s.after_intersection = int(r.total_candidates), int(r.after_intersection)
            s.after_not, s.after_filters = int(r.after_not), int(r.after_filters)
            if r.n_docs:
                s.docs = np.ctypeslib.as_array(v.docs, shape=(r.docs_begin + r.n_docs,))[r.docs_begin:].copy()
                s.scores = np.ctypeslib.as_array(v.scores, shape=(r.docs_begin + r.n_docs,))[r.docs_begin:].copy()
            if self._highlights and self._highlights[k - 1] is not None:
                opts = self._highlights[k - 1][0]
                s.snippets = [_render_snippet(hv.entries[r.docs_begin + j], opts) for j in range(r.n_docs)]
            s.facets = counts_of.get(k - 1, [])
            if self._documents and self._documents[k - 1] is not None:
                s.documents = [_page_document(dv.entries[r.docs_begin + j]) for j in range(r.n_docs)]
            out.append(s)
        return out

    def kernel_time_ms(self):
        ms, n = C.c_double(), C.c_uint32()
        check(load().mgx_batch_kernel_time_ms(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def algorithmic_bytes(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(load().mgx_batch_algorithmic_bytes(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def fetch_raw(self):
        """mgx_batch_fetch without building Python objects (the timed path of bench.py)."""
        v = _capi.ResultView()
        check(load().mgx_batch_fetch(self._h, C.byref(v)))
        return v

    def exchange_df(self, comm, stream=None):
        """mgx_batch_exchange_df: table-wide df of the text-level terms (df pass + RCCL all-reduce); before execute."""
        check(load().mgx_batch_exchange_df(self._h, comm._h, stream))

    def exchange(self, comm, stream=None):
        """mgx_batch_exchange: RCCL all-gather of every shard's top-k + merge; after execute, same stream."""
        check(load().mgx_batch_exchange(self._h, comm._h, stream))

    def count_df(self, stream=None):
        """df pass of the text-level terms only (sharded tables reduce the counts before execute)."""
        check(load().mgx_batch_count_df(self._h, stream))

    def df_buffer(self):
        """-> (device pointer of the u64 df counts, number of text-level terms)."""
        p, n = C.c_void_p(), C.c_uint32()
        check(load().mgx_batch_df_buffer(self._h, C.byref(p), C.byref(n)))
        return p.value, int(n.value)

    def topk_stride(self):
        s = C.c_uint32()
        check(load().mgx_batch_export_topk(self._h, None, None, C.byref(s), None))
        return int(s.value)

    def export_topk(self, blob64_ptr, blob32_ptr, stream=None):
        s = C.c_uint32()
        check(load().mgx_batch_export_topk(self._h, blob64_ptr, blob32_ptr, C.byref(s), stream))
        return int(s.value)

    def export_buffer(self):
        """-> (device pointer, bytes, byte offset of the 32-bit part) of the library-owned exchange blob, or
        (None, 0, 0) when the batch has none (docid-ordered pages export by copy)."""
        p, nb, off = C.c_void_p(), C.c_uint64(), C.c_uint64()
        check(load().mgx_batch_export_buffer(self._h, C.byref(p), C.byref(nb), C.byref(off)))
        return p.value, int(nb.value), int(off.value)

    def merge_shards(self, n_shards, blob64_ptr, blob32_ptr, stream=None, pitch64=0, pitch32=0):
        check(load().mgx_batch_merge_shards(self._h, n_shards, blob64_ptr, pitch64, blob32_ptr, pitch32, stream))


class Index:
    """Read side of mygramdb::index::Index (src/index/index.h:46-300) over one device shard.

    `total_docs` / `avg_doc_length` are the table's BM25Stats (global over all shards when sharded)."""

    def __init__(self, corpus=None, texts=None, first_doc_id=1, ngram_size=2, kanji_ngram_size=0, cross_boundary=True,
                 device=0, dense_threshold=0.0, total_docs=None, avg_doc_length=None, global_posting_sizes=None,
                 n_threads=0, normalize_nfkc=True, normalize_width="keep", normalize_lower=True, build_device=None,
                 resident=False):
        if corpus is None:
            corpus = Corpus.from_texts(texts if texts is not None else [])
        self.ngram_size = ngram_size
        # the Index object keeps kanji = ngram when 0 (index.cpp:31); query n-grams use the table config value
        self.kanji_ngram_size = kanji_ngram_size
        self.cross_boundary = cross_boundary
        # index.h:58-60: how QUERY terms are normalised; document texts arrive normalised (as Index::AddDocument's do)
        self.normalize_nfkc, self.normalize_width, self.normalize_lower = normalize_nfkc, normalize_width, normalize_lower
        if resident:
            # mgx_index_build_device on `build_device`: `columns` is the dictionary (docids / tf None), the texts are attached
            if build_device is None or build_device != device:
                raise ValueError("resident=True builds on the device that serves: build_device must equal device")
            self.columns, self.device_index = DeviceIndex.build_resident(
                corpus, first_doc_id, ngram_size, kanji_ngram_size, cross_boundary, device, dense_threshold, attach_text=True)
        else:
            self.columns = Columns(corpus, first_doc_id, ngram_size, kanji_ngram_size, cross_boundary, n_threads,
                                   device=build_device)
            self.device_index = DeviceIndex(self.columns, device, dense_threshold)
        self.corpus = corpus        # the DocumentStore's normalized texts
        self._text_attached = bool(resident)
        self.total_docs = self.columns.bm25_doc_count if total_docs is None else total_docs
        self.avg_doc_length = self.columns.avg_doc_length() if avg_doc_length is None else avg_doc_length
        # df source: posting sizes of the WHOLE table (a shard passes the global sizes so idf is identical everywhere)
        self._global_sizes = global_posting_sizes
        self._global_dict = None  # sharded tables: {gram bytes: table-wide posting size} over every shard's dictionary

    @classmethod
    def from_mgix(cls, data, device=0, dense_threshold=0.0, first_doc_id=0, n_docs=0):
        """Index::LoadFromData (src/index/index_serialization.cpp:260-420): an index over the postings of a reference
        dump, configured by the dump's own header. It holds doc ids only, so it answers everything but SORT _score."""
        self = cls.__new__(cls)
        cols = Columns.from_mgix(data, first_doc_id, n_docs)
        self.ngram_size, self.kanji_ngram_size, self.cross_boundary = cols.ngram_size, cols.kanji_ngram_size, cols.cross_boundary
        self.normalize_nfkc, self.normalize_width = cols.mgix["normalize_nfkc"], cols.mgix["normalize_width"]
        self.normalize_lower = cols.mgix["normalize_lower"]
        self.columns = cols
        self.device_index = DeviceIndex(cols, device, dense_threshold, with_scoring=False)
        self.corpus = None
        self._text_attached = False
        self.total_docs, self.avg_doc_length = 0, 0.0
        self._global_sizes = None
        self._global_dict = None
        return self

    @classmethod
    def from_dump(cls, data, table=None, device=0, dense_threshold=0.0):
        """A table of a reference dump (DUMP SAVE, "MGDB" v2: src/storage/dump_format_v2.cpp) as a ranking index: columns
        built from the dump's stored texts (and checked against its own MGIX index), texts attached, filter columns kept in
        `dump_filter_columns` [(name, value type 1..12, values, is_null, strings)]; `exists` marks the doc ids the store
        holds; `dump_primary_keys` [bytes | None by slot] are the documents' primary keys, given to the device index."""
        L = load()
        raw = bytes(data)
        h = C.c_void_p()
        check(L.mgx_dump_open(raw, len(raw), table.encode() if table else None, C.byref(h)))
        try:
            v = _capi.DumpView()
            check(L.mgx_dump_view_get(h, C.byref(v)))
            n = int(v.n_docs)
            info = v.index_info
            self = cls.__new__(cls)
            self.table_name = v.table_name.decode()
            self.ngram_size, self.kanji_ngram_size = int(info.ngram_size), int(info.kanji_ngram_size)
            self.cross_boundary = bool(info.cross_boundary_ngrams)
            self.normalize_nfkc, self.normalize_lower = bool(info.normalize_nfkc), bool(info.normalize_lower)
            self.normalize_width = info.normalize_width.decode()
            self.exists = np.ctypeslib.as_array(C.cast(v.exists, C.POINTER(C.c_uint8)), shape=(max(n, 1),))[:n].copy()
            toff = np.ctypeslib.as_array(C.cast(v.text_off, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
            tb = np.ctypeslib.as_array(C.cast(v.text_bytes, C.POINTER(C.c_uint8)), shape=(int(toff[-1]) + 16,)).copy()
            self.corpus = Corpus(tb, toff)
            self.dump_filter_columns = []
            for i in range(int(v.n_filter_columns)):
                fc = _capi.DumpFilterColumn()
                check(L.mgx_dump_filter_column_get(h, i, C.byref(fc)))
                vals = np.ctypeslib.as_array(C.cast(fc.values, C.POINTER(C.c_uint64)), shape=(max(n, 1),))[:n].copy()
                nul = np.ctypeslib.as_array(C.cast(fc.is_null, C.POINTER(C.c_uint8)), shape=(max(n, 1),))[:n].copy()
                strings = None
                if fc.value_type == 11:
                    so = np.ctypeslib.as_array(C.cast(fc.string_off, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
                    sb = np.ctypeslib.as_array(C.cast(fc.string_bytes, C.POINTER(C.c_uint8)), shape=(int(so[-1]) + 1,)).tobytes()
                    strings = [sb[int(so[k]): int(so[k + 1])] for k in range(n)]
                self.dump_filter_columns.append((fc.name.decode(), int(fc.value_type), vals, nul.astype(bool), strings))
            pkb, pko = C.c_void_p(), C.c_void_p()
            check(L.mgx_dump_primary_keys_get(h, C.byref(pkb), C.byref(pko)))
            po = np.ctypeslib.as_array(C.cast(pko, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
            pb = np.ctypeslib.as_array(C.cast(pkb, C.POINTER(C.c_uint8)), shape=(int(po[-1]) + 1,)).tobytes()
            self.dump_primary_keys = [pb[int(po[k]): int(po[k + 1])] if self.exists[k] else None for k in range(n)]
            check(L.mgx_dump_original_texts_get(h, C.byref(pkb), C.byref(pko)))
            oo = np.ctypeslib.as_array(C.cast(pko, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
            ob = np.ctypeslib.as_array(C.cast(pkb, C.POINTER(C.c_uint8)), shape=(int(oo[-1]) + 1,)).tobytes()
            # the store's original texts (None: it holds none for the slot); attach_original_text takes them with their maps
            self.dump_original_texts = [ob[int(oo[k]): int(oo[k + 1])] if oo[k + 1] > oo[k] else None for k in range(n)]
            ch = C.c_void_p()
            check(L.mgx_dump_take_columns(h, C.byref(ch)))
            cols = Columns.__new__(Columns)
            cols.ngram_size, cols.kanji_ngram_size, cols.cross_boundary = self.ngram_size, self.kanji_ngram_size, self.cross_boundary
            cols._adopt(ch)
            has_texts = bool(v.has_texts)
        finally:
            L.mgx_dump_destroy(h)
        self.columns = cols
        self.device_index = DeviceIndex(cols, device, dense_threshold, with_scoring=has_texts)
        if n:
            self.device_index.set_primary_keys(self.dump_primary_keys)  # Query(sort_primary_key=True) pages by them
        self._text_attached = False
        self.total_docs = cols.bm25_doc_count if has_texts else 0
        self.avg_doc_length = cols.avg_doc_length() if has_texts else 0.0
        self._global_sizes = None
        self._global_dict = None
        return self

    # ---- dictionary -------------------------------------------------------------------------------------------
    def posting_size(self, gram):
        if self._global_dict is not None:
            g = gram.encode("utf-8") if isinstance(gram, str) else bytes(gram)
            return int(self._global_dict.get(g, 0))
        gid = self.columns.lookup(gram)
        if gid is None:
            return 0
        if self._global_sizes is not None:
            return int(self._global_sizes[gid])
        return int(self.columns.offsets[gid + 1] - self.columns.offsets[gid])

    estimate_posting_size = posting_size  # index.cpp:756-759

    def ensure_text(self):
        """Text-level BM25 terms scan doc text on the device: upload it on first use."""
        if not self._text_attached:
            self.device_index.attach_text(self.corpus)
            self._text_attached = True

    def attach_original_text(self, originals, kinds, maps=None):
        """The documents' original texts (DeviceIndex.attach_original_text): SearchResult.snippets then come from the
        original of every page entry whose document has one, as Highlighter::GenerateOriginal builds them."""
        self.ensure_text()
        self.device_index.attach_original_text(originals, kinds, maps)

    def _ids(self, terms):
        """gram strings -> (ids of known grams, saw_unknown)."""
        ids, unknown = [], False
        for t in terms:
            gid = self.columns.lookup(t)
            if gid is None:
                unknown = True
            else:
                ids.append(gid)
        return ids, unknown

    # ---- Index::Search* ---------------------------------------------------------------------------------------
    def search_and(self, terms, limit=0, reverse=False):
        """Index::SearchAnd, index.cpp:199-368."""
        if len(terms) == 0:
            return np.zeros(0, np.uint32)  # :203
        ids, unknown = self._ids(terms)
        if unknown:
            return np.zeros(0, np.uint32)  # :211-215
        a = np.asarray(ids, dtype=np.uint32)
        p, n = C.POINTER(C.c_uint32)(), C.c_uint64()
        check(load().mgx_and(self.device_index._h, a.ctypes.data, len(a), limit, int(reverse), C.byref(p),
                             C.byref(n)))
        return _take_u32(p, n.value)

    def search_or(self, terms):
        """Index::SearchOr, index.cpp:418-448 (unknown terms skipped)."""
        ids, _ = self._ids(terms)
        if not ids:
            return np.zeros(0, np.uint32)
        a = np.asarray(sorted(set(ids)), dtype=np.uint32)
        p, n = C.POINTER(C.c_uint32)(), C.c_uint64()
        check(load().mgx_or(self.device_index._h, a.ctypes.data, len(a), C.byref(p), C.byref(n)))
        return _take_u32(p, n.value)

    def search_not(self, all_docs, terms):
        """Index::SearchNot, index.cpp:450-486."""
        docs = np.ascontiguousarray(all_docs, dtype=np.uint32)
        ids, _ = self._ids(terms)
        if len(terms) == 0 or not ids:
            return docs.copy()  # :451-453 / nothing to exclude
        a = np.asarray(sorted(set(ids)), dtype=np.uint32)
        p, n = C.POINTER(C.c_uint32)(), C.c_uint64()
        check(load().mgx_not(self.device_index._h, docs.ctypes.data, len(docs), a.ctypes.data, len(a), C.byref(p),
                             C.byref(n)))
        return _take_u32(p, n.value)

    def search_by_threshold(self, terms, threshold):
        """Index::SearchByThreshold, index.cpp:488-578."""
        if len(terms) == 0 or threshold == 0:
            return np.zeros(0, np.uint32)
        uniq = sorted(set(t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in terms))  # :496-497
        if threshold > len(uniq):
            return np.zeros(0, np.uint32)
        if threshold == len(uniq):
            return self.search_and(uniq)  # :504-506
        ids, _ = self._ids(uniq)  # missing grams do not count (:512-518)
        if len(ids) < threshold:
            return np.zeros(0, np.uint32)
        a = np.asarray(ids, dtype=np.uint32)
        p, n = C.POINTER(C.c_uint32)(), C.c_uint64()
        check(load().mgx_threshold(self.device_index._h, a.ctypes.data, len(a), threshold, C.byref(p), C.byref(n)))
        return _take_u32(p, n.value)

    def filter_by_ngrams(self, candidates, terms):
        """Index::FilterByNgrams, index.cpp:370-416 (caller order and duplicates kept)."""
        cand = np.ascontiguousarray(candidates, dtype=np.uint32)
        if len(cand) == 0:
            return np.zeros(0, np.uint32)
        if len(terms) == 0:
            return cand.copy()
        ids, unknown = self._ids(terms)
        if unknown:
            return np.zeros(0, np.uint32)
        a = np.asarray(ids, dtype=np.uint32)
        p, n = C.POINTER(C.c_uint32)(), C.c_uint64()
        check(load().mgx_retain(self.device_index._h, cand.ctypes.data, len(cand), a.ctypes.data, len(a),
                                C.byref(p), C.byref(n)))
        return _take_u32(p, n.value)

    # ---- BM25Scorer / ResultSorter ----------------------------------------------------------------------------
    def score_documents(self, candidates, terms, dfs, total_docs, avg_doc_length, k1=1.2, b=0.75):
        """BM25Scorer::ScoreDocuments (bm25_scorer.cpp:47-99): tf columns when every term is exactly one n-gram, the
        doc text otherwise."""
        if len(terms) != len(dfs):
            raise _capi.MgxError(2, "BM25 search_terms and term_doc_freqs must have identical lengths")
        cand = np.ascontiguousarray(candidates, dtype=np.uint32)
        tis = [self.term_info(t) for t in terms]
        if any(len(ti.grams) != 1 or ti.grams[0] != ti.normalized.encode("utf-8") for ti in tis):
            # some term is not one n-gram: count every term in the doc text, like the reference
            self.ensure_text()
            tb = [ti.normalized.encode("utf-8") for ti in tis]
            off = np.zeros(len(tb) + 1, dtype=np.uint32)
            off[1:] = np.cumsum([len(x) for x in tb])
            data = np.frombuffer(b"".join(tb) + b"\0" * 16, dtype=np.uint8).copy()
            idfs = np.asarray([compute_idf(total_docs, d) for d in dfs], dtype=np.float64)
            out = np.zeros(max(len(cand), 1), dtype=np.float64)
            check(load().mgx_score_documents_text(self.device_index._h, cand.ctypes.data, len(cand), data.ctypes.data,
                                                  off.ctypes.data, idfs.ctypes.data, len(tb), float(avg_doc_length),
                                                  float(k1), float(b), out.ctypes.data))
            return out[: len(cand)]
        gids = []
        for t in terms:
            gid = self.columns.lookup(t)
            gids.append(0xFFFFFFFF if gid is None else gid)
        g = np.asarray(gids, dtype=np.uint32)
        idfs = np.asarray([compute_idf(total_docs, d) for d in dfs], dtype=np.float64)
        out = np.zeros(max(len(cand), 1), dtype=np.float64)
        check(load().mgx_score_documents(self.device_index._h, cand.ctypes.data, len(cand), g.ctypes.data,
                                         idfs.ctypes.data, len(g), float(avg_doc_length), float(k1), float(b),
                                         out.ctypes.data))
        return out[: len(cand)]

    def sort_by_score(self, results, scores, descending=True, limit=0, offset=0):
        """ResultSorter::SortByScore, result_sorter.cpp:661-716."""
        r = np.ascontiguousarray(results, dtype=np.uint32)
        s = np.ascontiguousarray(scores, dtype=np.float64)
        p, n = C.POINTER(C.c_uint32)(), C.c_uint64()
        check(load().mgx_sort_by_score(self.device_index._h, r.ctypes.data, s.ctypes.data, len(r), int(descending),
                                       limit, offset, C.byref(p), C.byref(n)))
        return _take_u32(p, n.value)

    # ---- search_pipeline ---------------------------------------------------------------------------------------
    def term_info(self, term, fuzzy=0):
        """GenerateTermInfos for one term (search_pipeline.cpp:569-603); df from posting sizes (single-gram terms)."""
        ti = TermInfo()
        ti.term = term
        ti.normalized = normalize_text(term, self.normalize_nfkc, self.normalize_width, self.normalize_lower)
        grams = generate_query_ngrams(ti.normalized, self.ngram_size, self.kanji_ngram_size, self.cross_boundary)
        ti.grams = sorted(set(g.encode("utf-8") for g in grams))  # DeduplicateSorted: bytewise
        ti.gram_ids = []
        size = None  # SIZE_MAX
        for g in ti.grams:
            ps = self.posting_size(g)
            if ps > 0:
                size = ps if size is None else min(size, ps)
                gid = self.columns.lookup(g)  # None: another shard has the gram, this one holds no posting for it
                ti.gram_ids.append(_capi.GRAM_ABSENT if gid is None else gid)
            else:
                size = 0
                break
        ti.estimated_size = size
        # a term that IS its single n-gram scores from the gram's tf column (df = posting count); any other term
        # needs the text: tf by CountTermOccurrences, df by PopulateTermDocumentFrequency (search_pipeline.cpp:542-565)
        ti.df = size if (len(ti.grams) == 1 and size and ti.grams[0] == ti.normalized.encode("utf-8")) else None
        ti.threshold = 0
        if fuzzy and ti.grams:
            # ExecuteWithFuzzy, search_pipeline.cpp:1685-1703: theta = |grams| - d * n_eff, at least 1; n_eff = the kanji
            # size when more than half of the grams are at most 3 bytes long
            n_eff = self.ngram_size if self.ngram_size > 0 else 2
            if self.kanji_ngram_size > 0 and sum(1 for g in ti.grams if len(g) <= 3) > len(ti.grams) // 2:
                n_eff = self.kanji_ngram_size
            drop = fuzzy * n_eff
            ti.threshold = len(ti.grams) - drop if len(ti.grams) > drop else 1
            # Index::SearchByThreshold (index.cpp:488-578) over the DISTINCT grams: theta == all of them -> SearchAnd
            # (an unknown gram empties it); otherwise unknown grams are skipped and fewer than theta known ones -> {}
            known = [g for g in ti.grams if self.posting_size(g) > 0]
            ti.fuzzy_ids = [(_capi.GRAM_ABSENT if self.columns.lookup(g) is None else self.columns.lookup(g)) for g in known]
            if ti.threshold == len(ti.grams):
                ti.fuzzy_empty = len(known) != len(ti.grams)
            else:
                ti.fuzzy_empty = len(known) < ti.threshold
        return ti

    def prepare(self, queries, into=None):
        """Compiles queries the way ExecuteFullPipeline's regular branch plans them (search_pipeline.cpp:2002-2030,
        Execute :795-869) and uploads them as one batch. `into`: a PreparedBatch to re-use (mgx_batch_reset)."""
        cqueries, keep, shells, orders, highlights = [], [], [], [], []
        for q in queries:
            tis = [self.term_info(t, q.fuzzy) for t in q.terms]
            hl = None
            if q.highlight is not None:
                # the reference's all_search_terms: search_text + and_terms; the CollectAstScoringTerms leaves of an
                # expression (search_pipeline.cpp:1812-1816, 1848-1853); a FUZZY query's terms as given
                self.ensure_text()
                by_term = {t.term: t.normalized for t in tis}
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
                hl = (q.highlight, build_highlight_terms([by_term[t] for t in names]))
            if q.fuzzy and q.expr is None:
                # ExecuteWithFuzzy (search_pipeline.cpp:1659-1744): terms in the order given (no size sort); a term
                # without n-grams ends the query; per term "at least theta of its known grams", AND across terms
                order = list(range(len(tis)))
                shell = SearchResult()
                shell.term_order = order
                orders.append(order)
                if not tis or any(not t.grams for t in tis):
                    shell.empty_term_detected = True
                    shells.append(shell)
                    continue
                cterms = (_capi.Term * len(tis))()
                scored = []
                if q.verify_text:
                    self.ensure_text()  # PostFilterByFuzzyText (search_pipeline.cpp:1746-1755) reads the stored texts
                for j, t in enumerate(tis):
                    ids_list = [_capi.GRAM_ABSENT] if (t.fuzzy_empty or not t.fuzzy_ids) else t.fuzzy_ids
                    ids = np.asarray(ids_list, dtype=np.uint32)
                    keep.append(ids)
                    thr = 0 if (t.fuzzy_empty or t.threshold >= len(ids)) else t.threshold
                    idf, text_ptr, text_len = 0.0, None, 0
                    # SORT _score: the EXACT term is scored (search_handler.cpp:428-456 over GenerateTermInfos' infos,
                    # search_pipeline.cpp:1895-1899). A term with an unknown n-gram occurs in no text: tf = df = 0, it
                    # adds nothing and is left out of the scored list.
                    if q.sort_score and len(t.fuzzy_ids) == len(t.grams) and not t.fuzzy_empty:
                        scored.append(j)
                        if t.df is None:  # text-level term
                            self.ensure_text()
                            tb = np.frombuffer(t.normalized.encode("utf-8"), dtype=np.uint8).copy()
                            keep.append(tb)
                            text_ptr, text_len = tb.ctypes.data, len(tb)
                        else:
                            idf = compute_idf(self.total_docs, t.df)
                    if q.verify_text and text_ptr is None:
                        # the filter checks every normalized term (a scored single-gram term then takes tf from the
                        # text, which equals its gram's tf column, and df from the df pass, which equals t.df)
                        tb = np.frombuffer(t.normalized.encode("utf-8"), dtype=np.uint8).copy()
                        keep.append(tb)
                        text_ptr, text_len = tb.ctypes.data, len(tb)
                    cterms[j] = _capi.Term(ids.ctypes.data, len(ids), thr, idf, text_ptr, text_len)
                nts = []
                for nt in q.not_terms:
                    ti = self.term_info(nt)
                    if not ti.grams:
                        raise _capi.MgxError(4, "NOT term shorter than one n-gram is not on the device path")
                    if ti.estimated_size == 0:
                        continue
                    nts.append(ti)
                cnots = (_capi.Term * max(len(nts), 1))()
                for j, t in enumerate(nts):
                    ids = np.asarray(t.gram_ids, dtype=np.uint32)
                    keep.append(ids)
                    cnots[j] = _capi.Term(ids.ctypes.data, len(ids), 0, 0.0, None, 0)
                cf = (_capi.Filter * max(len(q.filters), 1))()
                for j, (bid, negate) in enumerate(q.filters):
                    cf[j] = _capi.Filter(bid, int(negate))
                keep.extend([cterms, cnots, cf])
                cq = _capi.Query(C.cast(cterms, C.c_void_p), len(tis), C.cast(cnots, C.c_void_p), len(nts),
                                 C.cast(cf, C.c_void_p), len(q.filters),
                                 _capi.SORT_SCORE if q.sort_score else _capi.SORT_DOCID, q.limit, q.offset,
                                 int(q.descending), 0, q.k1, q.b, self.total_docs, self.avg_doc_length)
                _set_conditions(cq, q, keep)
                _set_sort_column(cq, q)
                if q.verify_text:
                    cq.fuzzy_verify_distance = q.fuzzy
                if q.sort_score:
                    sc = np.asarray(scored, dtype=np.uint32)
                    keep.append(sc)
                    cq.score_terms = sc.ctypes.data if len(sc) else C.cast(cterms, C.c_void_p).value  # (non-NULL: "none")
                    cq.n_score_terms = len(sc)
                cqueries.append(cq)
                highlights.append(hl)
                shells.append(None)
                continue
            if q.expr is not None:
                order = list(range(len(tis)))  # expression leaves keep their first-use order
            else:
                order = sorted(range(len(tis)), key=lambda i: (float("inf") if tis[i].estimated_size is None
                                                               else tis[i].estimated_size))  # stable, :2012-2014
            tis = [tis[i] for i in order]
            shell = SearchResult()
            shell.term_order = order
            orders.append(order)
            expr_tokens = None
            # verify_text over an expression (search_pipeline.cpp:1505-1578): the tree is re-evaluated over each
            # candidate's text, so every leaf carries its normalized text (exact_text / fuzzy_verify_distance + expr)
            tree_verify = q.expr is not None and q.verify_text
            if q.expr is not None:
                # ExecuteWithBooleanAst (search_pipeline.cpp:1408-1578): a term with an unknown gram is an empty
                # doc set inside the tree, not the end of the query
                toks = []
                if q.fuzzy:
                    # FUZZY d over an expression: every leaf is fuzzy_term_search (search_pipeline.cpp:1424-1445) — a
                    # leaf without n-grams is the empty set (:1431-1433), any other "at least theta of its known grams"
                    # (Index::SearchByThreshold); the scored terms stay the exact terms
                    def leaf_empty(t):
                        return not t.grams or t.fuzzy_empty or not t.fuzzy_ids
                else:
                    def leaf_empty(t):
                        return t.estimated_size in (0, None)

                def emit(e):
                    if isinstance(e, str):
                        i = q.terms.index(e)
                        # an empty leaf is still evaluated on the text under tree_verify (it matters under a NOT): it
                        # goes as a TERM of the absent gram with its text; only "" is false there as well
                        if leaf_empty(tis[i]) and not (tree_verify and tis[i].normalized):
                            toks.append((_capi.EXPR_EMPTY, 0))
                        else:
                            toks.append((_capi.EXPR_TERM, i))
                        return
                    for c in e[1:]:
                        emit(c)
                    op = {"and": _capi.EXPR_AND, "or": _capi.EXPR_OR, "not": _capi.EXPR_NOT}[e[0]]
                    toks.append((op, len(e) - 1))
                emit(q.expr)
                expr_tokens = (_capi.ExprToken * len(toks))(*[_capi.ExprToken(o, a) for o, a in toks])
                keep.append(expr_tokens)
                # SORT _score over an expression: the TERM leaves that are not under a NOT, in tree order, repeats kept
                # (CollectAstScoringTerms, search_pipeline.cpp:232-254); a leaf with an unknown gram occurs in no text
                # (tf = df = 0) and is left out
                expr_scored = []

                def collect(e, under_not):
                    if isinstance(e, str):
                        i = q.terms.index(e)
                        if not under_not and tis[i].estimated_size not in (0, None):
                            expr_scored.append(i)
                        return
                    for c in e[1:]:
                        collect(c, under_not or e[0] == "not")
                collect(q.expr, False)
                # placeholder grams for EMPTY leaves so that every mgx_term stays well-formed
                for t in tis:
                    if leaf_empty(t):
                        t.gram_ids, t.threshold = [_capi.GRAM_ABSENT if tree_verify else 0], 0
                    elif q.fuzzy:
                        t.gram_ids = t.fuzzy_ids
            elif any(t.estimated_size in (0, None) and (t.grams or not t.normalized) for t in tis):
                shell.empty_term_detected = True  # Execute :804-810
                shells.append(shell)
                continue
            if any(not t.grams for t in tis) and q.expr is not None and (not q.fuzzy or q.sort_score):
                raise _capi.MgxError(4, "a term shorter than one n-gram inside an expression "
                                        "(SearchNormalizedSubstring) is not on the device path")
            exact = q.expr is None and (q.verify_text or any(
                has_uncovered_hybrid_fragment(t.normalized, self.ngram_size, self.kanji_ngram_size, self.cross_boundary)
                for t in tis))
            if exact or tree_verify:
                self.ensure_text()
            cterms = (_capi.Term * len(tis))()
            for j, t in enumerate(tis):
                ids = np.asarray(t.gram_ids, dtype=np.uint32)
                keep.append(ids)
                thr = t.threshold if (q.fuzzy and t.threshold < len(ids)) else 0
                idf, text_ptr, text_len = 0.0, None, 0
                if exact or (tree_verify and t.normalized) or (not t.grams and q.expr is None):
                    # (no grams at all: a term shorter than one n-gram — the device scans the texts for it,
                    # query::SearchNormalizedSubstring, src/query/substring_search.h:24-42)
                    self.ensure_text()
                    tb = np.frombuffer(t.normalized.encode("utf-8"), dtype=np.uint8).copy()
                    keep.append(tb)
                    text_ptr, text_len = tb.ctypes.data, len(tb)
                if q.sort_score:
                    if t.df is None:  # text-level term
                        self.ensure_text()
                        tb = np.frombuffer(t.normalized.encode("utf-8"), dtype=np.uint8).copy()
                        keep.append(tb)
                        text_ptr, text_len = tb.ctypes.data, len(tb)
                    else:
                        idf = compute_idf(self.total_docs, t.df)
                cterms[j] = _capi.Term(ids.ctypes.data if len(ids) else None, len(ids), thr, idf, text_ptr, text_len)
            nts = []
            for nt in q.not_terms:
                ti = self.term_info(nt)
                if not ti.grams:
                    if not ti.normalized:
                        continue  # "" is contained in nothing (SearchNormalizedSubstring returns {})
                    self.ensure_text()
                elif ti.estimated_size == 0:
                    continue  # an unknown gram: the NOT term matches nothing
                nts.append(ti)
            cnots = (_capi.Term * max(len(nts), 1))()
            for j, t in enumerate(nts):
                ids = np.asarray(t.gram_ids, dtype=np.uint32)
                keep.append(ids)
                text_ptr, text_len = None, 0
                if not t.grams:  # substring NOT term
                    tb = np.frombuffer(t.normalized.encode("utf-8"), dtype=np.uint8).copy()
                    keep.append(tb)
                    text_ptr, text_len = tb.ctypes.data, len(tb)
                cnots[j] = _capi.Term(ids.ctypes.data if len(ids) else None, len(ids), 0, 0.0, text_ptr, text_len)
            cf = (_capi.Filter * max(len(q.filters), 1))()
            for j, (bid, negate) in enumerate(q.filters):
                cf[j] = _capi.Filter(bid, int(negate))
            keep.extend([cterms, cnots, cf])
            cq = _capi.Query(C.cast(cterms, C.c_void_p), len(tis), C.cast(cnots, C.c_void_p), len(nts),
                             C.cast(cf, C.c_void_p), len(q.filters),
                             _capi.SORT_SCORE if q.sort_score else _capi.SORT_DOCID, q.limit, q.offset,
                             int(q.descending), 0, q.k1, q.b, self.total_docs, self.avg_doc_length)
            _set_sort_column(cq, q)
            cq.exact_text = int(exact or (tree_verify and not q.fuzzy))
            if tree_verify and q.fuzzy:
                cq.fuzzy_verify_distance = q.fuzzy
            _set_conditions(cq, q, keep)
            if expr_tokens is not None and q.sort_score:
                sc = np.asarray(expr_scored, dtype=np.uint32)
                keep.append(sc)
                cq.score_terms = sc.ctypes.data if len(sc) else C.cast(cterms, C.c_void_p).value  # (non-NULL: "none")
                cq.n_score_terms = len(sc)
            if expr_tokens is not None:
                cq.expr = C.cast(expr_tokens, C.c_void_p)
                cq.n_expr = len(expr_tokens)
                if q.universe is not None:
                    cq.universe_first, cq.universe_count = q.universe
            cqueries.append(cq)
            highlights.append(hl)
            shells.append(None)
        if into == "raw":  # (facet: the compiled C queries themselves)
            return cqueries, keep, shells
        # FACET in a batch: the requests of the device queries; a query resolved on the host counts nothing
        wanted = [getattr(q, "facet_columns", None) for q in queries]
        facets = [w for w, shell in zip(wanted, shells) if shell is None]
        for w, shell in zip(wanted, shells):
            if shell is not None and w:
                known = self.device_index.facet_values
                shell.facets = [np.zeros(known.get(c, 0), np.uint64) for c in w]
        # page documents: the requests of the device queries; a query resolved on the host has no page
        documents = [getattr(q, "documents", None) for q, shell in zip(queries, shells) if shell is None]
        if into is not None:
            into.reset(cqueries, keep, shells, orders, highlights, facets, documents)
            return into
        return PreparedBatch(self, cqueries, keep, shells, orders, highlights, facets, documents)

    def facet_counts(self, query, column_id, n_values):
        """mgx_facet_counts: (matched documents, counts per value id) of the query's whole result set."""
        cqueries, keep, shells = self.prepare([query], into="raw")
        if shells[0] is not None:  # resolved on the host: an empty result
            return 0, np.zeros(n_values, np.uint64)
        counts = np.zeros(max(n_values, 1), np.uint64)
        matched = C.c_uint64()
        check(load().mgx_facet_counts(self.device_index._h, C.byref(cqueries[0]), column_id, counts.ctypes.data,
                                      C.byref(matched)))
        return int(matched.value), counts[:n_values]

    def search_batch(self, queries):
        b = self.prepare(queries)
        b.execute()
        return b.fetch()
