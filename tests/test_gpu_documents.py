"""-m gpu: page documents through the C ABI (engine.Query(documents=[column ids]), DeviceIndex.attach_primary_key_bytes,
SearchResult.documents). Every entry's flags, key bytes, values and null mask are compared with a model that is
independent of the device: the host arrays this test attached, looked up by doc id. Values compare as bits, keys as
bytes: there is no tolerance.

Two batches hold the page shapes between them, because one batch with a highlighted query and a query sorted by a filter
column or by the primary key is a pinned refusal of mgx_batch_set_highlight: the first holds the fused and the deep
SORT _score pages, the doc-id pages both ways, limit 1024, a short page, an empty one, an offset past the total, queries
without a request between the others and a query that is highlighted as well; the second holds the column-sorted and
key-sorted pages beside score and doc-id pages. A third test merges a main index and a delta (mgx_batch_merge_local)."""
import ctypes as C

import numpy as np
import pytest

from pkg import mg

from gpu_util import Pair  # noqa: E402

pytestmark = pytest.mark.gpu
Query = mg.engine.Query
cap = mg._capi
N_DOCS, FIRST = 20_000, 5  # two 16384-doc tiles, the second partial
INVALID_ARGUMENT, OUT_OF_RANGE, NOT_IMPLEMENTED = 2, 3, 4
NO = cap.DOC_NO_COLUMN
I64_MIN, U64_MAX = -(1 << 63), (1 << 64) - 1
NAN_BITS = 0x7FF8_0000_DEAD_BEEF  # a NaN with a payload: compared as bits


def make_keys(n, rng):
    """[bytes | None] by slot: the edges of a 64-lane wave and of a 256-byte row, "007" beside "7", the empty key,
    documents without a key, bytes that are not UTF-8."""
    special = [b"", b"k", b"a" * 63, b"b" * 64, b"c" * 65, b"d" * 255, b"e" * 256, b"f" * 257, b"007", b"7", None,
               b"\xff\xfe\x80\x00\xc3", b"\x00", "é日本".encode()]
    keys = []
    for i in range(n):
        if i % 3 == 0:
            k = special[(i // 3) % len(special)]
            keys.append(k if k is None or len(k) < 60 else k[:-1] + bytes([i % 251]))
        else:
            keys.append(b"pk%d" % rng.integers(0, 10 ** int(rng.integers(1, 12))))
    return keys


def dense_grams(index, k):
    """The k grams of the index with the longest posting lists (no space inside), as strings."""
    c = index.columns
    sizes = np.diff(c.offsets.astype(np.int64))
    order = [g for g in np.argsort(-sizes, kind="stable") if b" " not in c.gram(g)]
    return [c.gram(g).decode() for g in order[:k]]


class Table:
    def __init__(self):
        self.p = Pair(corpus=mg.Corpus.synthetic(N_DOCS, seed=91), first_doc_id=FIRST)
        self.p.dev.ensure_text()
        rng = np.random.default_rng(92)
        di = self.dev_index = self.p.dev.device_index
        self.keys = make_keys(N_DOCS, rng)
        di.attach_primary_key_bytes(self.keys)
        di.set_primary_keys(self.keys)
        n = N_DOCS
        signed = rng.integers(-1000, 1000, n).astype(np.int64)
        signed[::7] = I64_MIN
        signed_null = rng.random(n) < 0.2
        unsigned = rng.integers(0, 1 << 62, n).astype(np.uint64)
        unsigned[::5] = U64_MAX
        f64 = rng.standard_normal(n)
        f64[::4] = -0.0
        f64 = f64.view(np.uint64).copy()
        f64[1::4] = NAN_BITS
        f64_null = rng.random(n) < 0.1
        ranks = rng.integers(0, 300, n).astype(np.uint64)  # ranks in a sorted dictionary of 300 strings
        self.cols = {}  # column id -> (stored 8 bytes as uint64 by slot, is-NULL by slot)
        self.c_signed = di.add_filter_column(signed, signed_null)
        self.cols[self.c_signed] = (signed.view(np.uint64), signed_null)
        self.c_unsigned = di.add_filter_column(unsigned)
        self.cols[self.c_unsigned] = (unsigned, np.zeros(n, bool))
        self.c_f64 = di.add_filter_column(f64.view(np.float64), f64_null)
        self.cols[self.c_f64] = (f64, f64_null)
        self.c_rank = di.add_filter_column(ranks, value_ids=ranks.astype(np.uint32), n_values=300)
        self.cols[self.c_rank] = (ranks, np.zeros(n, bool))
        c = self.p.dev.columns
        sizes = np.diff(c.offsets.astype(np.int64))
        order = [g for g in np.argsort(-sizes, kind="stable") if b" " not in c.gram(g)]
        self.dense = [c.gram(g).decode() for g in order[:4]]
        self.sparse = [c.gram(g).decode() for g in order if 4 < sizes[g] <= 60]
        assert sizes[order[0]] > 3000

    def want(self, doc, columns):
        """(key, values as uint64, null mask) of a doc id from the host arrays."""
        slot = doc - FIRST
        vals, mask = [], 0
        for c, col in enumerate(columns):
            nul = col == NO or bool(self.cols[col][1][slot])
            vals.append(0 if nul else int(self.cols[col][0][slot]))
            mask |= int(nul) << c
        return self.keys[slot], vals, mask

    def check(self, q, g):
        if q.documents is None:
            assert g.documents == []
            return 0
        assert len(g.documents) == len(g.docs)
        for doc, d in zip(g.docs.tolist(), g.documents):
            key, vals, mask = self.want(doc, q.documents)
            assert d is not None and not d.mapped, doc
            assert d.key == key, (doc, d.key, key)
            assert d.values.tolist() == vals and d.null_mask == mask, (doc, q.documents)
        return len(g.docs)


@pytest.fixture(scope="module")
def table():
    return Table()


def raw_view(batch):
    """The mgx_document_view of a fetched batch."""
    dv = cap.DocumentView()
    cap.check(cap.load().mgx_batch_fetch_documents(batch._h, C.byref(dv)))
    return dv


def run_thrice(t, qs):
    """Executes the same batch object twice and once more after mgx_batch_reset; the three results must be equal and
    every entry must match the model. Also: n_entries against the fetched docs, zero entries without a request."""
    dev = t.p.dev
    batch = dev.prepare(qs)
    runs = []
    for step in range(3):
        if step == 2:
            dev.prepare(qs, into=batch)  # mgx_batch_reset: the requests are dropped and attached again
        batch.execute()
        got = batch.fetch()
        dv = raw_view(batch)
        assert dv.n_entries == sum(len(g.docs) for g in got)
        begin = 0
        for q, g in zip(qs, got):  # (entry i belongs to docs[i] of the fetched view: the queries' pages back to back)
            for j in range(len(g.docs)):
                e = dv.entries[begin + j]
                if q.documents is None:
                    assert (e.flags, e.key_len, e.null_mask, e.n_columns) == (0, 0, 0, 0) and not e.key and not e.values
                else:
                    assert e.flags & cap.DOC_FOUND and e.n_columns == len(q.documents)
            begin += len(g.docs)
        checked = sum(t.check(q, g) for q, g in zip(qs, got))
        runs.append([(g.total, g.docs.tolist(), [(d.key, d.values.tolist(), d.null_mask) for d in g.documents]) for g in got])
    assert runs[0] == runs[1] == runs[2]
    plain = dev.search_batch([Query(**{**_kw(q), "documents": None}) for q in qs])
    for g, a in zip(got, plain):  # the pages are those of the same batch without a request
        assert g.total == a.total and g.docs.tolist() == a.docs.tolist()
    return got, checked


def _kw(q):
    return dict(terms=q.terms, not_terms=q.not_terms, filters=q.filters, sort_score=q.sort_score, limit=q.limit,
                offset=q.offset, descending=q.descending, conditions=q.conditions, sort_column=q.sort_column,
                sort_primary_key=q.sort_primary_key, highlight=q.highlight)


def test_score_and_docid_pages_of_one_batch(table):
    t = table
    d, s = t.dense, t.sparse
    every = [t.c_signed, t.c_unsigned, t.c_f64, t.c_rank]
    wide = [every[i % 4] if i % 5 else NO for i in range(32)]  # 32 columns, repeats and absent columns among them
    qs = [
        Query([d[0]], sort_score=True, limit=10, documents=every),                  # 0 fused SORT _score
        Query([d[0]], limit=20),                                                    # 1 no request
        Query([d[0]], limit=50, descending=False, documents=[t.c_signed]),          # 2 doc ids ascending
        Query([d[1]], limit=50, descending=True, documents=[]),                     # 3 reversed, keys only
        Query([d[0]], sort_score=True, offset=1000, limit=100, documents=[t.c_f64, t.c_f64]),  # 4 deep, a column twice
        Query([d[1]], sort_score=True, limit=5),                                    # 5 no request
        Query([d[0]], limit=1024, documents=[NO, t.c_unsigned]),                    # 6 limit 1024, an absent column
        Query([s[0]], limit=100, documents=wide),                                   # 7 shorter than its limit
        Query([d[0]], conditions=[(t.c_signed, 0, 123456)], limit=10, documents=every),        # 8 a total of 0
        Query([d[2]], sort_score=True, limit=10, highlight=True, documents=[t.c_rank]),        # 9 highlighted as well
        Query([s[1]], sort_score=True, offset=5000, limit=10, documents=every),     # 10 an offset past the total
        Query([d[0]], limit=0),                                                     # 11 no request, unbounded
        Query([d[0]], sort_score=True, limit=1024, descending=False, documents=[t.c_signed, NO]),  # 12 ascending scores
    ]
    got, checked = run_thrice(t, qs)
    assert len(got[0].docs) == 10 and len(got[4].docs) == 100 and len(got[6].docs) == 1024 and len(got[12].docs) == 1024
    assert 0 < len(got[7].docs) < 100 and got[8].total == 0 and len(got[10].docs) == 0 and got[10].total > 0
    assert len(got[9].snippets) == 10 and all(b"<em>" in x for x in got[9].snippets)
    assert min(got[2].docs) < FIRST + 16384 <= max(got[3].docs)  # pages on both sides of the tile boundary
    assert checked > 2300
    # the shapes the keys and columns must have been met on these pages
    seen = [doc for i in (0, 2, 3, 4, 6, 12) for doc in got[i].docs.tolist()]
    lens = {None if t.keys[doc - FIRST] is None else len(t.keys[doc - FIRST]) for doc in seen}
    assert {None, 0, 1, 63, 64, 65, 255, 256, 257} <= lens
    assert any(t.cols[t.c_signed][0][doc - FIRST] == I64_MIN % (1 << 64) and not t.cols[t.c_signed][1][doc - FIRST] for doc in got[12].docs)
    assert any(t.cols[t.c_f64][0][doc - FIRST] == NAN_BITS for doc in got[4].docs)
    assert any(t.cols[t.c_f64][0][doc - FIRST] == 1 << 63 for doc in got[4].docs)  # -0.0


def test_column_and_key_sorted_pages_of_one_batch(table):
    t = table
    d, s = t.dense, t.sparse
    every = [t.c_signed, t.c_unsigned, t.c_f64, t.c_rank]
    qs = [
        Query([d[0]], sort_column=t.c_rank, descending=False, offset=30, limit=100, documents=every),  # fused selection
        Query([d[0]], limit=20),
        Query([d[0]], sort_column=t.c_rank, descending=True, offset=7, limit=64, documents=[t.c_rank]),
        Query([d[1]], sort_column=t.c_unsigned, descending=True, offset=1000, limit=100, documents=[t.c_unsigned, NO]),  # full sort
        Query([d[0]], sort_primary_key=True, descending=True, limit=100, documents=every),  # the reference's default order
        Query([d[1]], sort_primary_key=True, descending=False, offset=10, limit=1024, documents=[]),
        Query([d[0]], sort_score=True, limit=10, documents=[t.c_f64]),
        Query([s[0]], sort_primary_key=True, descending=True, offset=5000, limit=10, documents=every),  # past the total
        Query([d[2]], limit=30, descending=True, documents=[t.c_signed]),
        Query([d[0]], sort_score=True, limit=5),
    ]
    got, checked = run_thrice(t, qs)
    assert [len(g.docs) for g in got[:6]] == [100, 20, 64, 100, 100, 1024] and len(got[7].docs) == 0
    ranks = [int(x.values[0]) for x in got[2].documents]
    assert ranks == sorted(ranks, reverse=True)  # the gathered values are the order the page was sorted by
    assert checked > 1400


def refused(call):
    rc = call()
    return rc, cap.load().mgx_last_error().decode()


def test_refusals_leave_the_index_usable(table):
    t = table
    L = cap.load()
    dev = t.p.dev
    d = t.dense
    plain_q = Query([d[0]], limit=20, descending=False)
    plain_want = dev.search_batch([plain_q])[0].docs.tolist()

    def still_serves():
        assert dev.search_batch([plain_q])[0].docs.tolist() == plain_want

    def requests(n, columns=(), enabled=True):
        reqs = (cap.DocumentRequest * max(n, 1))()
        ids = (C.c_uint32 * max(len(columns), 1))(*columns)
        for i in range(n):
            reqs[i] = cap.DocumentRequest(int(enabled), len(columns), ids)
        return reqs, ids

    two = [Query([d[0]], sort_score=True, limit=5), Query([d[1]], limit=5)]
    one_req, _keep1 = requests(2, [t.c_signed])
    # null arguments, a wrong n_queries, a second call, a call after the first execute, fetch before mgx_batch_fetch
    b = dev.prepare(two)
    for call in (lambda: L.mgx_batch_set_documents(None, one_req, 2, 0), lambda: L.mgx_batch_set_documents(b._h, None, 2, 0),
                 lambda: L.mgx_batch_set_documents(b._h, one_req, 1, 0), lambda: L.mgx_batch_fetch_documents(b._h, None),
                 lambda: L.mgx_batch_defer_documents(None, 1), lambda: L.mgx_index_max_primary_key_bytes(None, None),
                 lambda: L.mgx_index_attach_primary_key_bytes(t.dev_index._h, None, None, None)):
        assert refused(call)[0] == INVALID_ARGUMENT
        still_serves()
    assert L.mgx_batch_set_documents(b._h, one_req, 2, 0) == 0
    rc, msg = refused(lambda: L.mgx_batch_set_documents(b._h, one_req, 2, 0))
    assert rc == INVALID_ARGUMENT and "once" in msg
    dv = cap.DocumentView()
    rc, msg = refused(lambda: L.mgx_batch_fetch_documents(b._h, C.byref(dv)))
    assert rc == INVALID_ARGUMENT and "mgx_batch_fetch" in msg
    b.execute()
    rc, msg = refused(lambda: L.mgx_batch_fetch_documents(b._h, C.byref(dv)))
    assert rc == INVALID_ARGUMENT and "mgx_batch_fetch" in msg
    b.fetch()
    assert L.mgx_batch_fetch_documents(b._h, C.byref(dv)) == 0 and dv.n_entries == 10
    b2 = dev.prepare(two)
    b2.execute()
    rc, msg = refused(lambda: L.mgx_batch_set_documents(b2._h, one_req, 2, 0))
    assert rc == INVALID_ARGUMENT and "before the first execute" in msg
    still_serves()
    # a request on a faceted query
    fb = dev.prepare([Query([d[0]], facet_columns=[t.c_rank]), Query([d[1]], limit=5)])
    rc, msg = refused(lambda: L.mgx_batch_set_documents(fb._h, one_req, 2, 0))
    assert rc == INVALID_ARGUMENT and "query 0" in msg and "faceted" in msg
    with pytest.raises(ValueError):
        Query([d[0]], facet_columns=[t.c_rank], documents=[])
    still_serves()
    # limit 0 and above 1024, an unknown column id, more than 32 columns, the arena's cap
    for limit in (0, 1025):
        bl = dev.prepare([Query([d[1]], limit=5), Query([d[0]], limit=limit)])
        rc, msg = refused(lambda: L.mgx_batch_set_documents(bl._h, one_req, 2, 0))
        assert rc == OUT_OF_RANGE and "query 1" in msg and "limit" in msg, msg
        still_serves()
    bc = dev.prepare(two)
    bad_col, _keep2 = requests(2, [t.c_signed, 77])
    rc, msg = refused(lambda: L.mgx_batch_set_documents(bc._h, bad_col, 2, 0))
    assert rc == OUT_OF_RANGE and "query 0" in msg and "column" in msg
    many, _keep3 = requests(2, [t.c_signed] * 33)
    rc, msg = refused(lambda: L.mgx_batch_set_documents(bc._h, many, 2, 0))
    assert rc == OUT_OF_RANGE and "query 0" in msg and "32" in msg
    big = dev.prepare([Query([d[1]], limit=5), Query([d[0]], limit=1024)])
    rc, msg = refused(lambda: L.mgx_batch_set_documents(big._h, one_req, 2, 300_000))
    assert rc == OUT_OF_RANGE and "query 1" in msg and "MGX_DOC_ARENA_CAP" in msg and "lower limit" in msg and "max_key_bytes" in msg
    assert L.mgx_batch_set_documents(bc._h, one_req, 2, 0) == 0  # (the refused batch takes a good request afterwards)
    bc._documents = [[t.c_signed], [t.c_signed]]
    bc.execute()
    got = bc.fetch()
    assert sum(t.check(Query(documents=[t.c_signed]), g) for g in got) == 10
    still_serves()
    # records sized for shorter keys than the index holds: the fetch says so, it returns no cut key
    short = dev.prepare([Query([d[0]], limit=1024, descending=False)])
    keys_only, _keep4 = requests(1)
    assert L.mgx_batch_set_documents(short._h, keys_only, 1, 8) == 0
    short.execute()
    short.fetch()
    rc, msg = refused(lambda: L.mgx_batch_fetch_documents(short._h, C.byref(dv)))
    assert rc == OUT_OF_RANGE and "query 0" in msg and "max_key_bytes" in msg
    still_serves()
    # every sharded entry point, before anything is touched
    sb = dev.prepare([Query([d[0]], sort_score=True, limit=5, documents=[]), Query([d[0]], sort_score=True, limit=5)])
    sb.execute()
    stride = C.c_uint32()
    dummy = (C.c_uint64 * 64)()
    blob, nbytes, off32 = C.c_void_p(), C.c_uint64(), C.c_uint64()
    fn = cap.GATHER_FN(lambda *a: 7)
    calls = {
        "mgx_batch_export_topk": lambda: L.mgx_batch_export_topk(sb._h, None, None, C.byref(stride), None),
        "mgx_batch_export_buffer": lambda: L.mgx_batch_export_buffer(sb._h, C.byref(blob), C.byref(nbytes), C.byref(off32)),
        "mgx_batch_merge_shards": lambda: L.mgx_batch_merge_shards(sb._h, 1, dummy, 0, C.cast(dummy, C.c_void_p), 0, None),
        "mgx_batch_exchange": lambda: L.mgx_batch_exchange(sb._h, None, None),
        "mgx_batch_execute_gather": lambda: L.mgx_batch_execute_gather(sb._h, 2, fn, None, None),
        "mgx_batch_execute_sharded": lambda: L.mgx_batch_execute_sharded(sb._h, None, None),
    }
    for name, call in calls.items():
        rc, msg = refused(call)
        assert rc == NOT_IMPLEMENTED and name in msg and "sharded" in msg and "documents" in msg, (name, msg)
    got = sb.fetch()  # the batch itself is served as before
    assert t.check(Query(documents=[]), got[0]) == 5
    # mgx_batch_merge_local over two indexes of which neither is a delta
    ma = dev.prepare([Query([d[0]], sort_score=True, limit=5, documents=[])])
    mb = dev.prepare([Query([d[0]], sort_score=True, limit=5, documents=[])])
    ma.execute()
    mb.execute()
    others = (C.c_void_p * 1)(mb._h.value)
    rc, msg = refused(lambda: L.mgx_batch_merge_local(ma._h, others, 1, None))
    assert rc == NOT_IMPLEMENTED and "one main index and one delta" in msg
    assert t.check(Query(documents=[]), ma.fetch()[0]) == 5
    still_serves()
    # an index without attached keys
    bare = mg.Index(corpus=mg.Corpus.synthetic(500, seed=3), first_doc_id=1)
    assert bare.device_index.max_primary_key_bytes() == 0 and t.dev_index.max_primary_key_bytes() == 257
    with pytest.raises(cap.MgxError) as e:
        bare.prepare([Query([dense_grams(bare, 1)[0]], limit=5, documents=[])])
    assert e.value.code == INVALID_ARGUMENT and "mgx_index_attach_primary_key_bytes" in str(e.value)


def test_replaced_keys_are_what_later_batches_return(table):
    """mgx_index_attach_primary_key_bytes called again replaces the bytes (and the longest key)."""
    t = table
    q = Query([t.dense[0]], limit=40, descending=False, documents=[])
    old = t.keys
    try:
        t.keys = [b"r%d" % (i * 3) if i % 4 else None for i in range(N_DOCS)]
        t.dev_index.attach_primary_key_bytes(t.keys)
        assert t.dev_index.max_primary_key_bytes() == len(b"r%d" % ((N_DOCS - 1) * 3))
        assert t.check(q, t.p.dev.search_batch([q])[0]) == 40
    finally:
        t.keys = old
        t.dev_index.attach_primary_key_bytes(old)
    assert t.check(q, t.p.dev.search_batch([q])[0]) == 40


def gather(index, doc_ids, columns, mapped=None, mapped_columns=None, max_key_bytes=0):
    """mgx_documents_gather -> [None | (mapped, key or None, values, null mask)] per id."""
    L = cap.load()
    ids = np.ascontiguousarray(doc_ids, dtype=np.uint32)
    cols = (C.c_uint32 * max(len(columns), 1))(*columns)
    mcols = (C.c_uint32 * max(len(columns), 1))(*(mapped_columns or []))
    rec, stride = C.c_void_p(), C.c_uint64()
    cap.check(L.mgx_documents_gather(index._h, mapped._h if mapped is not None else None, ids.ctypes.data, len(ids),
                                     len(columns), cols, mcols if mapped is not None else None, max_key_bytes,
                                     C.byref(rec), C.byref(stride)))
    if not len(ids):
        assert not rec.value
        return []
    raw = C.string_at(rec.value, len(ids) * stride.value)
    L.mgx_free(rec)
    out = []
    for i in range(len(ids)):
        r = raw[i * stride.value:(i + 1) * stride.value]
        flags, key_len, mask, n_cols = np.frombuffer(r[:16], np.uint32).tolist()
        if not flags & cap.DOC_FOUND:
            assert (key_len, mask, n_cols) == (0, 0, 0)
            out.append(None)
            continue
        assert n_cols == len(columns)
        values = np.frombuffer(r[16:16 + 8 * n_cols], np.uint64).tolist()
        key = r[16 + 8 * n_cols:16 + 8 * n_cols + key_len] if flags & cap.DOC_HAS_KEY else None
        out.append((bool(flags & cap.DOC_MAPPED), key, values, mask))
    return out


def test_gather_over_an_id_list_without_a_batch(table):
    """mgx_documents_gather: the rows of a caller's id list, unknown ids among them, on a leased stand-alone call."""
    t = table
    rng = np.random.default_rng(7)
    ids = np.concatenate([[0, FIRST - 1, FIRST, FIRST + N_DOCS - 1, FIRST + N_DOCS, 0xFFFFFFFF, FIRST + 16383, FIRST + 16384],
                          rng.integers(FIRST, FIRST + N_DOCS, 3000)]).astype(np.uint32)
    columns = [t.c_signed, NO, t.c_f64, t.c_signed, t.c_rank, t.c_unsigned]
    rows = gather(t.dev_index, ids, columns)
    unknown = 0
    for doc, row in zip(ids.tolist(), rows):
        if not FIRST <= doc < FIRST + N_DOCS:
            assert row is None, doc
            unknown += 1
            continue
        key, vals, mask = t.want(doc, columns)
        assert row == (False, key, vals, mask), doc
    assert unknown == 4
    assert [r[1] for r in gather(t.dev_index, ids[2:4], [])] == [t.keys[0], t.keys[N_DOCS - 1]]  # keys only
    assert gather(t.dev_index, [], columns) == []
    # refusals, by code; the index serves afterwards
    L = cap.load()
    rec, stride = C.c_void_p(), C.c_uint64()
    one = (C.c_uint32 * 1)(FIRST)
    bad = (C.c_uint32 * 1)(77)
    many = (C.c_uint32 * 33)(*[t.c_signed] * 33)
    assert L.mgx_documents_gather(None, None, one, 1, 0, None, None, 0, C.byref(rec), C.byref(stride)) == INVALID_ARGUMENT
    assert L.mgx_documents_gather(t.dev_index._h, None, None, 1, 0, None, None, 0, C.byref(rec), C.byref(stride)) == INVALID_ARGUMENT
    assert L.mgx_documents_gather(t.dev_index._h, t.dev_index._h, one, 1, 0, None, None, 0, C.byref(rec), C.byref(stride)) == INVALID_ARGUMENT
    assert L.mgx_documents_gather(t.dev_index._h, None, one, 1, 1, bad, None, 0, C.byref(rec), C.byref(stride)) == OUT_OF_RANGE
    assert L.mgx_documents_gather(t.dev_index._h, None, one, 1, 33, many, None, 0, C.byref(rec), C.byref(stride)) == OUT_OF_RANGE
    long_key = FIRST + next(i for i, k in enumerate(t.keys) if k is not None and len(k) > 100)
    assert L.mgx_documents_gather(t.dev_index._h, None, (C.c_uint32 * 1)(long_key), 1, 0, None, None, 8, C.byref(rec),
                                  C.byref(stride)) == OUT_OF_RANGE
    assert "max_key_bytes" in L.mgx_last_error().decode() and not rec.value
    bare = mg.Index(corpus=mg.Corpus.synthetic(500, seed=3), first_doc_id=1)
    assert L.mgx_documents_gather(bare.device_index._h, None, one, 1, 0, None, None, 0, C.byref(rec), C.byref(stride)) == INVALID_ARGUMENT
    assert gather(t.dev_index, [FIRST], [t.c_rank])[0] == (False,) + tuple(t.want(FIRST, [t.c_rank]))


def test_gather_over_a_main_index_and_its_delta():
    m = Merged()
    ids = np.concatenate([[0, 4, 9_999, 10_001, 10_000 + 3 * m.N_DELTA, FIRST + m.N_MAIN], np.arange(FIRST, FIRST + 200),
                          m.ids[::5], [int(m.ids[100])]]).astype(np.uint32)
    rows = gather(m.main.device_index, ids, m.cm, mapped=m.delta.device_index, mapped_columns=m.cd)
    n_none = 0
    for doc, row in zip(ids.tolist(), rows):
        if doc not in m.slot_of and not FIRST <= doc < FIRST + m.N_MAIN:
            assert row is None, doc
            n_none += 1
            continue
        assert row == m.want(doc), doc
    assert n_none == 6 and len(rows[-1][1]) == 300


class Merged:
    """A main index and a delta whose documents carry table ids above the main index's through a doc map."""
    N_MAIN, N_DELTA = 3000, 1200

    def __init__(self):
        L = self.L = cap.load()
        rng = np.random.default_rng(95)
        self.main = mg.Index(corpus=mg.Corpus.synthetic(self.N_MAIN, seed=81), first_doc_id=FIRST)
        self.delta = mg.Index(corpus=mg.Corpus.synthetic(self.N_DELTA, seed=82), first_doc_id=1)
        self.ids = (10_000 + 3 * np.arange(self.N_DELTA)).astype(np.uint32)
        cap.check(L.mgx_index_set_doc_map(self.delta.device_index._h, self.ids.ctypes.data, self.N_DELTA))
        self.main.device_index.set_primary_key_shortcut(False)
        self.km = [b"%d" % v for v in rng.permutation(self.N_MAIN) * 7 + 50]
        self.kd = [b"%d" % v for v in rng.permutation(self.N_DELTA) * 7 + 53]
        self.km[11], self.kd[40], self.kd[9] = b"007", b"7", None
        self.kd[100] = b"x" * 300  # the longest key is the delta's: the primary's records must be sized for it
        for ix, keys in ((self.main, self.km), (self.delta, self.kd)):
            ix.device_index.set_primary_keys(keys)
            ix.device_index.attach_primary_key_bytes(keys)
        self.slot_of = {int(t): i for i, t in enumerate(self.ids)}
        # the main index holds columns a, b; the delta holds an unrelated column first, then a, b and one the main lacks
        nm, nd = self.N_MAIN, self.N_DELTA
        self.ma = (rng.integers(-9, 9, nm).astype(np.int64), rng.random(nm) < 0.3)
        self.mb = (rng.integers(0, 1 << 40, nm).astype(np.uint64), np.zeros(nm, bool))
        self.da = (rng.integers(-9, 9, nd).astype(np.int64), rng.random(nd) < 0.3)
        self.db = (rng.integers(0, 1 << 40, nd).astype(np.uint64), np.zeros(nd, bool))
        self.dc = (rng.integers(0, 50, nd).astype(np.uint64), rng.random(nd) < 0.5)
        self.cm = [self.main.device_index.add_filter_column(*self.ma), self.main.device_index.add_filter_column(self.mb[0]), NO]
        self.delta.device_index.add_filter_column(np.zeros(nd, np.int64))
        self.cd = [self.delta.device_index.add_filter_column(*self.da), self.delta.device_index.add_filter_column(self.db[0]),
                   self.delta.device_index.add_filter_column(*self.dc)]
        self.dense = dense_grams(self.main, 3)

    def want(self, doc):
        """(mapped, key, values, null mask) of a table id, for the request [a, b, c]."""
        if doc in self.slot_of:
            i = self.slot_of[doc]
            cols, key, mapped = (self.da, self.db, self.dc), self.kd[i], True
        else:
            i = doc - FIRST
            cols, key, mapped = (self.ma, self.mb, None), self.km[i], False
        vals, mask = [], 0
        for c, col in enumerate(cols):
            nul = col is None or bool(col[1][i])
            vals.append(0 if nul else int(col[0][i]) % (1 << 64))
            mask |= int(nul) << c
        return mapped, key, vals, mask

    def search(self, shapes, defer):
        """The same queries on both indexes (a sort column by each index's own id), the request [a, b, c] by each index's
        own ids, records sized for the longer of the two longest keys; the primary's kernel deferred to the merge or not."""
        bm = self.main.prepare([Query(**dict(kw, sort_column=self.cm[1]) if "sort_column" in kw else kw) for kw in shapes])
        bd = self.delta.prepare([Query(**dict(kw, sort_column=self.cd[1]) if "sort_column" in kw else kw) for kw in shapes])
        longest = max(self.main.device_index.max_primary_key_bytes(), self.delta.device_index.max_primary_key_bytes())
        assert longest == 300
        bm._set_documents([self.cm] * len(shapes), longest)
        bd._set_documents([self.cd] * len(shapes), longest)
        cap.check(self.L.mgx_batch_defer_documents(bm._h, int(defer)))
        bm.execute()
        bd.execute()
        others = (C.c_void_p * 1)(bd._h.value)
        cap.check(self.L.mgx_batch_merge_local(bm._h, others, 1, None))
        got = bm.fetch()
        bd.fetch()
        return got


@pytest.mark.parametrize("defer", [True, False])
def test_a_main_index_and_its_delta(defer):
    m = Merged()
    d = m.dense
    shapes = [
        dict(terms=[d[0]], sort_score=True, limit=50),                            # score group
        dict(terms=[d[0]], limit=100, descending=False),                          # doc-page group, ascending
        dict(terms=[d[1]], limit=100, descending=True),                           # and reversed: the delta's ids first
        dict(terms=[d[0]], sort_score=True, offset=1000, limit=60),               # bitmap group: deep SORT _score
        dict(terms=[d[0]], sort_primary_key=True, descending=True, limit=200),    # the reference's default order
        dict(terms=[d[1]], sort_column="b", descending=False, offset=20, limit=80),  # column b of either index
    ]
    got = m.search(shapes, defer)
    n_mapped = n_plain = 0
    for g, kw in zip(got, shapes):
        assert len(g.documents) == len(g.docs) > 0, kw
        for doc, x in zip(g.docs.tolist(), g.documents):
            mapped, key, vals, mask = m.want(doc)
            assert x is not None and x.mapped == mapped, (kw, doc)
            assert x.key == key and x.values.tolist() == vals and x.null_mask == mask, (kw, doc)
            n_mapped += mapped
            n_plain += not mapped
    assert n_mapped > 100 and n_plain > 100
    assert [len(g.docs) for g in got] == [50, 100, 100, 60, 200, 80]
