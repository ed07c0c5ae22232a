"""-m gpu: SORT by primary key through the C ABI (engine.Query(sort_primary_key=True), DeviceIndex.set_primary_keys).
Every page is compared with the reference's string-key model (primary_key_ref.py) applied to the oracle's result set of
the same query: doc ids and totals are exact, there is no tolerance. One index: the fused selection (offset + limit <=
1024), the expand-and-sort path beyond it, the doc-id shortcut of monotone keys and its absence (MGX_PK_SORT_GENERAL=1).
Two indexes (a main index and a delta, mgx_batch_merge_local): the merge by numbers and the merge by key strings
(key_merge_kernel) against the model over the documents of both."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pkg import mg  # (first: it puts the repository root on sys.path, which the child process below starts without)

import primary_key_ref as P  # noqa: E402
from gpu_util import Pair  # noqa: E402

pytestmark = pytest.mark.gpu
Query = mg.engine.Query
N_DOCS, FIRST = 40_001, 5  # three 16384-doc tiles, the last partial
INVALID_ARGUMENT, NOT_IMPLEMENTED = 2, 4
U64 = (1 << 64) - 1
# (offset, limit): a small page; an offset inside the fused path; offset + limit = 1024, its last size; 1025, the full
# sort; unbounded; an offset past every total
PAGES = [(0, 10), (37, 100), (24, 1000), (25, 1000), (0, 0), (50_000, 10)]
_COLSORT = re.compile(r"\[mgx\] column sort: (\d+) fused runs in (\d+) workgroups, (\d+) full-sort runs")
_KEYMERGE = re.compile(r"\[mgx\] key merge: (\d+) queries, (\d+) elements")


def key_set(name, n, rng):
    """[bytes | None] by slot."""
    if name == "shuffled":  # numeric only, in no order: the extremes, both sides of 2^63, and "007" beside "7"
        vals = rng.permutation(n).astype(object) + 100
        keys = [b"%d" % v for v in vals]
        for slot, k in zip(rng.choice(n, 6, replace=False), (b"0", b"%d" % ((1 << 63) - 1), b"%d" % (1 << 63), b"%d" % U64, b"007", b"7")):
            keys[slot] = k
        return keys
    if name == "mixed":
        pool = [b"", b"a", b"ab", b"abc", b"abd", b"\x80", b"\xff\x01", "é".encode(), b"18446744073709551616",
                b"99999999999999999999999", b"pk9", b"pk10", b"007", b"7", b"12a"]
        keys = []
        for i in range(n):
            r = rng.random()
            if r < 0.05:
                keys.append(None)  # no key: the doc id
            elif r < 0.35:
                keys.append(pool[rng.integers(0, len(pool))])  # heavy ties, shared prefixes
            elif r < 0.7:
                keys.append(b"pk%d" % rng.integers(0, 100_000))
            else:
                keys.append(b"%d" % rng.integers(0, 60_000))  # numeric keys in a dictionary of strings
        return keys
    assert name == "monotone"  # never decreasing, with ties and with two spellings of a number
    return [(b"0%d" if i % 5 == 0 else b"%d") % (7 + i // 2) for i in range(n)]


class Table:
    def __init__(self, n_docs=N_DOCS, first=FIRST, seed=71):
        self.n, self.first = n_docs, first
        self.p = Pair(corpus=mg.Corpus.synthetic(n_docs, seed=seed), first_doc_id=first)
        rng = np.random.default_rng(seed + 1)
        flt = rng.integers(-40, 40, n_docs).astype(np.int64)
        self.cond_col = self.p.add_column(flt, rng.random(n_docs) < 0.1)
        c = self.p.dev.columns
        sizes = np.diff(c.offsets.astype(np.int64))
        order = [g for g in np.argsort(-sizes, kind="stable") if b" " not in c.gram(g)]
        self.dense = [c.gram(g).decode() for g in order[:6]]
        sparse = [c.gram(g).decode() for g in order if 4 < sizes[g] <= 60]
        self.shapes = {
            "dense": dict(terms=[self.dense[0]]),
            "few": dict(terms=[sparse[0]]),
            "not_filter": dict(terms=[self.dense[1]], not_terms=[self.dense[2]], conditions=[(self.cond_col, 5, 0)]),  # >= 0
            "expr": dict(expr=("or", ("and", self.dense[0], self.dense[3]), sparse[1])),
        }
        self.base = {}
        for name, kw in self.shapes.items():
            _, docs, _, r = self.p.oracle_query(Query(limit=0, descending=False, **kw))
            self.base[name] = (np.asarray(docs, np.int64).tolist(), r)
        self.keys = None
        self._sorted = {}

    def use(self, name):
        """Replaces the index's keys (mgx_index_set_primary_keys called again)."""
        self.keys = key_set(name, self.n, np.random.default_rng(len(name))) if name else None
        self._sorted = {}
        if name:
            self.p.dev.device_index.set_primary_keys(self.keys)

    def pk_of(self, doc):
        return self.keys[doc - self.first] if self.keys is not None else None

    def want(self, shape, descending, offset, limit):
        key = (shape, descending)
        if key not in self._sorted:
            self._sorted[key] = P.sort_docs(self.base[shape][0], self.pk_of, not descending)
        s = self._sorted[key]
        return s[min(offset, len(s)):min(offset + (limit or len(s)), len(s))]

    def batch(self, pages=PAGES, neighbours=True):
        """Every shape x direction x page, with a score query, a docid page and an unbounded query between them."""
        qs, meta = [], []
        for shape, kw in self.shapes.items():
            for descending in (False, True):
                for offset, limit in pages:
                    qs.append(Query(sort_primary_key=True, descending=descending, offset=offset, limit=limit, **kw))
                    meta.append((shape, descending, offset, limit))
                if neighbours:
                    qs.append(Query([self.dense[0]], sort_score=True, limit=10))
                    meta.append("score")
                    qs.append(Query([self.dense[0]], limit=20, descending=descending))
                    meta.append("page")
                    qs.append(Query(**self.shapes["not_filter"], limit=0, descending=descending))
                    meta.append("all")
        return qs, meta

    def check(self, qs, meta, got):
        plain = {s: self.p.dev.search_batch([Query(limit=0, descending=False, **kw)])[0] for s, kw in self.shapes.items()}
        others = [q for q, k in zip(qs, meta) if isinstance(k, str)]
        alone = self.p.dev.search_batch(others) if others else []
        j = 0
        for g, k in zip(got, meta):
            if isinstance(k, str):  # the neighbours answer as they do without a key-sorted query in the batch
                a = alone[j]
                j += 1
                assert g.total == a.total and g.docs.tolist() == a.docs.tolist() and np.array_equal(g.scores, a.scores), k
                continue
            shape, descending, offset, limit = k
            assert g.docs.tolist() == self.want(shape, descending, offset, limit), k
            assert not np.any(g.scores), k
            base, r = self.base[shape]
            assert g.total == len(base) == plain[shape].total, k
            for c in ("total_candidates", "after_intersection", "after_not", "after_filters"):
                assert getattr(g, c) == getattr(plain[shape], c), (k, c)
                if not r["empty_term_detected"]:
                    assert getattr(g, c) == r[c], (k, c)


@pytest.fixture(scope="module")
def table():
    t = Table()
    assert len(t.base["dense"][0]) > 4096 and 0 < len(t.base["few"][0]) < 100
    return t


def test_an_index_without_keys_pages_by_doc_id(table):
    """(first: the module's index has no keys yet.) Offset 0 takes the doc-id shortcut, the other pages the selection
    and the full sort with the table doc id as the value."""
    t = table
    t.use(None)
    qs, meta = t.batch(neighbours=False)
    got = t.p.dev.search_batch(qs)
    t.check(qs, meta, got)
    for g, (shape, descending, offset, limit) in zip(got, meta):
        ids = t.base[shape][0][::-1] if descending else t.base[shape][0]
        assert g.docs.tolist() == ids[offset:offset + (limit or len(ids))]


@pytest.mark.parametrize("keys", ["shuffled", "mixed"])
def test_pages_equal_the_model_over_the_oracles_result_set(table, keys, monkeypatch, capfd):
    t = table
    t.use(keys)
    qs, meta = t.batch()
    monkeypatch.setenv("MGX_VERBOSE", "1")
    capfd.readouterr()
    got = t.p.dev.search_batch(qs)
    err = capfd.readouterr().err
    monkeypatch.delenv("MGX_VERBOSE")
    m = _COLSORT.search(err)
    assert m and int(m.group(1)) > 0 and int(m.group(3)) > 0, err[-400:]  # the fused selection and the full sort ran
    assert not _KEYMERGE.search(err)  # one index: nothing to merge
    t.check(qs, meta, got)
    if keys == "shuffled":  # "007" and "7": one sort key, the tie goes to the doc id in the sort's direction
        a, b = sorted(FIRST + s for s, k in enumerate(t.keys) if k in (b"007", b"7"))
        r = t.p.dev.search_batch([Query(expr=("or", *t.dense[:4]), sort_primary_key=True, descending=d, limit=0) for d in (False, True)])
        for g, first, second in ((r[0], a, b), (r[1], b, a)):
            docs = g.docs.tolist()
            if a in docs and b in docs:
                assert docs.index(second) == docs.index(first) + 1


def _dump(names):
    """Child-process body (the parent sets MGX_PK_SORT_GENERAL): the pages of each key set as JSON on stdout."""
    t = Table()
    out = {}
    for name in names:
        t.use(name or None)
        qs, _ = t.batch(neighbours=False)
        out[name] = [g.docs.tolist() for g in t.p.dev.search_batch(qs)]
    print("PAGES " + json.dumps(out))


def test_monotone_keys_take_the_doc_id_shortcut_and_the_general_path_agrees(table, monkeypatch, capfd):
    t = table
    t.use("monotone")
    qs, meta = t.batch(neighbours=False)
    got = t.p.dev.search_batch(qs)
    t.check(qs, meta, got)
    for g, (shape, descending, offset, limit) in zip(got, meta):  # key order is doc-id order, ties included
        ids = t.base[shape][0][::-1] if descending else t.base[shape][0]
        assert g.docs.tolist() == ids[offset:offset + (limit or len(ids))]
    first = [(q, k) for q, k in zip(qs, meta) if k[2] == 0]
    monkeypatch.setenv("MGX_VERBOSE", "1")
    capfd.readouterr()
    t.p.dev.search_batch([q for q, _ in first])
    err = capfd.readouterr().err
    monkeypatch.delenv("MGX_VERBOSE")
    assert not _COLSORT.search(err), err[-400:]  # offset 0: plain docid pages, no key is read
    env = dict(os.environ, MGX_PK_SORT_GENERAL="1", MGX_VERBOSE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", "", "monotone"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _COLSORT.search(r.stderr), r.stderr[-400:]  # the child sorted by key
    pages = json.loads([x for x in r.stdout.splitlines() if x.startswith("PAGES ")][0][6:])
    assert pages["monotone"] == [g.docs.tolist() for g in got]
    for page, (shape, descending, offset, limit) in zip(pages[""], meta):  # no keys, no shortcut: still the docid page
        ids = t.base[shape][0][::-1] if descending else t.base[shape][0]
        assert page == ids[offset:offset + (limit or len(ids))]


def test_refusals_and_argument_errors(table):
    t = table
    t.use("shuffled")
    terms = [t.dense[0]]
    dev = t.p.dev

    def refused(qs):
        with pytest.raises(mg._capi.MgxError) as e:
            dev.search_batch(qs)
        return e.value.code, str(e.value)
    q = Query(terms, sort_primary_key=True, limit=5)
    q.sort_column = 1
    assert refused([q])[0] == INVALID_ARGUMENT
    q = Query(terms, sort_primary_key=True, limit=5)
    q.sort_key_bias = 1
    assert refused([q])[0] == INVALID_ARGUMENT
    with pytest.raises(ValueError):
        Query(terms, sort_score=True, sort_primary_key=True)
    with pytest.raises(ValueError):
        Query(terms, sort_column=0, sort_primary_key=True)
    code, msg = refused([Query(terms, sort_score=True, limit=5, highlight=True), Query(terms, sort_primary_key=True, limit=5)])
    assert code == NOT_IMPLEMENTED and "highlight" in msg and "primary key" in msg
    # the sharded entry points that need no communicator
    L = mg._capi.load()
    batch = dev.prepare([Query(terms, sort_score=True, limit=5), Query(terms, sort_primary_key=True, limit=5)])
    batch.execute()
    stride = C.c_uint32()
    dummy = (C.c_uint64 * 64)()
    blob, nbytes, off32 = C.c_void_p(), C.c_uint64(), C.c_uint64()
    fn = mg._capi.GATHER_FN(lambda *a: 7)
    calls = {
        "mgx_batch_export_topk": lambda: L.mgx_batch_export_topk(batch._h, None, None, C.byref(stride), None),
        "mgx_batch_export_buffer": lambda: L.mgx_batch_export_buffer(batch._h, C.byref(blob), C.byref(nbytes), C.byref(off32)),
        "mgx_batch_merge_shards": lambda: L.mgx_batch_merge_shards(batch._h, 1, dummy, 0, C.cast(dummy, C.c_void_p), 0, None),
        "mgx_batch_execute_gather": lambda: L.mgx_batch_execute_gather(batch._h, 2, fn, None, None),
    }
    for name, call in calls.items():
        assert call() == NOT_IMPLEMENTED, name
        msg = L.mgx_last_error().decode()
        assert "sharded" in msg and "primary key" in msg, (name, msg)
    got = batch.fetch()  # the batch itself is served as before
    assert got[1].docs.tolist() == t.want("dense", True, 0, 5)


# ---- a main index and its delta: mgx_batch_merge_local ----

class Merged:
    """A main index and a delta index whose documents carry table ids above the main index's."""
    N_MAIN, N_DELTA = 3000, 1200

    def __init__(self):
        self.main = Table(self.N_MAIN, FIRST, seed=81)
        self.delta = Pair(corpus=mg.Corpus.synthetic(self.N_DELTA, seed=82), first_doc_id=1)
        self.ids = (10_000 + 3 * np.arange(self.N_DELTA)).astype(np.uint32)  # table id of every delta slot, ascending
        self.L = mg._capi.load()
        mg._capi.check(self.L.mgx_index_set_doc_map(self.delta.dev.device_index._h, self.ids.ctypes.data, self.N_DELTA))
        self.main.p.dev.device_index.set_primary_key_shortcut(False)
        d = self.main.dense
        one = self._one_sided(d)
        self.queries = {
            "dense": dict(terms=[d[0]]),
            "expr": dict(expr=("or", ("and", d[0], d[3]), d[4])),
            "main_only": dict(terms=one[0]),
            "delta_only": dict(terms=one[1]),
        }
        self.base = {}
        for name, kw in self.queries.items():
            q = Query(limit=0, descending=False, **kw)
            a = np.asarray(self.main.p.oracle_query(q)[1], np.int64).tolist()
            b = [int(self.ids[x - 1]) for x in np.asarray(self.delta.oracle_query(q)[1], np.int64).tolist()]
            self.base[name] = (a, b)
        assert min(len(x) for x in self.base["dense"]) >= 300  # runs that cross the 256-thread workgroup boundary
        assert self.base["main_only"][0] and not self.base["main_only"][1]
        assert self.base["delta_only"][1] and not self.base["delta_only"][0]

    def _one_sided(self, dense):
        """Two-gram ANDs both indexes know, one matching in the main index only, one in the delta only."""
        found = [None, None]
        cm, cd = self.main.p.dev.columns, self.delta.dev.columns
        sizes = np.diff(cm.offsets.astype(np.int64))
        rare = [cm.gram(g).decode() for g in np.argsort(sizes, kind="stable") if sizes[g] > 2 and b" " not in cm.gram(g)][:40]
        for a in rare:
            for b in rare:
                if a >= b or (found[0] and found[1]):
                    continue
                q = Query([a, b], limit=0, descending=False)
                try:
                    nm, nd = self.main.p.oracle_query(q)[0], self.delta.oracle_query(q)[0]
                except Exception:  # noqa: BLE001 (a gram one index does not know)
                    continue
                if self.delta.dev.posting_size(a) == 0 or self.delta.dev.posting_size(b) == 0:
                    continue
                if nm and not nd and not found[0]:
                    found[0] = [a, b]
                if nd and not nm and not found[1]:
                    found[1] = [a, b]
        assert found[0] and found[1]
        return found

    def set_keys(self, main_keys, delta_keys):
        self.km, self.kd = main_keys, delta_keys
        self.main.p.dev.device_index.set_primary_keys(main_keys)
        self.delta.dev.device_index.set_primary_keys(delta_keys)

    def pk_of(self, doc):
        return self.kd[(doc - 10_000) // 3] if doc >= 10_000 else self.km[doc - FIRST]

    def search(self, qs):
        bm, bd = self.main.p.dev.prepare(qs), self.delta.dev.prepare(qs)
        bm.execute()
        bd.execute()
        others = (C.c_void_p * 1)(bd._h.value)
        mg._capi.check(self.L.mgx_batch_merge_local(bm._h, others, 1, None))
        got = bm.fetch()
        side = bd.fetch()
        return got, side


@pytest.fixture(scope="module")
def merged():
    return Merged()


def _variant_keys(variant, n_main, n_delta):
    rng = np.random.default_rng(len(variant))
    main = [b"%d" % v for v in rng.permutation(n_main) * 7 + 50]
    delta = [b"%d" % v for v in rng.permutation(n_delta) * 7 + 53]  # interleaves with the main index's keys
    main[11], delta[4] = b"007", b"7"  # one sort key in both indexes: tied by table id
    delta[9] = None  # no key: its table id, 10027
    if variant == "numeric_and_one_string":
        delta[100] = b"pk5"  # the delta becomes a dictionary of strings; the main index's digits are derived
    if variant == "both_ranks":
        for i in range(0, n_main, 3):
            main[i] = b"pk%d" % i
        for i in range(0, n_delta, 2):
            delta[i] = [b"pk%d" % (i + 1), b"", b"\x80z", b"pk", b"p", b"18446744073709551616"][(i // 2) % 6] if i % 4 else b"pk%d" % i
        main[11], delta[4] = b"007", b"7"
    return main, delta


@pytest.mark.parametrize("variant", ["both_numeric", "numeric_and_one_string", "both_ranks"])
def test_a_main_index_and_its_delta_merge_by_key(merged, variant, monkeypatch, capfd):
    m = merged
    m.set_keys(*_variant_keys(variant, m.N_MAIN, m.N_DELTA))
    # windows: unbounded; small; one that straddles both sides deep in the fused path; the full sort
    pages = [(0, 0), (0, 10), (290, 400), (700, 1000), (5000, 10)]
    qs, meta = [], []
    for name, kw in m.queries.items():
        for descending in (False, True):
            for offset, limit in pages:
                qs.append(Query(sort_primary_key=True, descending=descending, offset=offset, limit=limit, **kw))
                meta.append((name, descending, offset, limit))
    qs.append(Query([m.main.dense[0]], limit=20))  # a docid page beside them
    monkeypatch.setenv("MGX_VERBOSE", "1")
    capfd.readouterr()
    got, side = m.search(qs)
    err = capfd.readouterr().err
    monkeypatch.delenv("MGX_VERBOSE")
    km = _KEYMERGE.search(err)
    if variant == "both_numeric":
        assert not km, err[-400:]  # numbers compare as they are: the rank merge
    else:
        assert km and int(km.group(1)) == len(meta) and int(km.group(2)) > 600, err[-400:]
    straddles = 0
    for g, k in zip(got, meta):
        name, descending, offset, limit = k
        a, b = m.base[name]
        want = P.page(a + b, m.pk_of, not descending, offset, limit)
        assert g.docs.tolist() == want, (variant,) + k
        assert g.total == len(a) + len(b) and not np.any(g.scores), k
        straddles += 0 < sum(d >= 10_000 for d in want) < len(want)
    assert straddles > 8
    ids = sorted(m.base["dense"][0] + m.base["dense"][1], reverse=True)[:20]
    assert got[-1].docs.tolist() == ids
    for descending in (False, True):  # "007" (main, doc 16) and "7" (delta, doc 10012): neighbours, ordered by table id
        s = P.sort_docs(list(range(FIRST, FIRST + m.N_MAIN)) + m.ids.tolist(), m.pk_of, not descending)
        i = s.index(16)
        assert s[i + (-1 if descending else 1)] == 10_012


def test_a_monotone_main_index_needs_the_shortcut_off_to_merge(merged):
    m = merged
    m.set_keys([b"%d" % i for i in range(m.N_MAIN)], [b"%d" % (5 * i) for i in range(m.N_DELTA)])
    qs = [Query([m.main.dense[0]], sort_primary_key=True, limit=10)]
    m.main.p.dev.device_index.set_primary_key_shortcut(True)
    try:
        with pytest.raises(mg._capi.MgxError) as e:
            m.search(qs)
        assert e.value.code == INVALID_ARGUMENT and "mgx_index_set_primary_key_shortcut" in str(e.value)
    finally:
        m.main.p.dev.device_index.set_primary_key_shortcut(False)
    got, _ = m.search(qs)
    a, b = m.base["dense"]
    assert got[0].docs.tolist() == P.page(a + b, m.pk_of, False, 0, 10)


if __name__ == "__main__":
    assert sys.argv[1] == "--dump"
    _dump(sys.argv[2:])
