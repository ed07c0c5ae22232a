"""-m gpu: SORT <filter column> ASC|DESC through the C ABI (engine.Query(sort_column=...)). Every page is compared with
the reference's string-key model (column_sort_ref.py) applied to the oracle's result set of the same query: doc ids and
totals are exact, there is no tolerance. The fused selection (offset + limit <= 1024) and the expand-and-sort path
(beyond, limit 0, MGX_COLSORT_FULL=1) must agree with the model and so with each other."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pkg import mg  # (first: it puts the repository root on sys.path, which the child process below starts without)

import column_sort_ref as R  # noqa: E402
from gpu_util import Pair  # noqa: E402

pytestmark = pytest.mark.gpu
Query = mg.engine.Query
N_DOCS, FIRST = 40_001, 5  # three 16384-doc tiles, the last partial
OUT_OF_RANGE, INVALID_ARGUMENT, NOT_IMPLEMENTED = 3, 2, 4
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
COLUMNS = ("int7", "int_ext", "double", "uint", "string", "bool")
LIMITS, OFFSETS = (1, 10, 100, 1024, 0), (0, 7, 1000, 50_000)
PAGES = [(o, l) for l in LIMITS for o in OFFSETS] + [(24, 1000), (25, 1000)]  # offset + limit = 1024 | 1025: the path switch
_LINE = re.compile(r"\[mgx\] column sort: (\d+) fused runs in (\d+) workgroups, (\d+) full-sort runs")


def _column_values(name, rng):
    """[None | (type, v)] by slot."""
    n = N_DOCS
    if name == "int7":  # 7 distinct values, 10 % NULL
        v = rng.integers(-3, 4, n)
        nul = rng.random(n) < 0.1
        return [None if z else ("int64", int(x)) for x, z in zip(v, nul)]
    if name == "int_ext":  # extremes, no NULL (INT64_MIN without NULLs sorts exactly)
        pool = [I64MIN, I64MIN + 1, -1, 0, 1, I64MAX - 1, I64MAX, 1 << 40, -(1 << 40)]
        return [("int64", pool[i]) for i in rng.integers(0, len(pool), n)]
    if name == "double":
        pool = [0.0, -0.0, float("inf"), float("-inf"), 5e-324, -5e-324, 1.5, -1.5, 1e300, -1e300, 2.2250738585072014e-308]
        nul = rng.random(n) < 0.1
        return [None if z else ("double", pool[i]) for i, z in zip(rng.integers(0, len(pool), n), nul)]
    if name == "uint":  # both sides of INT64_MAX
        pool = [0, 1, I64MAX - 1, I64MAX, I64MAX + 1, I64MAX + 2, R.U64, 12345]
        return [("uint64", pool[i]) for i in rng.integers(0, len(pool), n)]
    if name == "string":  # holds "" and NULLs: the two tie
        pool = ["", "a", "A", "ab", "b", "é", "zz"]
        nul = rng.random(n) < 0.1
        return [None if z else ("string", pool[i]) for i, z in zip(rng.integers(0, len(pool), n), nul)]
    assert name == "bool"
    return [("bool", bool(x)) for x in rng.integers(0, 2, n)]


class Table:
    def __init__(self):
        self.p = Pair(corpus=mg.Corpus.synthetic(N_DOCS, seed=71), first_doc_id=FIRST)
        rng = np.random.default_rng(72)
        di = self.p.dev.device_index
        self.values, self.col = {}, {}
        for name in COLUMNS:
            vals = self.values[name] = _column_values(name, rng)
            cls, ranks, bias, bits, nulls = R.column_of(vals)
            arr = np.asarray(bits, dtype=np.uint64)
            arr = arr.view(np.int64) if cls == R.SIGNED else arr.view(np.float64) if cls == R.DOUBLE else arr
            self.col[name] = (di.add_filter_column(arr, np.asarray(nulls, bool)), ranks, bias)
        flt = rng.integers(-40, 40, N_DOCS).astype(np.int64)
        self.cond_col = self.p.add_column(flt, rng.random(N_DOCS) < 0.1)  # FILTER operand the oracle knows too
        c = self.p.dev.columns
        sizes = np.diff(c.offsets.astype(np.int64))
        order = [g for g in np.argsort(-sizes, kind="stable") if b" " not in c.gram(g)]
        dense = [c.gram(g).decode() for g in order[:6]]
        sparse = [c.gram(g).decode() for g in order if 4 < sizes[g] <= 60]
        nothing = None
        for a in sparse[:12]:  # two rare grams no document holds together: the query reaches the device and matches nothing
            for b in sparse[:12]:
                if a < b and self.p.oracle_query(Query([a, b], limit=0, descending=False))[0] == 0:
                    nothing = [a, b]
        assert nothing is not None
        self.shapes = {
            "dense": dict(terms=[dense[0]]),
            "few": dict(terms=[sparse[0]]),
            "nothing": dict(terms=nothing),
            "not_filter": dict(terms=[dense[1]], not_terms=[dense[2]], conditions=[(self.cond_col, 5, 0)]),  # >= 0
            "expr": dict(expr=("or", ("and", dense[0], dense[3]), sparse[1])),
        }
        self.base = {}
        for name, kw in self.shapes.items():
            total, docs, _, r = self.p.oracle_query(Query(limit=0, descending=False, **kw))
            self.base[name] = (np.asarray(docs, np.int64).tolist(), r)
        assert len(self.base["dense"][0]) > 4096  # several LDS runs and a global stage in the full sort
        assert 0 < len(self.base["few"][0]) < 100
        self._sorted = {}

    def query(self, shape, column, descending, offset, limit):
        cid, ranks, bias = self.col[column]
        return Query(sort_column=cid, sort_ranks=ranks, sort_key_bias=bias, descending=descending, offset=offset,
                     limit=limit, **self.shapes[shape])

    def want(self, shape, column, descending, offset, limit):
        """The reference's page: string keys over the oracle's result set (sorted once per shape, column, direction)."""
        key = (shape, column, descending)
        if key not in self._sorted:
            docs = self.base[shape][0]
            vals = self.values[column]
            self._sorted[key] = R.sort_entries(docs, {d: vals[d - FIRST] for d in docs}, not descending)
        s = self._sorted[key]
        return R.apply_offset_limit(s, offset, limit if limit else len(s))


@pytest.fixture(scope="module")
def table():
    return Table()


def _mixed_batch(t, column):
    """Every shape x direction x page of one column, with a score query and two docid queries between them."""
    qs, meta = [], []
    dense = t.shapes["dense"]["terms"]
    for shape in t.shapes:
        for descending in (False, True):
            for offset, limit in PAGES:
                qs.append(t.query(shape, column, descending, offset, limit))
                meta.append((shape, descending, offset, limit))
            qs.append(Query(dense, sort_score=True, limit=10))
            meta.append("score")
            qs.append(Query(dense, limit=20, descending=descending))
            meta.append("page")
            qs.append(Query(**t.shapes["not_filter"], limit=0, descending=descending))
            meta.append("all")
    return qs, meta


@pytest.mark.parametrize("column", COLUMNS)
def test_pages_equal_the_model_over_the_oracles_result_set(table, column, monkeypatch, capfd):
    t = table
    qs, meta = _mixed_batch(t, column)
    monkeypatch.setenv("MGX_VERBOSE", "1")
    capfd.readouterr()
    got = t.p.dev.search_batch(qs)
    err = capfd.readouterr().err
    monkeypatch.delenv("MGX_VERBOSE")
    m = _LINE.search(err)
    assert m and int(m.group(1)) > 0 and int(m.group(3)) > 0, err[-400:]  # both paths ran
    assert int(m.group(2)) > int(m.group(1))  # ... and some run was merged from several workgroups
    others = [q for q, k in zip(qs, meta) if isinstance(k, str)]
    alone = t.p.dev.search_batch(others)  # the same neighbours without a column-sorted query in the batch
    plain = {}
    for shape in t.shapes:
        plain[shape] = t.p.dev.search_batch([Query(limit=0, descending=False, **t.shapes[shape])])[0]
    j = 0
    for q, g, k in zip(qs, got, meta):
        if isinstance(k, str):
            a = alone[j]
            j += 1
            assert g.total == a.total and g.docs.tolist() == a.docs.tolist() and np.array_equal(g.scores, a.scores), k
            continue
        shape, descending, offset, limit = k
        want = t.want(shape, column, descending, offset, limit)
        assert g.docs.tolist() == want, (column,) + k
        assert not np.any(g.scores), k
        base, r = t.base[shape]
        assert g.total == len(base) == plain[shape].total, k
        for c in ("total_candidates", "after_intersection", "after_not", "after_filters"):
            assert getattr(g, c) == getattr(plain[shape], c), (k, c)
            if not r["empty_term_detected"]:
                assert getattr(g, c) == r[c], (k, c)


def _dump(column):
    """Child-process body: the column's pages as JSON on stdout (the parent sets MGX_COLSORT_FULL)."""
    t = Table()
    qs, meta = _mixed_batch(t, column)
    got = t.p.dev.search_batch(qs)
    print("PAGES " + json.dumps([g.docs.tolist() for g in got]))


def test_forced_full_sort_returns_the_default_pages(table):
    """MGX_COLSORT_FULL=1 in a fresh child process: every page through expand -> column_keys_kernel -> the bitonic sort."""
    column = "int7"
    qs, meta = _mixed_batch(table, column)
    default = [g.docs.tolist() for g in table.p.dev.search_batch(qs)]
    env = dict(os.environ, MGX_COLSORT_FULL="1", MGX_VERBOSE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", column], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    m = _LINE.search(r.stderr)
    assert m and int(m.group(1)) == 0 and int(m.group(3)) > 0, r.stderr[-400:]  # no fused run in the child
    line = [x for x in r.stdout.splitlines() if x.startswith("PAGES ")][0]
    assert json.loads(line[6:]) == default


def test_refusals(table):
    t = table
    terms = t.shapes["dense"]["terms"]
    di = t.p.dev.device_index

    def refused(qs, **kw):
        with pytest.raises(mg._capi.MgxError) as e:
            t.p.dev.search_batch(qs, **kw)
        return e.value.code, str(e.value)
    cid = t.col["int7"][0]
    assert refused([Query(terms, sort_column=10_000)])[0] == OUT_OF_RANGE
    assert refused([Query(terms, sort_column=t.col["string"][0], sort_ranks=True, sort_key_bias=2)])[0] == INVALID_ARGUMENT
    assert refused([Query(terms, sort_column=cid, sort_key_bias=1)])[0] == INVALID_ARGUMENT  # a bias without ranks
    assert refused([Query(terms, sort_column=cid, sort_ranks=True)])[0] == INVALID_ARGUMENT  # ranks on a signed column
    with pytest.raises(ValueError):
        Query(terms, sort_score=True, sort_column=cid)
    # INT64_MIN beside NULLs / the all-ones double beside NULLs: marked when the column is added, refused when sorted by
    v = np.zeros(N_DOCS, np.int64)
    v[3] = I64MIN
    nul = np.zeros(N_DOCS, bool)
    nul[9] = True
    code, msg = refused([Query(terms, sort_column=di.add_filter_column(v, nul))])
    assert code == NOT_IMPLEMENTED and "INT64_MIN" in msg
    d = np.zeros(N_DOCS, np.uint64)
    d[3] = R.U64
    code, msg = refused([Query(terms, sort_column=di.add_filter_column(d.view(np.float64), nul))])
    assert code == NOT_IMPLEMENTED
    exact = di.add_filter_column(v, np.zeros(N_DOCS, bool))  # without NULLs the same values sort exactly
    g = t.p.dev.search_batch([Query(terms, sort_column=exact, descending=False, limit=1)])[0]
    assert g.docs.tolist() == ([FIRST + 3] if FIRST + 3 in t.base["dense"][0] else t.base["dense"][0][:1])
    # a highlighted batch that holds a column-sorted query
    code, msg = refused([Query(terms, sort_score=True, limit=5, highlight=True), Query(terms, sort_column=cid, limit=5)])
    assert code == NOT_IMPLEMENTED and "highlight" in msg
    # the sharded entry points that need no communicator
    _sharded_refusals(t.p.dev, terms, cid, comm=None)


def _sharded_refusals(dev, terms, cid, comm):
    """Every sharded entry point refuses a batch that holds a column-sorted query, before it touches anything."""
    import ctypes as C
    L = mg._capi.load()
    batch = dev.prepare([Query(terms, sort_score=True, limit=5), Query(terms, sort_column=cid, limit=5)])
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
    if comm is not None:
        calls["mgx_batch_exchange"] = lambda: L.mgx_batch_exchange(batch._h, comm._h, None)
        calls["mgx_batch_execute_sharded"] = lambda: L.mgx_batch_execute_sharded(batch._h, comm._h, None)
    for name, call in calls.items():
        assert call() == NOT_IMPLEMENTED, name
        msg = L.mgx_last_error().decode()
        assert "sharded" in msg and "filter column" in msg, (name, msg)
    got = batch.fetch()  # the batch itself is served as before
    assert len(got[1].docs) == 5
    return sorted(calls)


def test_sharded_entry_points_that_take_a_communicator_refuse():
    """mgx_batch_exchange and mgx_batch_execute_sharded, over a communicator of one rank, in a fresh child process (the
    suite's own process opens no RCCL communicator)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sharded"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert "REFUSED mgx_batch_exchange mgx_batch_execute_gather mgx_batch_execute_sharded mgx_batch_export_buffer " \
           "mgx_batch_export_topk mgx_batch_merge_shards" in r.stdout, r.stdout[-1000:]


def _sharded_child():
    from mygram_db_amd import dist
    corpus = mg.Corpus.synthetic(20_000, seed=73)
    idx = mg.Index(corpus=corpus, first_doc_id=1)
    c = idx.columns
    sizes = np.diff(c.offsets.astype(np.int64))
    gram = max((g for g in range(c.n_grams) if b" " not in c.gram(g)), key=lambda g: sizes[g])
    cid = idx.device_index.add_filter_column(np.arange(20_000, dtype=np.int64))
    comm = dist.Comm(rank=0, world=1, device=0)
    print("REFUSED " + " ".join(_sharded_refusals(idx, [c.gram(gram).decode()], cid, comm)))


if __name__ == "__main__":
    if sys.argv[1] == "--sharded":
        _sharded_child()
    else:
        assert sys.argv[1] == "--dump"
        _dump(sys.argv[2])
