#!/usr/bin/env python3
"""SORT by primary key against the orders it should cost the same as, in one process and one session. Not used by the
driver.

    python tools/bench_pksort.py [--docs 1000000] [--queries 256] [--limit 100] [--reps 7] [--delta 0] [--out FILE]

The table: a synthetic corpus; the queries: 2-term ANDs of frequent words, LIMIT --limit, DESC. Each pair below
alternates (`--reps` timed repetitions of execute -> fetch on a prepared batch after a warm-up; medians and spreads):
  (i)  shuffled numeric keys, SORT by primary key, against the same queries sorted by an int64 filter column that holds
       the same numbers: the same selection kernel over the same data shape;
  (ii) keys that ascend with the doc slot, SORT by primary key (the doc-id shortcut), against the plain doc-id page;
       MGX_PK_SORT_GENERAL=1 (read once per process by the library) shows the general path on the same keys.
  (iii) --delta N: a delta index of N documents beside the main index, both prepared, executed and merged
       (mgx_batch_merge_local): numeric keys on both sides (rank_merge_kernel) against a delta whose keys are strings
       (key_merge_kernel). Kernel times come from a run of its own under
       `rocprofv3 --kernel-trace --stats -- python tools/bench_pksort.py --delta 8000 ...`.
Every page of (i) and (ii) is compared with its partner's for equality of doc ids."""
import argparse
import collections
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def frequent_words(corpus, sample, n):
    cnt = collections.Counter()
    for i in range(sample):
        for wd in bytes(corpus.text(i)).decode("utf-8").split():
            if len(wd) >= 3:
                cnt[wd] += 1
    return [wd for wd, _ in cnt.most_common(n)]


def summary(ms):
    return {"median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "runs_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--limit", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--delta", type=int, default=0, help="documents of a delta index merged with the main index (iii)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mg = entry.load_package()
    _capi, Query = mg._capi, mg.engine.Query
    L = _capi.load()
    corpus = mg.Corpus.synthetic(args.docs, seed=42)
    idx = mg.Index(corpus=corpus, ngram_size=2)
    di = idx.device_index
    rng = np.random.default_rng(9)
    words = frequent_words(corpus, min(args.docs, 20_000), 24)
    pairs = [(a, b) for a in words for b in words if a < b]
    picked = [pairs[i] for i in rng.permutation(len(pairs))[: args.queries]]
    while len(picked) < args.queries:
        picked += picked[: args.queries - len(picked)]

    def batch(**order):
        return [Query([a, b], limit=args.limit, descending=True, **order) for a, b in picked]

    def runner(index, queries):
        b = index.prepare(queries)
        rv = _capi.ResultView()

        def run():
            t0 = time.perf_counter()
            b.execute()
            _capi.check(L.mgx_batch_fetch(b._h, C.byref(rv)))
            return (time.perf_counter() - t0) * 1e3
        return b, run

    def compare(pair, reps):
        (ba, ra), (bb, rb) = pair
        for _ in range(2):
            ra()
            rb()
        a_ms, b_ms = [], []
        for _ in range(reps):
            a_ms.append(ra())
            b_ms.append(rb())
        same = all(x.docs.tolist() == y.docs.tolist() and x.total == y.total for x, y in zip(ba.fetch(), bb.fetch()))
        return summary(a_ms), summary(b_ms), same

    out = {"workload": "%d docs, bigram; %d two-term ANDs of frequent words, LIMIT %d DESC" % (args.docs, len(picked), args.limit),
           "pk_sort_general_env": os.environ.get("MGX_PK_SORT_GENERAL")}
    # (i) shuffled numeric keys | an int64 column of the same numbers
    shuffled = rng.permutation(args.docs).astype(np.int64) + 1000
    column = di.add_filter_column(shuffled)
    di.set_primary_keys([b"%d" % v for v in shuffled])
    a, b, same = compare((runner(idx, batch(sort_primary_key=True)), runner(idx, batch(sort_column=column))), args.reps)
    out["shuffled_numeric"] = {"primary_key": a, "int64_column": b, "pages_equal": same,
                               "differ_by_more_than_both_spreads": abs(a["median_ms"] - b["median_ms"]) > a["spread_ms"] + b["spread_ms"]}
    # (ii) monotone keys | the doc-id page
    di.set_primary_keys([b"%d" % (7 + i) for i in range(args.docs)])
    a, b, same2 = compare((runner(idx, batch(sort_primary_key=True)), runner(idx, batch())), args.reps)
    out["monotone"] = {"primary_key": a, "docid_page": b, "pages_equal": same2,
                       "differ_by_more_than_both_spreads": abs(a["median_ms"] - b["median_ms"]) > a["spread_ms"] + b["spread_ms"]}
    ok = same and same2
    # (iii) a delta index: the merge by numbers | by key strings
    if args.delta:
        n_delta = args.delta
        dcorpus = mg.Corpus.synthetic(n_delta, seed=43)
        delta = mg.Index(corpus=dcorpus, ngram_size=2)
        ids = (args.docs + 10 + np.arange(n_delta)).astype(np.uint32)
        _capi.check(L.mgx_index_set_doc_map(delta.device_index._h, ids.ctypes.data, n_delta))
        di.set_primary_key_shortcut(False)
        di.set_primary_keys([b"%d" % v for v in shuffled])
        dkeys = rng.permutation(n_delta) * 97 + 5
        qs = batch(sort_primary_key=True)
        merged = {}
        for name, keys in (("numeric", [b"%d" % v for v in dkeys]), ("string", [b"pk%d" % v for v in dkeys])):
            delta.device_index.set_primary_keys(keys)
            bm, bd = idx.prepare(qs), delta.prepare(qs)
            others = (C.c_void_p * 1)(bd._h.value)
            rv, dv = _capi.ResultView(), _capi.ResultView()

            def run():
                t0 = time.perf_counter()
                bm.execute()
                bd.execute()
                _capi.check(L.mgx_batch_merge_local(bm._h, others, 1, None))
                _capi.check(L.mgx_batch_fetch(bm._h, C.byref(rv)))
                _capi.check(L.mgx_batch_fetch(bd._h, C.byref(dv)))
                return (time.perf_counter() - t0) * 1e3
            for _ in range(2):
                run()
            merged[name] = summary([run() for _ in range(args.reps)])
        out["delta_%d" % n_delta] = merged
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
