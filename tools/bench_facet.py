#!/usr/bin/env python3
"""FACET in a batch against the one-query path, in one process and one session. Not used by the driver.

    python tools/bench_facet.py [--docs 1000000] [--queries 256] [--reps 5] [--out profiles/facet_batch_measurements.json]

The table: a synthetic corpus with value-id columns of 2, 1000 and 100 000 distinct values (--cardinalities). The queries:
2-term ANDs of frequent words (--dense: the universe, a FACET without search terms), each faceted on every column.
  (a) the one-query path: one mgx_facet_counts call per (query, column) on compiled mgx_query structs;
  (b) one prepared batch with the requests attached: execute -> fetch -> fetch_facets.
(a) and (b) alternate, `--reps` repetitions each after a warm-up; the medians and the spreads (max - min) are reported, and
every count of (b) is compared with (a)'s for equality. (b) is also timed with one column at a time.

MGX_FACET_BALLOT_MAX=<n> (read once per process by the library) moves the cardinality threshold of the kernel's ballot
path: 0 sends every column through LDS atomics. Kernel times come from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/bench_facet.py ...`.
"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense", action="store_true", help="every query is the universe (FACET without search terms)")
    ap.add_argument("--cardinalities", default="2,1000,100000", help="distinct values of each column")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    CARDINALITIES = tuple(int(x) for x in args.cardinalities.split(","))
    mg = entry.load_package()
    _capi, Query = mg._capi, mg.engine.Query
    L = _capi.load()
    corpus = mg.Corpus.synthetic(args.docs, seed=42)
    idx = mg.Index(corpus=corpus, ngram_size=2)
    rng = np.random.default_rng(9)
    cols = []
    for nv in CARDINALITIES:
        ids = rng.integers(0, nv, args.docs).astype(np.uint32)
        cols.append(idx.device_index.add_filter_column(ids.astype(np.int64), None, value_ids=ids, n_values=nv))
    words = frequent_words(corpus, min(args.docs, 20_000), 24)
    pairs = [(a, b) for a in words for b in words if a < b]
    picked = [pairs[i] for i in rng.permutation(len(pairs))[: args.queries]]
    while len(picked) < args.queries:
        picked += picked[: args.queries - len(picked)]

    def search_part(a, b, **more):
        # --dense: NOT(<a term no document holds>) is every document, the search part of a FACET without terms
        return Query(expr=("not", "0909"), **more) if args.dense else Query([a, b], **more)

    def queries(columns):
        return [search_part(a, b, facet_columns=columns) for a, b in picked]

    # (a): the compiled C queries, one call per (query, column)
    cqueries, keep, shells = idx.prepare([search_part(a, b, limit=0) for a, b in picked], into="raw")
    assert all(s is None for s in shells)
    single = [[np.zeros(nv, np.uint64) for nv in CARDINALITIES] for _ in picked]
    matched = C.c_uint64()

    def run_single():
        t0 = time.perf_counter()
        for qi, cq in enumerate(cqueries):
            for ci, col in enumerate(cols):
                _capi.check(L.mgx_facet_counts(idx.device_index._h, C.byref(cq), col, single[qi][ci].ctypes.data,
                                               C.byref(matched)))
        return (time.perf_counter() - t0) * 1e3

    def batch_runner(columns):
        b = idx.prepare(queries(columns))
        rv, fv = _capi.ResultView(), _capi.FacetView()

        def run():
            t0 = time.perf_counter()
            b.execute()
            _capi.check(L.mgx_batch_fetch(b._h, C.byref(rv)))
            _capi.check(L.mgx_batch_fetch_facets(b._h, C.byref(fv)))
            return (time.perf_counter() - t0) * 1e3
        return b, run

    b_all, run_all = batch_runner(cols)
    per_column = [batch_runner([c]) for c in cols]
    for _ in range(2):  # warm-up: arenas, pinned blocks, code objects
        run_single()
        run_all()
        for _, run in per_column:
            run()
    a_ms, b_ms = [], []
    col_ms = [[] for _ in cols]
    for _ in range(args.reps):
        a_ms.append(run_single())
        b_ms.append(run_all())
        for k, (_, run) in enumerate(per_column):
            col_ms[k].append(run())
    # equality of every count
    got = b_all.fetch()
    compared = mismatched = 0
    total_matched = 0
    for qi, r in enumerate(got):
        total_matched += r.total
        for ci in range(len(cols)):
            compared += len(single[qi][ci])
            mismatched += int(np.count_nonzero(r.facets[ci] != single[qi][ci]))
    a, b = summary(a_ms), summary(b_ms)
    out = {
        "workload": "%d docs, bigram; %d %s, each faceted on columns of %s values"
                    % (args.docs, len(picked), "universe queries" if args.dense else "two-term ANDs of frequent words",
                       "/".join(str(c) for c in CARDINALITIES)),
        "ballot_max_env": os.environ.get("MGX_FACET_BALLOT_MAX"),
        "matched_documents_mean": total_matched / len(got),
        "single_calls": {"calls": len(picked) * len(cols), **a},
        "one_batch": b,
        "one_batch_one_column": {str(nv): summary(ms) for nv, ms in zip(CARDINALITIES, col_ms)},
        "speedup_of_medians": a["median_ms"] / b["median_ms"],
        "batch_beats_single_calls_by_more_than_both_spreads": a["median_ms"] - b["median_ms"] > a["spread_ms"] + b["spread_ms"],
        "counts_compared": compared,
        "counts_mismatched": mismatched,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0 if mismatched == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
