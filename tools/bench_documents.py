#!/usr/bin/env python3
"""Page documents on the device against a batch without them and against the per-value reads they replace, in one
process and one session. Not used by the driver.

    python tools/bench_documents.py [--docs 1000000] [--queries 1024] [--limit 10] [--reps 7] [--out profiles/documents_measurements.json]

The table is tools/bench_facet.py's: a synthetic corpus with two filter columns, and a primary key per document. The
queries: SORT _score two-term ANDs of frequent words, top `--limit`. Timed, alternating, `--reps` repetitions each after three
warm-up rounds (execute -> fetch [-> fetch_documents]):
  (a) the batch without a request: what the same queries cost before the rows are asked for (compare this figure across
      commits for the unrequested batch);
  (b) the same batch with the request (keys + two columns);
  (c) the mgx_index_filter_column_read calls the request replaces: one per (page entry, column) of (a)'s pages.
`--plain-only` times (a) alone through entry points every commit has, so that the same file run on the parent commit's
tree gives the parent's figure. Medians and spreads (max - min) are reported; every value of (b) is compared with (c)'s and every key with the host's.
Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_documents.py ...`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402
from bench_facet import frequent_words  # noqa: E402


def summary(ms):
    return {"median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "runs_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--plain-only", action="store_true",
                    help="time (a) alone, through entry points every commit has: the figure to compare across commits")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mg = entry.load_package()
    _capi, Query = mg._capi, mg.engine.Query
    L = _capi.load()
    corpus = mg.Corpus.synthetic(args.docs, seed=42)
    idx = mg.Index(corpus=corpus, ngram_size=2)
    di = idx.device_index
    rng = np.random.default_rng(9)
    col_a = rng.integers(-1000, 1000, args.docs).astype(np.int64)
    nul_a = rng.random(args.docs) < 0.1
    col_b = rng.integers(0, 1 << 40, args.docs).astype(np.uint64)
    cols = [di.add_filter_column(col_a, nul_a), di.add_filter_column(col_b)]
    keys = [b"pk%d" % v for v in rng.permutation(args.docs)]
    if not args.plain_only:
        di.attach_primary_key_bytes(keys)
    words = frequent_words(corpus, min(args.docs, 20_000), 48)
    pairs = [(a, b) for a in words for b in words if a < b]
    picked = [pairs[i] for i in rng.permutation(len(pairs))[: args.queries]]
    while len(picked) < args.queries:
        picked += picked[: args.queries - len(picked)]

    def queries(documents):
        more = {} if documents is None else {"documents": documents}
        return [Query([a, b], sort_score=True, limit=args.limit, **more) for a, b in picked]

    plain = idx.prepare(queries(None))
    rv = _capi.ResultView()
    if args.plain_only:
        for _ in range(3):
            plain.execute()
            _capi.check(L.mgx_batch_fetch(plain._h, C.byref(rv)))
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            plain.execute()
            _capi.check(L.mgx_batch_fetch(plain._h, C.byref(rv)))
            ms.append((time.perf_counter() - t0) * 1e3)
        out = {"workload": "%d docs, bigram; %d SORT _score two-term ANDs of frequent words, top %d; no request"
                           % (args.docs, len(picked), args.limit), "batch_without_request": summary(ms)}
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return 0
    asked = idx.prepare(queries(cols))
    dv = _capi.DocumentView()

    def run(batch, with_documents):
        t0 = time.perf_counter()
        batch.execute()
        _capi.check(L.mgx_batch_fetch(batch._h, C.byref(rv)))
        if with_documents:
            _capi.check(L.mgx_batch_fetch_documents(batch._h, C.byref(dv)))
        return (time.perf_counter() - t0) * 1e3

    pages = [r.docs.tolist() for r in idx.search_batch(queries(None))]
    bits, nul = C.c_uint64(), C.c_int()
    reads = {}

    def run_reads():
        t0 = time.perf_counter()
        for page in pages:
            for doc in page:
                for c in cols:
                    _capi.check(L.mgx_index_filter_column_read(di._h, c, doc, C.byref(bits), C.byref(nul), None))
                    reads[(doc, c)] = (bits.value, bool(nul.value))
        return (time.perf_counter() - t0) * 1e3

    for _ in range(3):  # warm-up: arenas, pinned blocks, code objects (two rounds left the first timed one 1.9 ms high)
        run(plain, False)
        run(asked, True)
    run_reads()
    a_ms, b_ms, c_ms = [], [], []
    for _ in range(args.reps):
        a_ms.append(run(plain, False))
        b_ms.append(run(asked, True))
    for _ in range(min(args.reps, 3)):
        c_ms.append(run_reads())
    asked.execute()
    got = asked.fetch()
    compared = mismatched = 0
    for page, r in zip(pages, got):
        assert r.docs.tolist() == page
        for doc, d in zip(page, r.documents):
            compared += 1 + len(cols)
            mismatched += d is None or d.key != keys[doc - 1]
            for k, c in enumerate(cols):
                v, n = reads[(doc, c)]
                mismatched += d is None or bool((d.null_mask >> k) & 1) != n or (not n and int(d.values[k]) != v)
    a, b, c = summary(a_ms), summary(b_ms), summary(c_ms)
    out = {
        "workload": "%d docs, bigram; %d SORT _score two-term ANDs of frequent words, top %d; keys + 2 columns"
                    % (args.docs, len(picked), args.limit),
        "page_entries": sum(len(p) for p in pages),
        "batch_without_request": a,
        "batch_with_request": b,
        "added_by_the_request_ms": b["median_ms"] - a["median_ms"],
        "filter_column_reads": {"calls": sum(len(p) for p in pages) * len(cols), **c},
        "values_compared": compared,
        "values_mismatched": int(mismatched),
    }
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0 if mismatched == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
