#!/usr/bin/env python3
"""Build time of an index's column arrays, host builder (mgx_columns_build, what every write went through) against the
device builder (mgx_columns_build_device), on the same corpus in the same run: the delta sizes of DESIGN.md section 9 (8k and
24k documents) and 1M documents, Corpus.synthetic, bigrams. Device time is the whole call: texts up, kernels, sort, columns
back down into host arrays. Warm runs; the median of --runs. One JSON line per size; the two views are compared as well.
Not used by the driver.

    python tools/bench_build.py [--sizes 8000,24000,1000000] [--runs 11] [--device 0] [--host-threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

ARRAYS = ("key_bytes", "key_off", "offsets", "docids", "tf", "doc_len", "tf_overflow_pos", "tf_overflow_val")
SCALARS = ("n_grams", "n_postings", "first_doc_id", "n_docs", "bm25_doc_count", "bm25_total_len")


def equal(a, b):
    return all(getattr(a, k) == getattr(b, k) for k in SCALARS) and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ARRAYS)


def timed(fn, runs):
    out, ms = None, []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8000,24000,1000000")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host-threads", type=int, default=16, help="threads of the host builder (0: one per hardware thread)")
    args = ap.parse_args()
    mg = entry.load_package()
    if mg._capi.load().mgx_device_count() <= args.device:
        raise SystemExit("needs an MI355X")
    for n in [int(x) for x in args.sizes.split(",")]:
        corpus = mg.Corpus.synthetic(n, seed=42)
        runs = args.runs
        host_fn = lambda: mg.Columns(corpus, 1, 2, 0, True, n_threads=args.host_threads)  # noqa: E731
        dev_fn = lambda: mg.Columns(corpus, 1, 2, 0, True, device=args.device)  # noqa: E731
        timed(host_fn, 2)
        timed(dev_fn, 2)  # (the first call makes the stream and the device allocation that later calls of this size reuse)
        host, host_ms = timed(host_fn, runs)
        dev, dev_ms = timed(dev_fn, runs)
        text_bytes = int(corpus.text_off[-1])
        down = sum(getattr(dev, k).nbytes for k in ("offsets", "docids", "tf", "doc_len", "tf_overflow_pos")) + 8 * dev.n_grams
        print(json.dumps({
            "docs": n, "text_bytes": text_bytes, "windows": int(dev.doc_len.astype(np.int64).sum() - np.count_nonzero(dev.doc_len)),
            "grams": dev.n_grams, "postings": dev.n_postings, "bytes_down": int(down), "runs": runs,
            "host_ms_median": float(np.median(host_ms)), "host_ms_min": float(min(host_ms)),
            "device_ms_median": float(np.median(dev_ms)), "device_ms_min": float(min(dev_ms)),
            "host_over_device": float(np.median(host_ms) / np.median(dev_ms)), "equal": bool(equal(host, dev)),
            "host_threads": args.host_threads,
        }), flush=True)


if __name__ == "__main__":
    main()
