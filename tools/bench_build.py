#!/usr/bin/env python3
"""Build time of an index's column arrays, host builder (mgx_columns_build, what every write went through) against the
device builder (mgx_columns_build_device), on the same corpus in the same run: the delta sizes of DESIGN.md section 9 (8k and
24k documents) and 1M documents, Corpus.synthetic, bigrams. Device time is the whole call: texts up, kernels, sort, columns
back down into host arrays. Warm runs; the median of --runs. One JSON line per size; the two views are compared as well.
Not used by the driver.

    python tools/bench_build.py [--sizes 8000,24000,1000000] [--runs 11] [--device 0] [--host-threads 16]

--index: end to end instead, three legs that each finish in a serving device index with the texts attached:
  A  host columns (mgx_columns_build) + mgx_index_create + mgx_index_attach_text
  B  device columns (mgx_columns_build_device) + the same two calls
  C  mgx_index_build_device: the postings and the texts never come back to the host
B and C alternate run by run; each gets 2 warm-ups, then the median and min / max of --runs. One JSON line per size, with the
host-to-device and device-to-host bytes of each leg computed from the shapes, and whether C's median lies below B's
minimum (the expectation at 1M documents) and not above B's maximum (at delta sizes).

    python tools/bench_build.py --index [--sizes ...] [--runs 11] [--host-runs 3]
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


def index_legs(mg, args, n):
    """One JSON line: legs A, B, C at n documents."""
    corpus = mg.Corpus.synthetic(n, seed=42)
    dev = args.device

    laps = []  # (columns, mgx_index_create, mgx_index_attach_text) ms of every A / B run

    def two_calls(build):
        t0 = time.perf_counter()
        cols = build()
        t1 = time.perf_counter()
        idx = mg.DeviceIndex(cols, dev)
        t2 = time.perf_counter()
        idx.attach_text(corpus)
        laps.append((1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (time.perf_counter() - t2)))
        return cols, idx

    leg_a = lambda: two_calls(lambda: mg.Columns(corpus, 1, 2, 0, True, n_threads=args.host_threads))  # noqa: E731
    leg_b = lambda: two_calls(lambda: mg.Columns(corpus, 1, 2, 0, True, device=dev))  # noqa: E731
    leg_c = lambda: mg.DeviceIndex.build_resident(corpus, 1, 2, 0, True, dev, 0.0, attach_text=True)  # noqa: E731
    for _ in range(2):  # (each result is released before the next build: one index of this size on the device at a time)
        leg_b()
        leg_c()
    b_ms, c_ms = [], []
    del laps[:]
    for _ in range(args.runs):  # B and C alternate
        for fn, ms in ((leg_b, b_ms), (leg_c, c_ms)):
            t0 = time.perf_counter()
            out = fn()
            ms.append(1e3 * (time.perf_counter() - t0))
            del out
    b_laps = np.median(np.asarray(laps), axis=0).round(3).tolist()
    timed(leg_a, 1)
    _, a_ms = timed(leg_a, args.host_runs)
    (cols_b, idx_b), (cols_c, idx_c) = leg_b(), leg_c()
    same = all(getattr(cols_b, k) == getattr(cols_c, k) for k in SCALARS) and \
        all(np.array_equal(getattr(cols_b, k), getattr(cols_c, k)) for k in ARRAYS if k not in ("docids", "tf")) and \
        idx_b.memory_bytes() == idx_c.memory_bytes()
    for g in np.argsort(-np.diff(cols_b.offsets.astype(np.int64)))[:8].tolist():
        d, t = idx_c.read_postings(g)
        lo, hi = int(cols_b.offsets[g]), int(cols_b.offsets[g + 1])
        same = same and np.array_equal(d, cols_b.docids[lo:hi]) and np.array_equal(t, cols_b.tf[lo:hi])
    # bytes over the bus, from the shapes: G grams, P postings, N documents, T text bytes, V overflow entries
    G, P, N, T, V = cols_b.n_grams, cols_b.n_postings, n, int(corpus.text_off[-1] - corpus.text_off[0]), len(cols_b.tf_overflow_pos)
    tiles = (N + 16383) // 16384
    derived = 4 * G + 8 * (G + 1)  # skip rows and the posting offsets (row lists and bitmap bounds come on top, by density)
    up_index = 5 * P + 4 * N + 16384 * tiles + 12 * V + derived
    up_text = T + 8 * (N + 1)
    dict_down = 8 * G + 8 * G + 4 * N + 8 * V + 12
    stat = lambda ms: {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}  # noqa: E731
    print(json.dumps({
        "mode": "index", "docs": n, "text_bytes": T, "grams": G, "postings": P, "runs": args.runs, "host_runs": args.host_runs,
        "A_host_columns_ms": stat(a_ms), "B_device_columns_ms": stat(b_ms), "C_resident_ms": stat(c_ms),
        "A_bytes": {"h2d": up_index + up_text, "d2h": 0},
        "B_bytes": {"h2d": up_text + up_index + up_text, "d2h": dict_down + 5 * P},
        "C_bytes": {"h2d": up_text + 12 * V + derived, "d2h": dict_down},
        "B_laps_ms_columns_create_attach": b_laps,
        "B_over_C": float(np.median(b_ms) / np.median(c_ms)),
        "C_median_below_B_min": bool(np.median(c_ms) < min(b_ms)), "C_median_not_above_B_max": bool(np.median(c_ms) <= max(b_ms)),
        "equal": bool(same), "host_threads": args.host_threads,
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8000,24000,1000000")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host-threads", type=int, default=16, help="threads of the host builder (0: one per hardware thread)")
    ap.add_argument("--index", action="store_true", help="end to end to a serving index with texts: legs A, B, C")
    ap.add_argument("--host-runs", type=int, default=3, help="--index: runs of leg A (the host builder is slow at 1M documents)")
    args = ap.parse_args()
    mg = entry.load_package()
    if mg._capi.load().mgx_device_count() <= args.device:
        raise SystemExit("needs an MI355X")
    if args.index:
        for n in [int(x) for x in args.sizes.split(",")]:
            index_legs(mg, args, n)
        return
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
