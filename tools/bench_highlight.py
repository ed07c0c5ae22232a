"""HIGHLIGHT on the device against the only path a caller had before it: mgx_index_read_text per page entry plus the host
highlighter (mgxt_highlight_generate) for the same pages.

Workload: 1024 x 3-term AND + BM25 top-10 on the synthetic table, highlight on for every query at default options.
Prints one JSON line. Run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_highlight.py` for the kernel
times (highlight_kernel, and the batch's kernels with and without it: --mode on / off runs one of the two only)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mode", choices=["both", "on", "off"], default="both")
    ap.add_argument("--host-path", type=int, default=1, help="time the read_text + host highlighter path too")
    a = ap.parse_args()
    mg = entry.load_package()
    L = mg._capi.load()
    L.mgx_index_read_text.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    corpus = mg.Corpus.synthetic(a.docs, seed=42)
    idx = mg.Index(corpus=corpus, first_doc_id=1, ngram_size=2, kanji_ngram_size=0, device=0)
    idx.ensure_text()
    cols = idx.columns
    sizes = np.diff(cols.offsets.astype(np.int64))
    letters = [g for g in range(cols.n_grams) if b" " not in cols.gram(g)]
    top = [cols.gram(g).decode() for g in sorted(letters, key=lambda g: -sizes[g])[:64]]
    rng = np.random.default_rng(1)

    def queries(highlight):
        out = []
        for _ in range(a.queries):
            t = rng.choice(len(top), 3, replace=False)
            out.append(mg.engine.Query([top[i] for i in t], sort_score=True, limit=10, highlight=highlight))
        return out

    def run(highlight):
        rng.bit_generator.state = np.random.default_rng(1).bit_generator.state
        b = idx.prepare(queries(highlight))
        for _ in range(3):
            b.execute()
            b.fetch_raw()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            b.execute()
            b.fetch_raw()
        dt = (time.perf_counter() - t0) / a.steps
        return b, dt * 1e3

    res = {"docs": a.docs, "queries": a.queries, "steps": a.steps}
    if a.mode in ("both", "off"):
        _, res["ms_per_batch_off"] = run(None)
    if a.mode in ("both", "on"):
        b, res["ms_per_batch_on"] = run(True)
        t0 = time.perf_counter()
        results = b.fetch()
        res["ms_fetch_and_render"] = (time.perf_counter() - t0) * 1e3
        res["entries"] = sum(len(r.docs) for r in results)
        if a.host_path:
            # the parent's only path: two blocking copies per page entry, then the host highlighter
            rng.bit_generator.state = np.random.default_rng(1).bit_generator.state  # the batch's own queries again
            qs = queries(True)
            buf = C.create_string_buffer(1 << 16)
            out = C.create_string_buffer(1 << 16)
            n = C.c_uint64(0)
            m = C.c_size_t(0)
            mismatches = 0
            t0 = time.perf_counter()
            for q, r in zip(qs, results):
                terms = mg.engine.build_highlight_terms(q.terms)
                arr = (C.c_char_p * len(terms))(*terms)
                lens = (C.c_size_t * len(terms))(*[len(t) for t in terms])
                for doc, snippet in zip(r.docs.tolist(), r.snippets):
                    mg._capi.check(L.mgx_index_read_text(idx.device_index._h, doc, buf, len(buf), C.byref(n)))
                    L.mgxt_highlight_generate(buf, n.value, arr, lens, len(terms), 100, 3, b"<em>", 4, b"</em>", 5, out,
                                              len(out), C.byref(m))
                    mismatches += out.raw[:m.value] != snippet
            res["ms_host_path"] = (time.perf_counter() - t0) * 1e3
            res["host_path_mismatches"] = int(mismatches)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
