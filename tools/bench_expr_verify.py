"""verify_text on boolean-expression queries (kOpVerifyTree): what the text filter costs a batch.

Workload: 1024 two-level trees (w1 AND w2) OR (w3 AND w4) over words of 4-8 letters out of the 1M-doc synthetic table
(each AND pair out of one document), docid DESC limit 100 — the setting of the kOpVerifyFuzzy measurement in DESIGN.md
section 4. --mode off: no verify_text; exact: verify_text; fuzzy: FUZZY 1 on every leaf (one edit in each word) with
verify_text; fuzzy-off: the same FUZZY trees without it. Prints one JSON line. Run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_expr_verify.py --mode ...` for the kernel times."""
import argparse
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
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--mode", choices=["off", "exact", "fuzzy", "fuzzy-off"], default="exact")
    a = ap.parse_args()
    mg = entry.load_package()
    corpus = mg.Corpus.synthetic(a.docs, seed=42)
    idx = mg.Index(corpus=corpus, first_doc_id=1, ngram_size=2, kanji_ngram_size=0, device=0)
    rng = np.random.default_rng(1)
    fuzzy = 1 if a.mode.startswith("fuzzy") else 0

    def pair():
        while True:
            words = [w for w in corpus.text(int(rng.integers(0, a.docs))).decode().split(" ") if 4 <= len(w) <= 8]
            if len(words) >= 2:
                pick = rng.choice(len(words), 2, replace=False)
                return [words[int(k)] for k in pick]

    def typo(w):
        i = int(rng.integers(1, len(w) - 1))
        ch = "abcdefghijklmnopqrstuvwxyz"[int(rng.integers(0, 26))]
        return w[:i] + ("z" if ch == w[i] else ch) + w[i + 1:]

    qs = []
    for _ in range(a.queries):
        w = pair() + pair()
        if fuzzy:
            w = [typo(x) for x in w]
        qs.append(mg.engine.Query(expr=("or", ("and", w[0], w[1]), ("and", w[2], w[3])), fuzzy=fuzzy,
                                  verify_text=a.mode in ("exact", "fuzzy"), limit=100, descending=True))
    b = idx.prepare(qs)
    b.execute()
    b.fetch_raw()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        b.execute()
        b.fetch_raw()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    res = b.fetch()
    print(json.dumps({"mode": a.mode, "docs": a.docs, "queries": a.queries, "steps": a.steps, "ms_per_batch": round(ms, 3),
                      "candidates": int(sum(r.after_filters for r in res)), "kept": int(sum(r.total for r in res))}))


if __name__ == "__main__":
    main()
