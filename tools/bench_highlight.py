"""HIGHLIGHT on the device against the only path a caller had before it: mgx_index_read_text per page entry plus the host
highlighter (mgxt_highlight_generate) for the same pages.

Workload: 1024 x 3-term AND + BM25 top-10 on the synthetic table, highlight on for every query at default options.
Prints one JSON line. Run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_highlight.py` for the kernel
times (highlight_kernel, and the batch's kernels with and without it: --mode on / off runs one of the two only).

--original identity|mapped attaches original texts made from the synthetic corpus (mgx_index_attach_original_text), so
that the batch launches highlight_original_kernel: `identity` upper-cases every word's first letter; `mapped` also writes
every 'e' inside a word as a full-width letter (three bytes) and "fi", "fl", "ff", "ij", "lj", "nj" as their one-character forms, which NFKC expands,
so that the documents need a real map (the index then normalizes nfkc + narrow + lower). The host path then also reads the original
per page entry and runs mgxt_highlight_generate_original."""
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


# two lower-case letters -> one character that NFKC expands back to them: ligatures and digraph letters
DIGRAPHS = [(b"fi", "\ufb01".encode()), (b"fl", "\ufb02".encode()), (b"ff", "\ufb00".encode()), (b"ij", "\u0133".encode()),
            (b"lj", "\u01c9".encode()), (b"nj", "\u01cc".encode())]


def make_originals(corpus, mapped):
    """Originals of the synthetic (lower-case ASCII) corpus, such that NormalizeText(nfkc, narrow, lower) of an original
    is the corpus text: every word's first letter upper-cased; `mapped`: also every other 'e' as the full-width U+FF45
    (three bytes, one code point) and every DIGRAPHS pair inside a document as its one character, which NFKC expands to
    two code points — so the two normalized code points both map to the one original code point, and every later pair of
    the document is shifted: a real map, one pair per normalized code point."""
    total = int(corpus.text_off[-1])
    text = np.array(corpus.text_bytes[:total], dtype=np.uint8)
    off = corpus.text_off.astype(np.int64)
    first = np.zeros(total, dtype=bool)
    first[1:] = text[:-1] == 0x20
    first[off[:-1][off[:-1] < total]] = True
    first &= (text >= 0x61) & (text <= 0x7A)
    upper = np.where(first, text - 32, text).astype(np.uint8)
    n_docs = len(off) - 1
    if not mapped:
        return {"bytes": np.concatenate([upper, np.zeros(16, np.uint8)]), "off": off.astype(np.uint64), "pairs": None,
                "map_off": np.zeros(n_docs + 1, np.uint64)}
    doc_of = np.repeat(np.arange(n_docs), np.diff(off))
    same_doc = np.zeros(total, dtype=bool)
    same_doc[:-1] = doc_of[:-1] == doc_of[1:]
    claimed = np.zeros(total, dtype=bool)
    lig_i = np.zeros(total, dtype=bool)  # the second letter of a digraph: it has no code point of its own in the original
    glyphs = []                          # (mask of the first letters, the character's UTF-8 bytes)
    for pair, utf8 in DIGRAPHS:
        cand = np.zeros(total, dtype=bool)
        cand[:-1] = (upper[:-1] == pair[0]) & (upper[1:] == pair[1]) & same_doc[:-1] & ~claimed[:-1] & ~claimed[1:]
        cand[1:] &= ~cand[:-1]           # ("fff": the first two letters only)
        claimed |= cand
        claimed[1:] |= cand[:-1]
        lig_i[1:] |= cand[:-1]
        glyphs.append((cand, utf8))
    wide = (upper == 0x65) & ~first & ~claimed
    glyphs.append((wide, b"\xef\xbd\x85"))
    width = np.ones(total, dtype=np.int64)
    width[lig_i] = 0
    for mask, utf8 in glyphs:
        width[mask] = len(utf8)
    start = np.zeros(total + 1, dtype=np.int64)
    np.cumsum(width, out=start[1:])
    out = np.zeros(int(start[-1]) + 16, dtype=np.uint8)
    plain = ~(claimed | wide)
    out[start[:-1][plain]] = upper[plain]
    for mask, utf8 in glyphs:
        w = start[:-1][mask]
        for k, byte in enumerate(utf8):
            out[w + k] = byte
    # code points of the original before each normalized code point (the ligature's 'i' shares its 'f''s)
    cps = np.zeros(total + 1, dtype=np.int64)
    np.cumsum(~lig_i, out=cps[1:])
    before = cps[:-1] - lig_i
    local = (before - cps[off[:-1]][doc_of]).astype(np.uint32)
    pairs = np.ascontiguousarray(np.stack([local, local + 1], axis=1))
    return {"bytes": out, "off": start[off].astype(np.uint64), "pairs": pairs, "map_off": off.astype(np.uint64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mode", choices=["both", "on", "off"], default="both")
    ap.add_argument("--host-path", type=int, default=1, help="time the read_text + host highlighter path too")
    ap.add_argument("--original", choices=["none", "identity", "mapped"], default="none")
    a = ap.parse_args()
    mg = entry.load_package()
    L = mg._capi.load()
    L.mgx_index_read_text.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    corpus = mg.Corpus.synthetic(a.docs, seed=42)
    idx = mg.Index(corpus=corpus, first_doc_id=1, ngram_size=2, kanji_ngram_size=0, device=0,
                   normalize_width="keep" if a.original == "none" else "narrow")
    idx.ensure_text()
    orig = None
    if a.original != "none":
        orig = make_originals(corpus, a.original == "mapped")
        n_docs = corpus.n_docs
        kind = np.full(n_docs, mg._capi.ORIG_MAPPED if a.original == "mapped" else mg._capi.ORIG_IDENTITY, np.uint8)
        mg._capi.check(L.mgx_index_attach_original_text(
            idx.device_index._h, orig["bytes"].ctypes.data, orig["off"].ctypes.data, kind.ctypes.data,
            orig["pairs"].ctypes.data if orig["pairs"] is not None else None, orig["map_off"].ctypes.data))
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

    res = {"docs": a.docs, "queries": a.queries, "steps": a.steps, "original": a.original}
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
                    if orig is None:
                        L.mgxt_highlight_generate(buf, n.value, arr, lens, len(terms), 100, 3, b"<em>", 4, b"</em>", 5,
                                                  out, len(out), C.byref(m))
                    else:  # the original and its map come from the host's own store
                        s = doc - 1
                        o0, o1 = int(orig["off"][s]), int(orig["off"][s + 1])
                        p0, p1 = int(orig["map_off"][s]), int(orig["map_off"][s + 1])
                        L.mgxt_highlight_generate_original(
                            orig["bytes"][o0:o1].tobytes(), o1 - o0, buf, n.value, int(kind[s]),
                            orig["pairs"][p0:p1].ctypes.data if p1 > p0 else None, p1 - p0, arr, lens, len(terms), 100, 3,
                            b"<em>", 4, b"</em>", 5, C.cast(out, C.c_void_p), len(out), C.byref(m))
                    mismatches += out.raw[:m.value] != snippet
            res["ms_host_path"] = (time.perf_counter() - t0) * 1e3
            res["host_path_mismatches"] = int(mismatches)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
