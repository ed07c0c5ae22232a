"""Worker of tests/test_gpu_fast_schedule.py, and the home of the table and the queries that module and this worker
share. The knobs that cut a fast-path query into work items and order them (MGX_ITEM_COST, MGX_WANT_ITEMS,
MGX_SEED_TILES, ... — DESIGN.md "Schedule knobs") are read once per process, so every forced schedule runs in a process
of its own: this script, started with the knobs in its environment.

    python fast_schedule_worker.py OUT.npz

builds the table, runs both batches twice, prints the [mgx] verbose lines (stderr) and writes totals, funnel counters,
page docids and fp64 scores of every query and every execute to OUT.npz. It imports no oracle: the parent holds the
expected values and compares.

The table: 64 tiles, the last one partial — the smallest table whose fast-path queries get a seed item (CutItems) —
made of the synthetic corpus with planted documents spliced in at three places: inside tiles 0-7 (what a seed item
covers), in a middle tile, and in the final partial tile. A planted document is

    <head: the three densest grams once> " " <a rare gram n times> <padding of dense grams up to a target length>

with n = 1..40 (tf 14, 15, 16: around the saturated nibble) and lengths of exactly 254, 255, 256 and 400 code points
(around the escape value of the byte length column). Three rare grams:

    k5  the same texts at all three places, each twice: tie classes of six that straddle the seed's tiles, the middle
        and the last tile;
    q7  the same, plus 120 documents only in the last tile that beat every other (n = 41..160): the whole page of a q7
        query lives in the tile that runs last;
    j4  the same, plus those 120 only inside tiles 0-7: the whole page is known to the seed, everything after it runs
        against the final bound.

Those documents saturate the nibble wherever they rank first, and a saturated nibble's block-max byte is the largest
there is. So each place also gets 120 copies each of three short texts that hold the densest gram 13 times, the two
densest 7 times each, the three densest 4 times each (TIE_TEXTS): the best unsaturated scores of the heavy queries over
those grams. More copies than the largest page sit inside the seed's tiles, so the seed publishes their score as the
query's bound; the page itself is the copies with the largest docids, all in the last tile, each of them EQUAL to the
bound it is held against: a quantised bound a hair too low, or a comparison that drops ties, loses the whole page."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from pkg import mg  # noqa: E402

Query = mg.engine.Query

TILE = 16384
N_TILES = 64
N_DOCS = 63 * TILE + 5000
SEED_TILES = 8                       # CutItems: min(16, (64 / 8) & ~7)
PLACES = {"seed": (0, SEED_TILES * TILE), "middle": (31 * TILE, 32 * TILE), "last": (63 * TILE, N_DOCS)}
RARE = ("k5", "q7", "j4")
LADDER = (1, 2, 3, 5, 8, 13, 14, 15, 16, 17, 25, 40)
LENGTHS = (0, 254, 255, 256, 400)    # 0: no padding
OTHER_PARAMS = (2.0, 0.3)            # the batch away from the default (k1, b)
TIE_COPIES = 120                     # per place: more than the largest offset + limit (107)
DENSE_THRESHOLD = 1e-4               # grams of 104 documents and more are bitmaps: the rare grams too (default: 1 / 256)
COUNTERS = ("total_candidates", "after_intersection", "after_not", "after_filters")


def dense_grams_of(text_bytes, n):
    """The n most frequent letter bigrams of a run of corpus bytes, most frequent first."""
    b = np.asarray(text_bytes, dtype=np.int64)
    pair = b[:-1] * 256 + b[1:]
    letters = (b >= 97) & (b <= 122)
    count = np.bincount(pair[letters[:-1] & letters[1:]], minlength=65536)
    top = np.argsort(-count, kind="stable")[:n]
    return [bytes([int(p) >> 8, int(p) & 255]).decode() for p in top]


def planted_text(dense, rare, n, length):
    head = dense[0] + dense[1] + dense[2]
    text = head + " " + rare * n
    if length:
        unit = " " + dense[3] + dense[4] + dense[5] + dense[6] + dense[7]
        text += (unit * (length // len(unit) + 1))[: length - len(text)]
        assert len(text) == length
    return text


def tie_texts(dense):
    return [" ".join([dense[0]] * 13), " ".join([dense[0], dense[1]] * 7), " ".join([dense[0], dense[1], dense[2]] * 4)]


def build_corpus():
    """-> (mg.Corpus, {place: sorted slots of its planted documents}, the eight grams the planted documents are made of:
    [0..2] in every one, [3..7] in the padded ones); deterministic."""
    base = mg.Corpus.synthetic(N_DOCS, seed=29)
    off = base.text_off.astype(np.int64)
    data = base.text_bytes[: int(off[-1])]
    dense = dense_grams_of(data[: int(off[20000])], 8)
    rng = np.random.default_rng(2029)
    plant = {}  # slot -> text
    where = {}
    for place, (lo, hi) in PLACES.items():
        texts = []
        for rare in RARE:
            for n in LADDER:
                for length in LENGTHS:
                    texts += [planted_text(dense, rare, n, length)] * 2
        if place == "last":
            texts += [planted_text(dense, "q7", n, 0) for n in range(41, 161)]
        if place == "seed":
            texts += [planted_text(dense, "j4", n, 0) for n in range(41, 161)]
        for t in tie_texts(dense):
            texts += [t] * TIE_COPIES
        slots = rng.choice(np.arange(lo, hi - 1), size=len(texts) - 1, replace=False).tolist() + [hi - 1]
        order = rng.permutation(len(texts)).tolist()
        for s, k in zip(slots, order):  # (the place's last slot is planted too: the table's last, partial word)
            plant[int(s)] = texts[k]
        where[place] = sorted(int(s) for s in slots)
    # splice: the runs of untouched documents stay slices of the synthetic bytes
    chunks, lengths = [], np.diff(off)
    at = 0
    for s in sorted(plant):
        chunks.append(data[int(off[at]):int(off[s])])
        t = np.frombuffer(plant[s].encode(), dtype=np.uint8)
        chunks.append(t)
        lengths[s] = len(t)
        at = s + 1
    chunks.append(data[int(off[at]):])
    chunks.append(np.zeros(16, np.uint8))
    new_off = np.zeros(N_DOCS + 1, dtype=np.uint64)
    new_off[1:] = np.cumsum(lengths).astype(np.uint64)
    return mg.Corpus(np.concatenate(chunks), new_off), where, dense


def filter_docs():
    """The filter row: about 70 % of the documents, the last one among them."""
    m = np.random.default_rng(17).random(N_DOCS) < 0.7
    m[-1] = True
    return (np.nonzero(m)[0] + 1).astype(np.uint32)


def dense_terms(columns, n=16):
    sizes = np.diff(columns.offsets.astype(np.int64))
    g = [i for i in np.argsort(-sizes, kind="stable").tolist() if b" " not in columns.gram(i)][:n]
    return [columns.gram(i).decode() for i in g], [int(sizes[i]) for i in g]


def make_queries(P, columns, row):
    """-> (the batch at the default (k1, b), the batch at OTHER_PARAMS): SORT _score queries over single-gram terms, all of
    a shape the fast path takes. `P` = the planted documents' grams (build_corpus), `row` = the id of the registered
    filter row."""
    D, _ = dense_terms(columns)
    pages = [(10, 0), (100, 7), (37, 5), (1, 0), (100, 0), (10, 5), (37, 0), (10, 7)]
    rng = np.random.default_rng(64)
    a = []
    k = 0

    def add(terms, nots=(), filt=None, desc=True, page=None):
        nonlocal k
        limit, offset = page if page is not None else pages[k % len(pages)]
        k += 1
        a.append(Query(list(terms), list(nots), filters=[filt] if filt is not None else [], sort_score=True, limit=limit,
                       offset=offset, descending=desc))

    # the rare grams alone and with dense grams: 1..5 scored terms, every page shape
    for rare in RARE:
        add([rare])
        add([rare], page=(1, 0))
        add([rare, P[0]])
        add([rare, P[1], P[2]])
        add([P[3], rare, P[4], P[0]])
        add([P[0], P[5], P[6], rare, P[7]])
    add(["q7"], page=(100, 7))
    add(["j4"], page=(100, 7))
    add(["k5", P[3]], page=(100, 7))
    # the densest grams together: est_density >= 0.05 (heavy queries: the re-mask of a tile's second half)
    add([D[0]], page=(100, 7))
    add([D[0], D[1]], page=(10, 0))
    add([D[0], D[1]], page=(37, 5))
    add([D[0], D[2]], page=(100, 0))
    add([D[1], D[0], D[2]], page=(10, 5))
    add([D[0], D[1], D[2]], page=(1, 0))
    # seeded mixes of dense grams, 1..5 terms
    for n_terms in (1, 2, 3, 4, 5):
        for _ in range(2):
            add([D[int(i)] for i in rng.choice(len(D), size=n_terms, replace=False)])
    # NOT terms and the filter row: the and-not and filter operand codes
    add([D[0], D[1]], nots=[D[6]])
    add(["q7", P[0]], nots=[P[7]])
    add(["k5"], nots=["j4", P[6]])
    add([D[2], D[4], D[5]], nots=[D[1]])
    add([D[0], D[3]], filt=(row, False))
    add(["q7"], filt=(row, False))
    add(["k5", P[1]], filt=(row, True))
    add([D[1], D[2]], nots=[D[8]], filt=(row, False))
    # ASC: the same schedule, no pruning
    add(["k5"], desc=False)
    add([D[0], D[1]], desc=False)
    add(["j4", P[2], P[3]], desc=False)
    add([D[4], D[6]], nots=[D[0]], desc=False)
    k1, b = OTHER_PARAMS
    picks = [0, 1, 3, 5, 6, 8, 11, 17, 19, 21, 22, 37, 40, 45]
    other = [Query(a[i].terms, a[i].not_terms, filters=a[i].filters, sort_score=True, limit=a[i].limit, offset=a[i].offset,
                   descending=a[i].descending, k1=k1, b=b) for i in picks]
    return a, other


def run_batches(index, batches, executes=2):
    """Every batch prepared once and executed `executes` times -> {name: array} for np.savez: per batch B and execute
    E, "bB_eE_counts" [n][5] (total and the four funnel counters), "bB_eE_len" [n], "bB_eE_docs" / "bB_eE_scores" (the
    pages, concatenated)."""
    out = {}
    for bi, qs in enumerate(batches):
        batch = index.prepare(qs)
        for e in range(executes):
            batch.execute()
            got = batch.fetch()
            key = "b%d_e%d_" % (bi, e)
            out[key + "counts"] = np.asarray([[g.total] + [int(getattr(g, c)) for c in COUNTERS] for g in got], np.int64)
            out[key + "len"] = np.asarray([len(g.docs) for g in got], np.int64)
            out[key + "docs"] = np.concatenate([g.docs.astype(np.uint32) for g in got])
            out[key + "scores"] = np.concatenate([g.scores.astype(np.float64) for g in got])
    return out


def main():
    os.environ["MGX_VERBOSE"] = "1"
    t0 = time.time()
    corpus, _, P = build_corpus()
    index = mg.Index(corpus=corpus, ngram_size=2, kanji_ngram_size=0, dense_threshold=DENSE_THRESHOLD)
    row = index.device_index.add_filter_bitmap(filter_docs())
    t1 = time.time()
    out = run_batches(index, make_queries(P, index.columns, row))
    np.savez(sys.argv[1], **out)
    print("fast_schedule_worker: build %.2f s, batches %.2f s" % (t1 - t0, time.time() - t1))


if __name__ == "__main__":
    main()
