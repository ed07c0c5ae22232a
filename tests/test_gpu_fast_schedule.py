"""-m gpu: the fast path's item schedule (CutItems / ScheduleItems), its seed bound and the layout of its block-max
bounds, on the smallest table whose queries get seed items: 64 tiles, the last one partial, with planted documents
inside the seed's tiles, in a middle tile and in the last tile (fast_schedule_worker.py describes them). One set of
SORT _score queries that all take bitmap_score_kernel — 1 to 5 scored terms, limits 1 / 10 / 37 / 100 with offsets
0 / 5 / 7, DESC and ASC, NOT terms, a filter row, the densest grams together, and a second batch at another (k1, b): a
batch's fast path takes one parameter set — is held against the oracle bit for bit: totals, the four funnel counters,
page docids and fp64 scores, on both executes of each prepared batch.

The same table and queries then run under forced schedules, each in a process of its own (the knobs are read once per
process). Results do not depend on the schedule, so every child must reproduce the oracle's values, and every
configuration proves from the [mgx] verbose lines that it ran the schedule it asked for.

Measured on an MI355X: the module takes 17 s (8.5 s of it the table and the oracle's answers), one
default-configuration worker 3.3 s from start to exit (CHILD_TIMEOUT is five times that)."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import fast_schedule_worker as W
from gpu_util import Pair
from pkg import ROOT

pytestmark = pytest.mark.gpu
Query = W.Query

CHILD_TIMEOUT = 17
KNOBS = ("MGX_ITEM_COST", "MGX_ITEM_MATCHES", "MGX_MAX_ITEM_TILES", "MGX_WANT_ITEMS", "MGX_SEED_TILES", "MGX_SORT_TILES",
         "MGX_XCD_AFFINITY", "MGX_HEAVY_DENSITY", "MGX_HEAVY_SQUEEZE", "MGX_FINE_DENSITY")
CONFIGS = {
    # one 8-tile seed plus seven 8-tile items per query; every bitmap gram has per-quarter bounds
    "shred": dict(MGX_ITEM_COST="1", MGX_WANT_ITEMS="100000000", MGX_FINE_DENSITY="0", MGX_XCD_AFFINITY="0",
                  MGX_SORT_TILES="8"),
    # a seed plus one 56-tile item (each wave walks seven tiles against the seed's bound); per-word bounds only; every
    # item in band 0
    "long": dict(MGX_ITEM_COST="1000000", MGX_WANT_ITEMS="1", MGX_FINE_DENSITY="2", MGX_HEAVY_DENSITY="0",
                 MGX_HEAVY_SQUEEZE="0"),
    # no seed: eight 8-tile items per query, the first at tile 0
    "noseed": dict(MGX_SEED_TILES="0", MGX_ITEM_MATCHES="1"),
}
_GROUP = re.compile(r"\[mgx\] score group: (\d+) queries; fast path (\d+) items \((\d+) queries, .*?list merge \d+ items; "
                    r"fast schedule: (\d+) seed items, at most (\d+) items per query, longest item (\d+) tiles")
_INDEX = re.compile(r"\[mgx\] index: (\d+) tiles, block-max bounds per quarter for (\d+) of (\d+) bitmap rows")
_stopped = []  # why nothing more is started on the device by this module (a child died on a signal or hung)


# ---- the table, the queries and what the oracle answers -------------------------------------------------------------

class Table:
    def __init__(self):
        corpus, where, grams = W.build_corpus()
        self.pair = p = Pair(corpus=corpus, dense_threshold=W.DENSE_THRESHOLD)
        c = p.dev.columns
        assert c.n_docs == W.N_DOCS and (c.n_docs + W.TILE - 1) // W.TILE == W.N_TILES
        row = p.add_filter(W.filter_docs())
        self.batches = W.make_queries(grams, c, row)
        planted = np.zeros(W.N_DOCS + 1, bool)  # by docid
        for slots in where.values():
            planted[np.asarray(slots) + 1] = True
        saturated = np.zeros(W.N_DOCS + 1, bool)  # a tf past the nibble, or a length past the byte column
        saturated[c.docids[c.tf >= 15]] = True
        saturated[1:] |= c.doc_len >= 255
        self.want, self.ties, self.saturated_pages, self.heavy = [], 0, 0, 0
        self.last_tile_pages = self.seed_tile_pages = 0
        sizes = np.diff(c.offsets.astype(np.int64))
        for qs in self.batches:
            rows = []
            for q in qs:
                # one entry past the page: the boundary falls inside a tie class when it scores like the page's last
                more = Query(q.terms, q.not_terms, filters=q.filters, sort_score=True, limit=q.limit + 1, offset=q.offset,
                             descending=q.descending, k1=q.k1, b=q.b)
                total, page, scores, r = p.oracle_query(more)
                assert not r["empty_term_detected"]
                if len(page) == q.limit + 1:
                    self.ties += scores[-1] == scores[-2]
                page, scores = page[: q.limit], scores[: q.limit]
                rows.append((total, [int(r[k]) for k in W.COUNTERS], page, scores))
                self.saturated_pages += bool((planted & saturated)[page].any())
                tiles = set(((page.astype(np.int64) - 1) // W.TILE).tolist())
                if q.descending and total > 200 and len(page) >= 10:
                    self.last_tile_pages += tiles == {W.N_TILES - 1}
                    self.seed_tile_pages += max(tiles) < W.SEED_TILES
                self.heavy += float(np.prod([sizes[c.lookup(t)] / c.n_docs for t in q.terms])) >= 0.05
            self.want.append(rows)

    def assert_coverage(self):
        """What keeps the comparison from passing vacuously; all of it from the oracle's side alone."""
        n = sum(len(qs) for qs in self.batches)
        assert 56 <= n <= 72, n
        assert self.ties >= 8, self.ties                        # the page boundary inside a tie class
        assert self.saturated_pages >= 8, self.saturated_pages  # a planted saturated document in the page
        assert self.last_tile_pages >= 3, self.last_tile_pages  # pages of 10+ out of hundreds of matches, all in the last tile
        assert self.seed_tile_pages >= 3, self.seed_tile_pages  # ... all inside the seed's tiles
        assert self.heavy >= 8, self.heavy                      # est_density >= 0.05: the second-half re-mask
        qs = [q for b in self.batches for q in b]
        assert {len(q.terms) for q in qs} == {1, 2, 3, 4, 5}
        assert {q.limit for q in qs} == {1, 10, 37, 100} and {q.offset for q in qs} == {0, 5, 7}
        assert sum(not q.descending for q in qs) >= 3 and sum(bool(q.not_terms) for q in qs) >= 4
        assert sum(bool(q.filters) for q in qs) >= 4
        assert {(q.k1, q.b) for q in self.batches[1]} == {W.OTHER_PARAMS}


@pytest.fixture(scope="module")
def table():
    return Table()


def _compare(table, name, arrays):
    """The arrays of run_batches (of this process or out of a child's .npz) against the oracle, every execute."""
    for bi, (qs, rows) in enumerate(zip(table.batches, table.want)):
        for e in range(2):
            key = "b%d_e%d_" % (bi, e)
            counts, lens = arrays[key + "counts"], arrays[key + "len"]
            docs, scores = arrays[key + "docs"], arrays[key + "scores"]
            assert len(counts) == len(lens) == len(qs), (name, key)
            at = np.concatenate([[0], np.cumsum(lens)])
            for i, (q, (total, funnel, page, want_scores)) in enumerate(zip(qs, rows)):
                ctx = (name, "batch %d execute %d query %d" % (bi, e, i), q.terms, q.not_terms, q.filters, q.limit, q.offset,
                       q.descending, q.k1, q.b)
                got_docs, got_scores = docs[at[i]:at[i + 1]], scores[at[i]:at[i + 1]]
                assert int(counts[i][0]) == total, (ctx, int(counts[i][0]), total)
                assert counts[i][1:].tolist() == funnel, (ctx, counts[i][1:].tolist(), funnel)
                assert got_docs.tolist() == page.tolist(), (ctx, got_docs[:8], page[:8])
                assert got_scores.tobytes() == np.asarray(want_scores, np.float64).tobytes(), (ctx, got_scores[:8],
                                                                                               want_scores[:8])


def _schedule(table, name, err):
    """The schedule the verbose lines report: one score-group line per prepared batch, every query on the fast path.
    -> [(seed items, most items of one query, longest item in tiles, queries)] per batch."""
    groups = [tuple(int(x) for x in m.groups()) for m in _GROUP.finditer(err)]
    assert len(groups) == len(table.batches), (name, err[-3000:])
    out = []
    for qs, (n, items, fast_queries, seeds, most, longest) in zip(table.batches, groups):
        assert n == fast_queries == len(qs), (name, n, fast_queries, len(qs))
        assert items >= len(qs)
        out.append((seeds, most, longest, len(qs)))
    return out


# ---- the default schedule, in this process ---------------------------------------------------------------------------

def test_default_schedule(table, monkeypatch, capfd):
    table.assert_coverage()
    for k in KNOBS:
        assert k not in os.environ, k
    monkeypatch.setenv("MGX_VERBOSE", "1")
    capfd.readouterr()
    arrays = W.run_batches(table.pair.dev, table.batches)
    err = capfd.readouterr().err
    monkeypatch.delenv("MGX_VERBOSE")
    for seeds, most, longest, n in _schedule(table, "default", err):
        assert seeds == n and most > 1 and longest <= W.N_TILES, (seeds, most, longest, n)  # a seed per query
    _compare(table, "default", arrays)


# ---- forced schedules, one child process each -------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CONFIGS))
def test_forced_schedule(table, name, tmp_path):
    if _stopped:
        pytest.skip("nothing more is started on the device: " + _stopped[0])
    table.assert_coverage()
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(CONFIGS[name])
    out = str(tmp_path / (name + ".npz"))
    cmd = [sys.executable, os.path.join(ROOT, "tests", "fast_schedule_worker.py"), out]
    t0 = time.time()
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        _stopped.append("the %s child ran into its %d s limit" % (name, CHILD_TIMEOUT))
        tail = (e.stderr or b"")[-3000:]
        pytest.fail("%s: %s" % (_stopped[0], tail.decode(errors="replace") if isinstance(tail, bytes) else tail))
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137):
        _stopped.append("the %s child ended with status %d" % (name, r.returncode))
        pytest.fail(_stopped[0] + "\n" + r.stdout[-1500:] + r.stderr[-3000:])
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    print("%s: child took %.1f s; %s" % (name, time.time() - t0, r.stdout.strip().splitlines()[-1]))
    # the schedule this configuration forces, from the child's verbose lines
    index = [tuple(int(x) for x in m.groups()) for m in _INDEX.finditer(r.stderr)]
    assert len(index) == 1 and index[0][0] == W.N_TILES, r.stderr[-3000:]
    _, fine_rows, bitmap_rows = index[0]
    assert bitmap_rows > 0
    for seeds, most, longest, n in _schedule(table, name, r.stderr):
        if name == "shred":
            assert (seeds, most, longest) == (n, 8, 8) and fine_rows == bitmap_rows, (seeds, most, longest, fine_rows)
        elif name == "long":
            assert (seeds, most, longest) == (n, 2, W.N_TILES - W.SEED_TILES) and fine_rows == 0, (seeds, most, longest,
                                                                                                    fine_rows)
        else:
            assert (seeds, most, longest) == (0, 8, 8) and 0 < fine_rows < bitmap_rows, (seeds, most, longest, fine_rows)
    with np.load(out) as arrays:
        _compare(table, name, arrays)
