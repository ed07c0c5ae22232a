"""mgx_batch_merge_shards against numpy (tests/shard_merge_ref.py) on blobs written by hand in the documented exchange
layout (include/mygram_gpu.h, mgx_batch_export_topk). The host batch is a few SORT _score queries on a tiny index: it
only fixes every query's limit, offset and direction; what it computed itself is replaced by the blobs.

Compared per query, all exact: total, number of docs, page doc ids, and the page scores bit for bit."""
import numpy as np
import pytest
import torch

import shard_merge_ref as R
from pkg import mg

pytestmark = pytest.mark.gpu

Query = mg.engine.Query
N_SHARDS = (1, 2, 3, 7, 16, 64)
# (limit, offset, descending) of the usual host batch: top_stride = 124 exceeds every other query's offset + limit
SPECS = ((10, 0, True), (10, 3, False), (37, 5, True), (1, 0, False), (100, 24, True), (7, 0, False), (1, 24, True))


class Host:
    """The tiny index and its prepared, once-executed batches by spec list."""

    def __init__(self):
        torch.cuda.set_device(0)
        self.index = mg.Index(texts=[b"ab cd", b"ab", b"cd ab ab", b"xy", b"ab xy cd", b"cd"], first_doc_id=1)
        self.batches = {}

    def batch(self, specs):
        if specs not in self.batches:
            b = self.index.prepare([Query(["ab"], sort_score=True, limit=lim, offset=off, descending=desc)
                                    for lim, off, desc in specs])
            assert b.n == len(specs)
            b.execute(torch.cuda.current_stream().cuda_stream)
            b.fetch()
            self.batches[specs] = b
        return self.batches[specs]

    def merge(self, specs, shard_lists, pitch_pad=0, separate=False):
        """shard_lists[r][q] = (scores, docs, total) of rank r for query q, best first. -> fetched results."""
        b = self.batch(specs)
        n, stride = len(specs), b.topk_stride()
        assert stride == max(lim + off for lim, off, _ in specs)
        ptr, nbytes, off32 = b.export_buffer()
        assert ptr and (nbytes, off32) == R.blob_bytes(n, stride)
        dirs = [desc for _, _, desc in specs]
        blobs = [R.pack_blob(lists, dirs, stride) for lists in shard_lists]
        stream = torch.cuda.current_stream().cuda_stream
        if separate:  # every rank's blob64 rank after rank, then every blob32: pitch 0 = the blob's own size
            assert pitch_pad == 0
            elems = n * stride + n
            buf = np.concatenate([x[:8 * elems] for x in blobs] + [x[off32:off32 + 4 * elems] for x in blobs])
            dev = torch.from_numpy(buf).to("cuda:0")
            b.merge_shards(len(blobs), dev.data_ptr(), dev.data_ptr() + 8 * elems * len(blobs), stream)
        else:
            buf, pitch = R.gather_blobs(blobs, pitch_pad)
            dev = torch.from_numpy(buf).to("cuda:0")
            b.merge_shards(len(blobs), dev.data_ptr(), dev.data_ptr() + off32, stream, pitch64=pitch // 8,
                           pitch32=pitch // 4)
        got = b.fetch()
        del dev
        return got

    def check(self, specs, shard_lists, **kw):
        got = self.merge(specs, shard_lists, **kw)
        assert len(got) == len(specs)
        for q, ((lim, off, desc), g) in enumerate(zip(specs, got)):
            total, docs, scores = R.merge_page([lists[q] for lists in shard_lists], desc, lim, off)
            ctx = (len(shard_lists), q, lim, off, desc, [len(lists[q][1]) for lists in shard_lists][:16])
            assert g.total == total, (ctx, g.total, total)
            assert len(g.docs) == len(docs), (ctx, len(g.docs), len(docs))
            assert g.docs.tolist() == docs.tolist(), (ctx, g.docs.tolist()[:8], docs.tolist()[:8])
            assert np.array_equal(g.scores.view(np.uint64), scores.view(np.uint64)), (ctx, g.scores[:8], scores[:8])


@pytest.fixture(scope="module")
def host():
    return Host()


TIES = np.array([0.25, 0.5, 0.5000000000000001, 1.75, 3.0])


def tied(rng, m):
    return TIES[rng.integers(0, len(TIES), size=m)]


def make_lists(rng, specs, counts, scores_of=tied, totals=None):
    """shard_lists for a batch: counts[r][q] entries of rank r for query q, scores from scores_of(rng, m) (or
    scores_of(rng, m, r, q)), doc ids unique over the whole batch (some above 2^31), totals[r][q] or the count."""
    n_shards = len(counts)
    n_docs = sum(sum(c) for c in counts)
    pool = (rng.choice((1 << 32) - 2, size=n_docs, replace=False) + 1).astype(np.uint32)
    at = 0
    out = []
    for r in range(n_shards):
        lists = []
        for q, (_, _, desc) in enumerate(specs):
            m = counts[r][q]
            docs = pool[at:at + m]
            at += m
            scores = scores_of(rng, m, r, q) if scores_of.__code__.co_argcount == 4 else scores_of(rng, m)
            s, d = R.sort_list(scores, docs, desc)
            lists.append((s, d, m if totals is None else totals[r][q]))
        out.append(lists)
    return out


def needed_of(specs):
    return [lim + off for lim, off, _ in specs]


@pytest.mark.parametrize("n_shards", N_SHARDS)
def test_counts_at_every_edge(host, n_shards):
    """All lists empty; one non-empty list (first, last); counts 0, 1, needed - 1 and needed mixed over the ranks, with
    tied scores so that the doc id decides across lists; totals larger than the counts."""
    rng = np.random.default_rng(n_shards)
    need = needed_of(SPECS)
    host.check(SPECS, make_lists(rng, SPECS, [[0] * len(SPECS) for _ in range(n_shards)]))
    for only in {0, n_shards - 1}:
        for fill in (lambda x: 1, lambda x: x - 1, lambda x: x):
            counts = [[(fill(x) if r == only else 0) for x in need] for r in range(n_shards)]
            host.check(SPECS, make_lists(rng, SPECS, counts))
    edge = lambda x: (0, 1, max(x - 1, 0), x)  # noqa: E731
    for shift in range(4):
        counts = [[edge(x)[(r + q + shift) % 4] for q, x in enumerate(need)] for r in range(n_shards)]
        totals = [[c + (r * 1000 + q if c == need[q] else 0) for q, c in enumerate(row)] for r, row in enumerate(counts)]
        host.check(SPECS, make_lists(rng, SPECS, counts, totals=totals))
    full = [[x for x in need] for _ in range(n_shards)]
    host.check(SPECS, make_lists(rng, SPECS, full))


@pytest.mark.parametrize("n_shards", N_SHARDS)
def test_every_key_equal_the_doc_id_alone_decides(host, n_shards):
    rng = np.random.default_rng(10 + n_shards)
    need = needed_of(SPECS)
    same = lambda rng, m: np.full(m, 1.5)  # noqa: E731
    host.check(SPECS, make_lists(rng, SPECS, [[x for x in need] for _ in range(n_shards)], same))
    host.check(SPECS, make_lists(rng, SPECS, [[(x - 1 if (r + q) % 2 else x) for q, x in enumerate(need)]
                                              for r in range(n_shards)], same))
    host.check(SPECS, make_lists(rng, SPECS, [[max(x // n_shards, 1) for x in need] for _ in range(n_shards)], same))


@pytest.mark.parametrize("n_shards", [2, 3, 16])
def test_two_shards_hold_equal_keys_with_interleaved_doc_ids(host, n_shards):
    """Ranks 0 and 1 hold the same scores at even and odd doc ids (the other ranks nothing, or worse entries)."""
    need = needed_of(SPECS)
    for others in (0, 3):
        shard_lists = []
        for r in range(n_shards):
            lists = []
            for q, (_, _, desc) in enumerate(SPECS):
                if r < 2:
                    docs = np.arange(need[q], dtype=np.uint32) * 2 + 1000 + r
                    scores = np.repeat(np.arange(need[q] // 4 + 1, dtype=np.float64), 4)[:need[q]] + 2.0
                else:
                    docs = np.arange(min(others, need[q]), dtype=np.uint32) + 10 * r
                    scores = np.full(len(docs), 1.0 if desc else 99.0)
                s, d = R.sort_list(scores, docs, desc)
                lists.append((s, d, len(d)))
            shard_lists.append(lists)
        host.check(SPECS, shard_lists)


@pytest.mark.parametrize("n_shards", N_SHARDS)
def test_keys_ordered_by_rank(host, n_shards):
    """Every list full, rank r's scores all inside (r, r + 1): increasing with the rank and decreasing. The whole page
    comes from one shard while the other full lists push the pruning bound to just under it."""
    rng = np.random.default_rng(20 + n_shards)
    need = needed_of(SPECS)
    counts = [[x for x in need] for _ in range(n_shards)]
    host.check(SPECS, make_lists(rng, SPECS, counts, lambda rng, m, r, q: r + rng.random(m)))
    host.check(SPECS, make_lists(rng, SPECS, counts, lambda rng, m, r, q: (n_shards - r) + rng.random(m)))
    # the same with one score per rank: the bound EQUALS every key of the winning list
    host.check(SPECS, make_lists(rng, SPECS, counts, lambda rng, m, r, q: np.full(m, float(r))))


@pytest.mark.parametrize("n_shards", [2, 3, 7, 16, 64])
def test_exactly_one_full_list(host, n_shards):
    """s_full == 1: only the full list's last key bounds the merge. The other lists (needed - 1 entries) hold entries
    above, at and below that key; a second bound taken from the full list's first entry would drop most of the page."""
    rng = np.random.default_rng(30 + n_shards)
    need = needed_of(SPECS)
    for full_rank in {0, n_shards - 1}:
        counts = [[(x if r == full_rank else x - 1) for x in need] for r in range(n_shards)]
        host.check(SPECS, make_lists(rng, SPECS, counts))
        host.check(SPECS, make_lists(rng, SPECS, counts,
                                     lambda rng, m, r, q: (np.linspace(5.0, 4.0, m) if r == full_rank else tied(rng, m) + 3.0)))


@pytest.mark.parametrize("needed,n_shards,n_full", [(10, 3, 3), (10, 7, 3), (124, 16, 7), (7, 2, 2), (1000, 3, 3),
                                                    (1024, 7, 5), (100, 64, 64), (100, 64, 3)])
def test_full_lists_whose_number_does_not_divide_needed(host, needed, n_shards, n_full):
    """F full lists, needed % F != 0, a = ceil(needed / F): every full list holds a - 1 high entries and then low ones,
    so the merged top needs needed - F * (a - 1) > 0 of the low entries. A bound taken at entry floor(needed / F)
    would sit among the high entries and cut them off."""
    assert needed % n_full and n_full > 1
    a = -(-needed // n_full)
    rng = np.random.default_rng(needed + n_shards)
    specs = ((needed - 5, 5, True), (needed, 0, False), (3, needed - 3, True)) if needed > 8 else \
        ((needed, 0, True), (needed - 1, 1, False))
    full = set(rng.choice(n_shards, size=n_full, replace=False).tolist())

    def scores_of(rng, m, r, q):
        if r not in full:
            return tied(rng, m)  # (between the high and the low entries in both directions: see below)
        desc = specs[q][2]
        high, low = (100.0, 0.001) if desc else (0.001, 100.0)
        return np.concatenate([high + rng.random(a - 1) * (1 if desc else 0.0001), np.full(m - (a - 1), low)])
    counts = [[(needed if r in full else int(rng.integers(0, needed))) for _ in specs] for r in range(n_shards)]
    host.check(specs, make_lists(rng, specs, counts, scores_of))


SPECIAL = np.array([-np.inf, -1.7976931348623157e308, -3.5, -2.2250738585072014e-308, -5e-324, -0.0, 0.0, 5e-324,
                    1e-310, 2.2250738585072014e-308, 3.5, 1.7976931348623157e308, np.inf])


@pytest.mark.parametrize("n_shards", [1, 3, 16])
def test_special_scores_in_both_directions(host, n_shards):
    """-0.0 and +0.0 (two keys: -0.0 ranks below +0.0), negative scores, infinities and denormals travel through the
    key and come back bit for bit, DESC and ASC."""
    rng = np.random.default_rng(40 + n_shards)
    need = needed_of(SPECS)
    special = lambda rng, m: SPECIAL[rng.integers(0, len(SPECIAL), size=m)]  # noqa: E731
    host.check(SPECS, make_lists(rng, SPECS, [[x for x in need] for _ in range(n_shards)], special))
    host.check(SPECS, make_lists(rng, SPECS, [[int(rng.integers(0, x + 1)) for x in need] for _ in range(n_shards)],
                                 special))
    zeros = lambda rng, m: np.array([-0.0, 0.0])[rng.integers(0, 2, size=m)]  # noqa: E731
    host.check(SPECS, make_lists(rng, SPECS, [[x for x in need] for _ in range(n_shards)], zeros))


@pytest.mark.parametrize("n_shards", [1, 2, 7, 64])
def test_totals_above_two_to_the_32(host, n_shards):
    rng = np.random.default_rng(50 + n_shards)
    need = needed_of(SPECS)
    counts = [[x for x in need] for _ in range(n_shards)]
    totals = [[(1 << 32) + (r << 33) + q + (0 if q % 2 else (1 << 40)) for q in range(len(SPECS))] for r in range(n_shards)]
    host.check(SPECS, make_lists(rng, SPECS, counts, totals=totals))


@pytest.mark.parametrize("n_shards,needed", [(3, 341), (16, 64), (1, 1024), (2, 512), (64, 16), (5, 205), (7, 147)])
def test_slots_around_the_staging_limit(host, n_shards, needed):
    """n_shards * needed = 1023, 1024 (staged in LDS) and 1025, 1029 (merged from global memory)."""
    assert n_shards * needed in (1023, 1024, 1025, 1029)
    rng = np.random.default_rng(needed)
    specs = ((needed - 4, 4, True), (needed, 0, False), (1, needed - 1, True))
    full = [[needed] * 3 for _ in range(n_shards)]
    host.check(specs, make_lists(rng, specs, full))
    host.check(specs, make_lists(rng, specs, full, lambda rng, m: rng.random(m)))
    host.check(specs, make_lists(rng, specs, [[int(rng.integers(0, needed + 1)) for _ in specs] for _ in range(n_shards)]))


@pytest.mark.parametrize("counts", [(682, 682, 683), (683, 683, 682), (683, 683, 683), (1023, 1023, 3), (1023, 1023, 1023)])
def test_survivors_around_the_ranking_limit(host, counts):
    """No list is full (needed = 1024), so nothing is pruned and every entry survives: 2047 and 2048 survivors are ranked
    among themselves in LDS, 2049 and more by binary search in the other lists."""
    assert sum(counts) in (2047, 2048, 2049, 3069) and max(counts) < 1024
    rng = np.random.default_rng(sum(counts))
    specs = ((1000, 24, True), (1024, 0, False), (24, 1000, False))
    rows = [[c] * 3 for c in counts]
    host.check(specs, make_lists(rng, specs, rows))
    host.check(specs, make_lists(rng, specs, rows, lambda rng, m: rng.random(m) - 0.5))


def test_many_survivors_under_a_bound(host):
    """64 full lists of 100 equal keys: the bound equals every key, all 6400 entries survive it and are ranked by
    binary search; and 16 full lists of 124 with few distinct scores."""
    rng = np.random.default_rng(7)
    specs = ((90, 10, True), (100, 0, False))
    host.check(specs, make_lists(rng, specs, [[100, 100] for _ in range(64)], lambda rng, m: np.full(m, 2.0)))
    host.check(SPECS, make_lists(rng, SPECS, [needed_of(SPECS) for _ in range(64)], lambda rng, m: np.full(m, -2.0)))


@pytest.mark.parametrize("n_shards", [2, 7])
def test_blob_pitches(host, n_shards):
    """The same lists as one buffer per rank at the blob's own pitch, at a padded pitch (0xFF between the ranks), and
    as separately gathered 64-bit and 32-bit blobs with pitch 0."""
    need = needed_of(SPECS)
    counts = [[(x if (r + q) % 3 else x // 2) for q, x in enumerate(need)] for r in range(n_shards)]
    for kw in ({}, {"pitch_pad": 8}, {"pitch_pad": 64}, {"separate": True}):
        host.check(SPECS, make_lists(np.random.default_rng(n_shards), SPECS, counts), **kw)
