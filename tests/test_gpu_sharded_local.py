"""Sharded tables of 1 to 8 shards in one process (tests/shard_util.py): every shard's export, the gathered blobs and
the merge on EVERY rank against the oracle over the whole table. Totals, page doc ids and fp64 scores are compared
exactly; every query of every case is asserted."""
import numpy as np
import pytest

from dist_worker import N_DOCS, table_texts
from gpu_util import OracleSide
from oracle import oracle as O
from pkg import mg

pytestmark = pytest.mark.gpu

Query = mg.engine.Query
LIMITS = (1, 10, 37, 100, 1000)
OFFSETS = (0, 5, 24)
BIG_WORLDS = (1, 2, 3, 5, 8)   # 40 000 docs: world 2 = two tiles per shard, world 8 = 5 000 docs, one tile
TIE_WORLDS = (1, 3, 5, 8)
N_TIE = 24_000


def tie_texts():
    """24 000 docs drawn from 30 prototype texts: every score class has hundreds of members in every shard."""
    rng = np.random.default_rng(5)
    words = ["alpha", "beta", "gamma", "delta", "kappa", "sigma"]
    protos = [" ".join(str(w) for w in rng.choice(words, size=int(rng.integers(2, 7)))) for _ in range(30)]
    return [protos[int(i)].encode() for i in rng.integers(0, len(protos), size=N_TIE)]


class Table:
    """One corpus, its LocalShards per world size (built once) and the oracle's answers per query list (computed once)."""

    def __init__(self, texts):
        self.texts = texts
        self._shards = {}
        self._want = {}
        corpus = mg.Corpus.from_texts(texts)
        self.oracle = OracleSide(mg.Columns(corpus, 1, 2, 0, True), corpus)  # (host only)

    def shards(self, world):
        from shard_util import LocalShards
        if world not in self._shards:
            self._shards[world] = LocalShards(self.texts, world, oracle=self.oracle)
        return self._shards[world]

    def run_and_check(self, world, name, queries, pitch_pad=0):
        """prepare once; execute + exchange + merge twice on the same batch objects (the second time through
        execute_gather, whose gather must never be called on shards this small); all ranks against the oracle."""
        sh = self.shards(world)
        batches = sh.prepare(queries)
        first = sh.run_prepared(batches, pitch_pad)
        if name not in self._want:
            self._want[name] = [sh.oracle.oracle_query(q) for q in queries]
        want = self._want[name]
        sh.check(queries, first, want)
        again = sh.run_prepared(batches, pitch_pad, through_gather=True)
        sh.check(queries, again, want)
        return want


@pytest.fixture(scope="module")
def big():
    return Table(table_texts())


@pytest.fixture(scope="module")
def tie():
    return Table(tie_texts())


def _columns(table):
    return table.oracle.columns


def _letter_grams(cols):
    sizes = np.diff(cols.offsets.astype(np.int64))
    return [(cols.gram(g), int(s)) for g, s in enumerate(sizes.tolist()) if s > 0 and b" " not in cols.gram(g)]


def big_score_queries(table, descending):
    """One batch of mixed pages: limit and offset cycle independently, so top_stride (1024) exceeds most queries' own
    offset + limit and most shards' counts."""
    cols = _columns(table)
    grams = _letter_grams(cols)
    w = np.asarray([s for _, s in grams], dtype=np.float64)
    rng = np.random.default_rng(5)
    term_lists = []
    for i in range(20):  # 2- and 3-term AND of grams, drawn by posting size as dist_worker.queries_for draws them
        pick = rng.choice(len(grams), size=2 + i % 2, replace=False, p=w / w.sum())
        term_lists.append(([grams[j][0].decode() for j in pick], []))
    common = [k.decode() for k, s in grams if s > N_DOCS // 4][:4]
    assert len(common) == 4
    for i in range(4):   # NOT terms
        term_lists.append(([common[i], common[(i + 1) % 4]], [common[(i + 2) % 4]]))
    term_lists.append((["the"], ["an"]))
    # text-level terms (words of 3+ bytes): df is summed over the shards before any rank takes idf
    words = sorted({x for i in range(0, N_DOCS, 997) for x in table.texts[i].decode().split(" ") if len(x) >= 3})
    for i in range(8):
        terms = [str(x) for x in rng.choice(words, size=2, replace=False)]
        if i % 2:
            terms.append(common[0])
        term_lists.append((terms, []))
    term_lists.append(([str(words[3])], []))
    # one-sided terms: most shards match nothing and export count 0
    term_lists += [(["k9"], []), (["7j"], []), (["k9", common[0]], []), (["7j", common[1]], []), (["k9k"], []),
                   (["7j7", "the"], []), (["k9"], ["7j"])]
    # unknown to the whole table: resolved on the host by every rank alike
    term_lists += [(["~#"], []), ([common[0], "~#"], [])]
    qs = []
    for i, (terms, nots) in enumerate(term_lists):
        qs.append(Query(terms, nots, sort_score=True, limit=LIMITS[i % 5], offset=OFFSETS[(i // 5 + i) % 3],
                        descending=descending))
    for lim in LIMITS:     # every limit x offset on one dense and one one-sided query
        for off in OFFSETS:
            qs.append(Query([common[0], common[2]], sort_score=True, limit=lim, offset=off, descending=descending))
            qs.append(Query(["k9"], sort_score=True, limit=lim, offset=off, descending=descending))
    return qs


@pytest.mark.parametrize("descending", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("world", BIG_WORLDS)
def test_sort_score_pages_on_the_synthetic_table(big, world, descending):
    qs = big_score_queries(big, descending)
    assert len({q.limit + q.offset for q in qs}) > 8
    want = big.run_and_check(world, ("score", descending), qs)
    totals = [t for t, _, _, _ in want]
    assert max(totals) > 10_000 and totals.count(0) >= 2 and 4 in totals  # dense, unknown and one-sided queries alike


TIE_TERMS = (["ma", "ga"], ["ka", "pp", "al"], ["al"], ["si", "gm", "ta"], ["be", "ta"], ["alpha", "beta"], ["delta"])


def tie_queries(descending):
    qs = []
    for i, terms in enumerate(TIE_TERMS):
        for k, lim in enumerate(LIMITS):
            qs.append(Query(terms, sort_score=True, limit=lim, offset=OFFSETS[(i + k) % 3], descending=descending))
    qs.append(Query(["al"], ["gamma"], sort_score=True, limit=37, offset=5, descending=descending))
    return qs


def full_ranking(side, q):
    """Every match of a SORT _score query in the reference's order, with its score (the page without its cut)."""
    terms = [O.normalize_text(t) for t in q.terms]
    r = O.execute(side.oidx, side.ostore, terms, [O.normalize_text(t) for t in q.not_terms], [], compute_df=True,
                  ngram_size=side.ngram_size, kanji_ngram_size=side.kanji_ngram_size, cross_boundary=side.cross_boundary)
    res = r["results"]
    sc = O.score_documents(side.ostore, res, [terms[i] for i in r["term_order"]], r["term_df"], side.N, side.avgdl,
                           q.k1, q.b)
    order = O.sort_by_score(res, sc, q.descending, 0, 0)
    lookup = dict(zip(res.tolist(), sc.tolist()))
    return order, np.asarray([lookup[d] for d in order.tolist()])


def test_tie_table_page_boundaries_fall_inside_classes_that_span_shards(tie):
    """Host only (oracle): the premise of the tie-table cases. For every world size at least one page ends inside a
    class of equal scores whose members live in more than one shard, so the docid tie-break across lists decides it."""
    from mygram_db_amd.dist import shard_range
    side = tie.oracle
    for descending in (True, False):
        hits = {w: 0 for w in TIE_WORLDS if w > 1}
        for q in tie_queries(descending):
            order, scores = full_ranking(side, q)
            cut = q.offset + q.limit
            if cut >= len(order) or scores[cut - 1] != scores[cut]:
                continue
            members = order[scores == scores[cut]].astype(np.int64)
            for w in hits:
                per = shard_range(N_TIE, 0, w)[1]
                hits[w] += int(len({int(r) for r in (members - 1) // per}) > 1)
        assert all(n >= 1 for n in hits.values()), hits


@pytest.mark.parametrize("descending", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("world", TIE_WORLDS)
def test_sort_score_pages_on_the_tie_table(tie, world, descending):
    want = tie.run_and_check(world, ("tie", descending), tie_queries(descending))
    assert any(t > 1000 for t, _, _, _ in want)


def _per_shard_counts(side, terms, world=8):
    res = O.execute(side.oidx, side.ostore, terms, [], [], compute_df=False, ngram_size=2, kanji_ngram_size=0,
                    cross_boundary=True)["results"].astype(np.int64)
    return np.bincount((res - 1) // (N_DOCS // world), minlength=world)


@pytest.mark.parametrize("descending", [True, False], ids=["desc", "asc"])
def test_unstaged_merge_of_eight_full_lists_and_of_eight_partial_lists(big, descending):
    """world 8, offset + limit = 1024, so 8 x 1024 slots are merged from global memory. Dense query: every shard's list
    is full (s_full = 8: both pruning bounds apply). Mid query: 300..900 matches per shard, no list is full, nothing is
    pruned and more than 2048 entries survive: the binary-search ranking."""
    side = big.oracle
    cols = side.columns
    grams = _letter_grams(cols)
    dense = [k.decode() for k, s in sorted(grams, key=lambda x: -x[1])[:2]]
    assert (_per_shard_counts(side, dense) >= 1024).all(), _per_shard_counts(side, dense)
    mid = None
    for k, s in sorted(grams, key=lambda x: -x[1]):
        c = _per_shard_counts(side, [k.decode()])
        if c.min() >= 300 and c.max() <= 900:
            mid = [k.decode()]
            break
    assert mid is not None
    c = _per_shard_counts(side, mid)
    assert c.min() >= 300 and c.max() <= 900 and c.sum() > 2048, c
    qs = [Query(dense, sort_score=True, limit=1000, offset=24, descending=descending),
          Query(mid, sort_score=True, limit=1000, offset=24, descending=descending),
          Query(dense, sort_score=True, limit=1024, offset=0, descending=descending),
          Query(mid, sort_score=True, limit=24, offset=1000, descending=descending)]
    want = big.run_and_check(8, ("unstaged", descending), qs)
    assert [len(p) for _, p, _, _ in want] == [1000, 1000, 1024, 24]


def page_queries(table):
    cols = _columns(table)
    grams = sorted(_letter_grams(cols), key=lambda x: -x[1])
    common = [k.decode() for k, _ in grams[:4]]
    assert grams[0][1] > 16_384 * 2  # (a page of 16 384 that is full, cut from more than twice as many matches)
    qs = []
    for descending in (True, False):
        for lim in (1, 100, 5_000, 16_384):
            qs.append(Query([common[0]], limit=lim, descending=descending))
            qs.append(Query([common[1], common[2]], limit=lim, descending=descending))
            qs.append(Query([common[0]], [common[3]], limit=lim, descending=descending))
        qs.append(Query(["k9"], limit=100, descending=descending))               # the first shards only
        qs.append(Query(["7j", common[0]], limit=1, descending=descending))      # the last shards only
        qs.append(Query(["7j"], limit=16_384, descending=descending))
        qs.append(Query(["the"], ["an"], limit=5_000, descending=descending))
        qs.append(Query(["k9"], ["7j"], limit=100, descending=descending))
    return qs


@pytest.mark.parametrize("world", BIG_WORLDS)
def test_docid_ordered_pages(big, world):
    qs = page_queries(big)
    want = big.run_and_check(world, "pages", qs)
    assert max(len(p) for _, p, _, _ in want) == 16_384


@pytest.mark.parametrize("pitch_pad", [0, 64])
@pytest.mark.parametrize("world", [3, 8])
def test_blobs_at_a_pitch_larger_than_the_blob(big, world, pitch_pad):
    """Rank r's blob at r * (bytes + pitch_pad), the padding filled with 0xFF: a read outside a blob is a wrong page."""
    big.run_and_check(world, ("score", True), big_score_queries(big, True), pitch_pad)
    big.run_and_check(world, "pages", page_queries(big), pitch_pad)


def test_run_prepares_executes_both_ways_and_merges(big):
    """LocalShards.run on its own (prepare, execute, exchange, merge; then again through execute_gather), checked by
    LocalShards.check with the oracle's answers computed there."""
    sh = big.shards(3)
    qs = big_score_queries(big, True)[:12] + big_score_queries(big, False)[20:32]
    sh.check(qs, sh.run(qs))
    sh.check(qs, sh.run(qs, pitch_pad=8))
