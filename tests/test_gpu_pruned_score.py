"""-m gpu: the survivors of block-max pruning in bitmap_score_kernel (SORT _score DESC over bitmap-form grams), against
the oracle bit for bit: 2..5 scored terms on an index of many tiles (later tiles run against a k-th best score), ties at
the page boundary, a saturated nibble of the rarest term and doc lengths past the byte column inside the page, both
orders (SORT _score ASC does not prune), and a table after deletes."""
import numpy as np
import pytest

from gpu_util import Pair
from pkg import mg

pytestmark = pytest.mark.gpu
Query = mg.engine.Query


def _dense_letter_grams(p, n):
    c = p.dev.columns
    sizes = np.diff(c.offsets.astype(np.int64))
    g = [i for i in range(c.n_grams) if b" " not in c.gram(i)]
    return [c.gram(i).decode() for i in sorted(g, key=lambda i: -sizes[i])[:n]]


@pytest.fixture(scope="module")
def pair400k():
    # 25 tiles: every wave of the workgroup walks several, so later tiles run against a k-th best score
    return Pair(corpus=mg.Corpus.synthetic(400_000, seed=7))


def test_two_to_five_scored_terms(pair400k):
    grams = _dense_letter_grams(pair400k, 48)
    rng = np.random.default_rng(11)
    qs = []
    for k in (2, 3, 4, 5):
        for it in range(8):
            pool = grams[:16] if it % 2 else grams
            terms = [str(t) for t in rng.choice(pool, size=k, replace=False)]
            qs.append(Query(terms, sort_score=True, limit=int(rng.choice([1, 10, 37, 100])),
                            offset=int(rng.choice([0, 0, 5])), descending=it != 7))
    pair400k.check(qs)


def test_ties_at_the_bound_and_saturated_rare_term_in_the_page():
    """Thousands of docs share each score (the page boundary falls inside a tie class), and the rarest term reaches
    tf >= 15 in docs longer than 255 bytes that belong in the page."""
    rng = np.random.default_rng(5)
    words = ["alpha", "beta", "gamma", "delta", "kappa", "sigma"]
    protos = [" ".join(str(w) for w in rng.choice(words, size=int(rng.integers(2, 7)))) for _ in range(30)]
    texts = [protos[int(i)] for i in rng.integers(0, len(protos), size=300_000)]
    for i in rng.choice(len(texts), size=400, replace=False).tolist():  # the term "qz", rare
        reps = int(rng.integers(1, 24))
        pad = " alpha beta" * int(rng.integers(0, 40))                    # up to ~440 bytes
        texts[i] = texts[i] + " " + "qz" * reps + pad
    p = Pair(docs=list(enumerate(texts, start=1)), ngram=2, kanji=0)
    qs = []
    for terms in (["qz", "al"], ["qz", "ta", "be"], ["ma", "ga"], ["ka", "pp", "al"], ["qz", "al", "be", "ma"],
                  ["qz", "si", "gm", "ta", "ph"]):
        for limit, offset in ((10, 0), (10, 3), (37, 0), (100, 7), (1, 0)):
            qs.append(Query(terms, sort_score=True, limit=limit, offset=offset))
        qs.append(Query(terms, sort_score=True, limit=10, descending=False))
    got = p.check(qs)
    assert any(g.total > 1000 for g in got)


def test_table_after_deletes():
    """Documents removed from the main index are cleared from its bitmaps: they are neither counted nor scored, and the
    pages of the table are those of an index built without them."""
    from mygram_db_amd import _shim_capi as S
    n = 120_000
    corpus = mg.Corpus.synthetic(n, seed=43)
    p = Pair(corpus=corpus)
    t = S.Table(p.dev)
    grams = _dense_letter_grams(p, 24)
    qs = [[grams[0], grams[3]], [grams[1], grams[2], grams[5]], [grams[4], grams[7]], [grams[2], grams[9], grams[11]]]
    docs = {i + 1: corpus.text(i) for i in range(n)}
    # remove the current top pages of every query (the docs pruning would otherwise keep) and a random spread
    gone = set()
    for terms in qs:
        _, page, _, _ = p.oracle_query(Query(terms, sort_score=True, limit=20))
        gone.update(int(d) for d in page.tolist())
    rng = np.random.default_rng(3)
    gone.update(int(d) for d in rng.choice(np.arange(1, n + 1), size=2000, replace=False).tolist())
    for d in sorted(gone):
        t.remove_document(d, docs.pop(d))
    want = Pair(docs=sorted(docs.items()), ngram=2, kanji=0)
    for terms in qs:
        for desc in (True, False):
            total, page, scores = t.search(terms, sort_by_score=True, descending=desc, limit=10)
            wt, wp, ws, _ = want.oracle_query(Query(terms, sort_score=True, descending=desc, limit=10))
            assert total == wt and page.tolist() == wp.tolist(), (terms, desc)
            assert np.array_equal(scores, ws), (terms, desc, scores, ws)
