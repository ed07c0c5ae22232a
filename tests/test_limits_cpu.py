"""CPU only: the corpora and query generators of the capacity-limit tests (limits_util.py) run through the oracle alone,
with the coverage conditions test_gpu_limits.py relies on asserted from the index columns and the oracle's answers."""
import numpy as np
import pytest

import funnel_util as FU
import limits_util as LU
from gpu_util import OracleSide
from oracle import oracle as O
from pkg import mg


def _side(texts=None, corpus=None):
    corpus = corpus if corpus is not None else mg.Corpus.from_texts(texts)
    return OracleSide(mg.Columns(corpus, 1, 2, 0, True), corpus)


@pytest.fixture(scope="module")
def thr_bitmap():
    texts, held = LU.threshold_corpus_bitmap()
    return _side(texts), held


@pytest.fixture(scope="module")
def thr_lists():
    texts, held = LU.threshold_corpus_lists()
    return _side(texts), held


@pytest.fixture(scope="module")
def long_words():
    return _side(LU.long_word_corpus())


@pytest.fixture(scope="module", params=["bitmap", "lists"])
def big_side(request):
    n, seed = (LU.BITMAP_DOCS, 61) if request.param == "bitmap" else (LU.LISTS_DOCS, 62)
    s = _side(corpus=mg.Corpus.synthetic(n, seed=seed))
    FU.register_cpu(s)
    return s


def _postings(side, gram):
    c = side.columns
    g = c.lookup(gram)
    assert g is not None, gram
    return c.docids[int(c.offsets[g]):int(c.offsets[g + 1])].astype(np.int64) - c.first_doc_id


def test_the_chosen_tokens_form_no_other_bigram(thr_bitmap):
    """The corpus holds the chosen tokens and grams with a space, nothing else; the columns hold what `held` says."""
    side, held = thr_bitmap
    c = side.columns
    assert len(LU.GRAMS) == 127 and len(set(LU.TOKENS)) == 169
    grams = {c.gram(g).decode() for g in range(c.n_grams)}
    assert {g for g in grams if " " not in g} == set(LU.TOKENS)
    for k in (0, 1, 63, 64, 99, 100, 126):
        assert _postings(side, LU.GRAMS[k]).tolist() == np.nonzero(held[:, k])[0].tolist()


def test_thetas_are_what_the_counters_need():
    assert LU.thetas(7) == [1, 2, 3, 4, 5, 6, 7]
    assert LU.thetas(127) == [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 126, 127]
    assert LU.thetas(64) == [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64]
    # a set bit above bit 3 in theta, and counts that carry into every counter bit
    assert any(th >> 6 for th in LU.thetas(127)) and any((th >> 5) & 1 for th in LU.thetas(65))


def test_threshold_corpus_bitmap_coverage(thr_bitmap):
    """(i) the count of the first T grams takes every value 0..T in both full tiles — and in the 77 documents of the last
    tile every value up to 66 plus every count next to a threshold in use (77 documents cannot take 128 values);
    (ii) counts theta - 1, theta, theta + 1 share a 64-document word for every (T, theta); (iii) at least 16 of the 127
    grams have list form (fewer than n_docs / 256 postings), some of them with a per-tile offset row (64 postings or more)
    and some without, and at least 64 have bitmap form."""
    side, held = thr_bitmap
    assert len(held) == LU.BITMAP_DOCS == 2 * 16384 + 77
    assert LU.threshold_coverage(held, 2) == list(LU.THRESHOLD_T)
    sizes = np.asarray([len(_postings(side, g)) for g in LU.GRAMS])
    lists = sizes < side.columns.n_docs / 256.0
    assert lists.sum() >= 16 and (~lists).sum() >= 64, (lists.sum(), sizes)
    assert (sizes[lists] >= 64).sum() >= 4 and (sizes[lists] < 64).sum() >= 4 and sizes.min() > 0, sizes[lists]
    assert held[-1].all() and held[-1 - 3, :124].all()  # the top bit of the partial last word is a match at every theta


def test_threshold_corpus_lists_coverage(thr_lists):
    """(i), (ii) for T <= 64 within the second tile; (iv) every posting of the grams in use lies in ONE tile — the second
    for GRAMS[:64], the first for GRAMS[64:] —, and the mixed queries find exactly theta of their lists in the first tile."""
    side, held = thr_lists
    assert len(held) == LU.LISTS_DOCS == 16384 + 300
    assert LU.threshold_coverage(held, 1, lists=True) == [T for T in LU.THRESHOLD_T if T <= 64]
    for k, g in enumerate(LU.GRAMS):
        p = _postings(side, g)
        assert len(p) > 0 and ((p >= LU.TILE).all() if k < 64 else (p < LU.TILE).all()), g
    second = 0
    for T, th, grams in LU.mixed_threshold_cases():
        assert len(grams) == T == len(set(grams))
        in_first = sum(bool((_postings(side, g) < LU.TILE).any()) for g in grams)
        assert in_first == th
        docs = side.oidx.search_by_threshold(grams, th).astype(np.int64) - 1
        assert (docs < LU.TILE).any(), (T, th)  # the tile that holds exactly theta of the lists has matches
        second += bool((docs >= LU.TILE).any())
    assert second >= 3


@pytest.mark.parametrize("which", ["bitmap", "lists"])
def test_oracle_threshold_equals_the_membership_count(which, request):
    """Index::SearchByThreshold of the oracle against the count written out in numpy, at every (T, theta) the device is
    asked: the reference of test_gpu_limits.py is pinned by a second, independent statement."""
    side, held = request.getfixturevalue("thr_" + which)
    cum = np.cumsum(held, axis=1)
    n = 0
    for T in LU.THRESHOLD_T:
        if which == "lists" and T > LU.LISTS_MAX_T:
            continue
        for th in LU.thetas(T):
            want = (np.nonzero(cum[:, T - 1] >= th)[0] + 1).tolist()
            assert side.oidx.search_by_threshold(LU.GRAMS[:T], th).tolist() == want, (T, th)
            assert 0 < len(want) < len(held)
            n += 1
    assert n >= (150 if which == "bitmap" else 100), n


def test_long_word_terms_match_some_documents_and_not_all(long_words):
    """The master string has 127 distinct grams; every accepted term, at FUZZY 1 and 2, matches at least one document and
    not all of them; theta (from the oracle) spans bit 6 for the long terms; the 129-letter term has 128 known grams."""
    side = long_words
    m = LU.master_string()
    terms, refused = LU.long_word_terms(side)
    assert len(m) == 128 and len(terms) == len(LU.PREFIX_GRAMS) + 1 and terms[len(LU.PREFIX_GRAMS) - 1] == m
    grams = {refused[i:i + 2] for i in range(128)}
    assert len(refused) == 129 and len(grams) == 128 and all(side.columns.lookup(g) is not None for g in grams)
    seen = set()
    for t in terms:
        for d in (1, 2):
            r = O.execute_fuzzy(side.oidx, side.ostore, [t], d, ngram_size=2, kanji_ngram_size=0, cross_boundary=True)
            assert 0 < len(r["results"]) < side.columns.n_docs, (t, d)
            seen.add(r["thetas"][0])
    assert {6, 4, 125, 123, 63, 61, 31, 29} <= seen, sorted(seen)
    typo = terms[-1]
    known = [g for g in {typo[i:i + 2] for i in range(127)} if side.columns.lookup(g) is not None]
    assert len(known) == 125  # fewer than the 127 theta starts from


def test_long_word_specs_meet_the_oracle(long_words):
    specs = LU.long_word_specs(long_words)
    want = FU.expected(long_words, specs, 0, 0)
    assert len(specs) == 108 and not any(w[3]["empty_term_detected"] for w in want)
    assert sum(w[0] > 0 for w in want) >= 0.8 * len(want)
    assert sum(bool(s.page.get("sort_score")) and w[0] > 0 for s, w in zip(specs, want)) >= 20


@pytest.mark.parametrize("shape", LU.SHAPES)
def test_chains_have_the_depth_they_claim_and_their_innermost_term_decides(big_side, shape):
    for d in LU.DEPTHS + (41,):
        tree = LU.chain(big_side, shape, d)
        assert LU.stack_depth(tree) == d and LU.n_tokens(tree) <= 512
        if d <= 40:
            LU.check_tree_coverage(big_side, tree)


def test_wide_trees_have_512_tokens_and_a_result(big_side):
    for tree in LU.wide_trees(big_side) + LU.wide_trees(big_side, distinct=24)[:1]:
        assert LU.n_tokens(tree) == 512 and LU.stack_depth(tree) == 1 and len(set(tree[1:])) <= 64
        LU.check_tree_coverage(big_side, tree, chain_shape=False)


def test_halves_chain_has_matches_in_both_tiles(thr_lists):
    """In the first tile the chain's result is its first operand's postings and nothing else; the second tile has matches of
    the deep AND."""
    side, held = thr_lists
    for d in (31, 32, 33, 39, 40):
        tree = LU.halves_chain(d)
        assert LU.stack_depth(tree) == d
        docs = side.oracle_query(LU.Query(expr=tree, limit=0, descending=False))[1].astype(np.int64) - 1
        assert docs[docs < LU.TILE].tolist() == np.nonzero(held[:LU.TILE, 64])[0].tolist() and (docs < LU.TILE).sum() > 50
        assert (docs >= LU.TILE).sum() > 10
