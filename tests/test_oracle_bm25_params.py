"""Pins the CPU oracle's BM25Scorer::ScoreDocuments (oracle/mygram_oracle.c) away from the default parameters: the whole
k1 x b grid the reference's schema accepts (k1 >= 0, 0 <= b <= 1), average doc lengths below 1 (clamped to 1), far
above and far below the corpus's own, and total_docs below the terms' df and 0. Two references: a pure-Python
restatement of bm25_scorer.cpp:77-86 in the reference's operation order (bit for bit), and an exact rational evaluation
with math.log for the idf (1e-13 relative). The -m gpu parameter tests lean on this oracle. Runs on CPU only."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O

K1 = [0.0, 1e-6, 0.3, 1.2, 2.0, 20.0, 1e4]
B = [0.0, 0.3, 0.75, 1.0]


def _corpus():
    rng = np.random.default_rng(23)
    words = ["ab", "abab", "cd", "xy", "東京", "ab東京", "q"]
    docs = {}
    for d in range(1, 401):
        docs[d] = " ".join(str(w) for w in rng.choice(words, size=int(rng.integers(1, 12))))
    docs[7] = "ab" * 20 + " cd"                      # tf 20: past the 4-bit nibble
    docs[8] = "ab" * 300 + " cd"                     # tf 300, 603 code points
    docs[9] = "東京" * 200 + " ab"                    # 400 CJK code points, 1200+ bytes
    docs[10] = "cd " + "x" * 254                     # dl 257: past the byte column
    docs[11] = "ab"                                  # dl 2
    docs[12] = ""                                    # no text: score 0
    return docs


def _idf(n, df):  # bm25_scorer.cpp:14-25
    if n == 0:
        return 0.0
    df = min(df, n)
    return math.log((float(n) - float(df) + 0.5) / (float(df) + 0.5) + 1.0)


def _restated(docs, cands, terms, dfs, n, avgdl, k1, b):
    """bm25_scorer.cpp:67-90, operation by operation (Python floats are IEEE doubles, evaluated left to right)."""
    idfs = [_idf(n, d) for d in dfs]
    out = []
    for c in cands:
        text = docs.get(c)
        score = 0.0
        if text:
            doc_length = float(len(text))  # code points
            for i, t in enumerate(terms):
                tf = float(text.count(t))  # CountTermOccurrences: non-overlapping
                if tf > 0.0:
                    length_norm = 1.0 - b + b * doc_length / max(avgdl, 1.0)
                    numerator = tf * (k1 + 1.0)
                    denominator = tf + k1 * length_norm
                    score += idfs[i] * numerator / denominator
        out.append(score)
    return np.asarray(out, dtype=np.float64)


def _exact(docs, cands, terms, dfs, n, avgdl, k1, b):
    """The same sum in exact rationals (only the idf's logarithm is a double)."""
    fk1, fb, favg = Fraction(k1), Fraction(b), max(Fraction(avgdl), Fraction(1))
    idfs = [Fraction(_idf(n, d)) for d in dfs]
    out = []
    for c in cands:
        text = docs.get(c)
        s = Fraction(0)
        if text:
            dl = Fraction(len(text))
            for i, t in enumerate(terms):
                tf = Fraction(text.count(t))
                if tf:
                    s += idfs[i] * tf * (fk1 + 1) / (tf + fk1 * (1 - fb + fb * dl / favg))
        out.append(s)
    return out


@pytest.fixture(scope="module")
def store():
    docs = _corpus()
    st = O.DocumentStore()
    for d, t in docs.items():
        st.add(d, t if t else None)
    n, total = st.bm25_stats()
    return docs, st, n, total / n


def _stat_cases(n, avgdl, dfs):
    return [("own", n, avgdl), ("avgdl-below-1", n, 0.37), ("avgdl-x10", n, avgdl * 10.0),
            ("avgdl-div10", n, avgdl / 10.0), ("N-below-df", min(dfs) // 2, avgdl), ("N-zero", 0, avgdl)]


@pytest.mark.parametrize("k1", K1)
@pytest.mark.parametrize("b", B)
def test_score_documents_matches_restatement_and_exact_sum(store, k1, b):
    docs, st, n, avgdl = store
    terms = ["ab", "cd", "東京", "ab東京"]
    dfs = [sum(1 for t in docs.values() if term in t) for term in terms]
    cands = np.asarray(list(range(1, 401)) + [9_000_000], dtype=np.uint32)
    for name, nn, avg in _stat_cases(n, avgdl, dfs):
        got = O.score_documents(st, cands, terms, dfs, nn, avg, k1, b)
        want = _restated(docs, cands.tolist(), terms, dfs, nn, avg, k1, b)
        assert np.array_equal(got, want), (name, k1, b, np.flatnonzero(got != want)[:5])
        exact = _exact(docs, cands.tolist(), terms, dfs, nn, avg, k1, b)
        for c, g, e in zip(cands.tolist(), got.tolist(), exact):
            if e == 0:
                assert g == 0.0, (name, k1, b, c)
            else:
                assert abs(Fraction(g) - e) <= Fraction(1, 10 ** 13) * abs(e), (name, k1, b, c, g, float(e))
        if nn == 0:
            assert not got.any()  # every idf is 0: every score is +0.0
        if k1 == 0.0 and nn:
            # k1 = 0: a term contributes its idf whatever tf and dl are (bm25_scorer_test.cpp:154-173; idf * tf / tf
            # rounds twice)
            one = O.score_documents(st, cands, ["ab"], dfs[:1], nn, avg, k1, b)
            has = np.asarray([bool(docs.get(c)) and "ab" in docs[c] for c in cands.tolist()])
            assert np.allclose(one[has], _idf(nn, dfs[0]), rtol=1e-15, atol=0) and not one[~has].any()
