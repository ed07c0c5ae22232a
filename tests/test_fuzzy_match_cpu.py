"""CPU differential test of the FUZZY verify_text matcher (mgx_fuzzy.hpp, the source kOpVerifyFuzzy compiles for the
device) through its host build mgxt_contains_fuzzy_match, against the oracle's ContainsFuzzyMatch
(src/utils/edit_distance.cpp:199-296), whose known answers tests/golden/fuzzy.json pins."""
import random

import pytest

import golden_util as G
from oracle import oracle as O
from pkg import mg

ASCII = "abcdefghij"
KANJI = [chr(c) for c in range(0x6771, 0x6771 + 12)] + ["東", "京", "都", "市", "大", "阪"]
KANA = [chr(c) for c in range(0x3042, 0x3042 + 8)]
WIDE = [chr(0x20000 + i) for i in range(6)] + ["\U0001F600", "\U0001F680"]  # 4-byte UTF-8
SEPS = [" ", "　", " ", "\t", "\r", "\n", "\r\n", " 　 "]


def hook(text, term, d):
    t, q = text.encode("utf-8"), term.encode("utf-8")
    r = mg._capi.load().mgxt_contains_fuzzy_match(t, len(t), q, len(q), d)
    assert r in (0, 1), r
    return bool(r)


def test_golden_contains_fuzzy_match():
    cases = G.load("fuzzy.json")["contains_fuzzy_match"]["cases"]
    assert cases
    for text, term, d, want in cases:
        assert hook(text, term, d) == want == O.contains_fuzzy_match(text, term, d), (text, term, d)


def test_distance_above_two_is_refused():
    assert mg._capi.load().mgxt_contains_fuzzy_match(b"abc", 3, b"abc", 3, 3) == -1


def edit(rng, s, alphabet, n_edits):
    """n_edits random substitutions / insertions / deletions / adjacent transpositions of the code points of s."""
    s = list(s)
    for _ in range(n_edits):
        kind = rng.randrange(4)
        if kind == 0 and s:
            s[rng.randrange(len(s))] = rng.choice(alphabet)
        elif kind == 1:
            s.insert(rng.randrange(len(s) + 1), rng.choice(alphabet))
        elif kind == 2 and len(s) > 1:
            del s[rng.randrange(len(s))]
        elif len(s) > 1:
            i = rng.randrange(len(s) - 1)
            s[i], s[i + 1] = s[i + 1], s[i]
    return "".join(s)


def word(rng, alphabet, lo, hi):
    return "".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi)))


def pick_term(rng, words, alphabet, d, lo=2, hi=8):
    """A term near a piece of some word (within d edits half of the time, further away otherwise) or a fresh one."""
    r = rng.random()
    if r < 0.85:
        w = rng.choice(words)
        a = rng.randrange(len(w))
        piece = w[a:a + rng.randint(lo, hi)] if rng.random() < 0.6 else w
        return edit(rng, piece, alphabet, rng.randint(0, d) if r < 0.5 else rng.randint(d + 1, d + 2)) or piece
    return word(rng, alphabet, lo, hi)


def gen(category, rng):
    d = rng.choice((1, 2))
    sep = " "
    if category == "ascii":
        words = [word(rng, ASCII, 1, 9) for _ in range(rng.randint(1, 8))]
        term = pick_term(rng, words, ASCII, d, 3, 9)
    elif category == "cjk":  # one unspaced run: the window rule
        words = [word(rng, KANJI + KANA, 3, 30)]
        term = pick_term(rng, words, KANJI + KANA, d, 2, 6)
    elif category == "mixed":
        al = ASCII[:5] + "".join(KANJI[:6])
        words = [word(rng, al, 1, 12) for _ in range(rng.randint(1, 5))]
        term = pick_term(rng, words, al, d, 2, 7)
    elif category == "wide":
        al = WIDE + KANJI[:4] + list(ASCII[:3])
        words = [word(rng, al, 1, 14) for _ in range(rng.randint(1, 4))]
        term = pick_term(rng, words, al, d, 2, 6)
    elif category == "separators":
        al = ASCII[:6] + "".join(KANJI[:4])
        words = [word(rng, al, 1, 8) for _ in range(rng.randint(2, 7))]
        term = pick_term(rng, words, al, d, 2, 7)
        text = ""
        for w in words:
            text += w + rng.choice(SEPS)
        return (text[:-1] if rng.random() < 0.5 else rng.choice(SEPS) + text), term, d
    elif category == "short_term":  # |term| <= d code points
        al = ASCII[:4] + "".join(KANJI[:3])
        words = [word(rng, al, 1, 6) for _ in range(rng.randint(1, 4))]
        term = word(rng, al, 1, d)
        if rng.random() < 0.5:  # ASCII words only: the whole-word rule, where a short term can still miss
            words = [word(rng, ASCII, 1, 6) for _ in range(rng.randint(1, 3))]
            term = word(rng, ASCII, 1, d)
    elif category == "long":  # terms and words over 64 code points
        cjk = rng.random() < 0.3
        al = KANJI[:8] if cjk else ASCII[:6]
        words = [word(rng, al, 66, 90) for _ in range(rng.randint(1, 2))]
        base = rng.choice(words)
        a = rng.randrange(max(1, len(base) - 65))
        piece = base[a:a + rng.randint(65, 80)] if cjk else base  # (an ASCII word is compared whole)
        term = edit(rng, piece, al, rng.randint(0, d) if rng.random() < 0.5 else rng.randint(d + 1, d + 3))
    else:
        raise AssertionError(category)
    return sep.join(words), term, d


CATEGORIES = {"ascii": 30000, "cjk": 15000, "mixed": 15000, "wide": 12000, "separators": 15000, "short_term": 12000,
              "long": 3000}


@pytest.mark.parametrize("category", sorted(CATEGORIES))
def test_random_against_oracle(category):
    rng = random.Random(0xF022 + sorted(CATEGORIES).index(category))
    n = CATEGORIES[category]
    hits = 0
    for _ in range(n):
        text, term, d = gen(category, rng)
        want = O.contains_fuzzy_match(text, term, d)
        assert hook(text, term, d) == want, (category, text, term, d, want)
        hits += want
    # both outcomes must occur often, or the category proves little
    assert 0.15 * n < hits < 0.85 * n, (category, hits, n)


def test_random_count_is_at_least_100k():
    assert sum(CATEGORIES.values()) >= 100_000
