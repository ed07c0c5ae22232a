"""Seeded documents for the tests of HIGHLIGHT over original texts: an original, its normalized text and the segments a
synthetic normalizer is given as a per-segment table (tests/highlight_original_ref.py takes exactly these). Shared by
tests/test_highlight_original_cpu.py and tests/test_gpu_highlight_original.py; nothing here is code under test."""

ALPHABETS = ["abcAB ", "abé東京\U00020000 ", "aAｱﾞ京\U0001F600b", "東京都あタ"]
LENGTHS = [1, 2, 7, 100, 10000]
FRAGMENTS = [1, 3, 100]
TAGS = [(b"<em>", b"</em>"), (b"[", b"]"), ("【".encode(), "】".encode()), (b"", b"")]


def make_case(rng, i):
    """(original, normalized, segments, terms, options). Segment shapes: 1 -> 1 (same or another character), 1 -> k
    expansions (k <= 4), m -> 1 contractions (m <= 3), 1 -> 0 deletions; every 9th document is unmappable (its whole-text
    normal form has another number of code points than its segments' pieces), every 11th pure 1 -> 1."""
    alphabet = ALPHABETS[i % len(ALPHABETS)]
    norm_alphabet = ALPHABETS[(i // 3) % len(ALPHABETS)] if i % 2 else alphabet
    dense = i % 5 == 2  # few distinct characters: many matches, merged and clamped windows, more windows than fragments
    if dense:
        alphabet, norm_alphabet = alphabet[:2] + " ", norm_alphabet[:2]
    identity_only = i % 11 == 0
    segments = []
    for _ in range(rng.randint(1, 60 if dense else 40)):
        r = rng.random()
        if identity_only or r < 0.55:
            c = rng.choice(alphabet)
            segments.append((c, c if rng.random() < 0.6 else rng.choice(norm_alphabet)))
        elif r < 0.75:
            segments.append((rng.choice(alphabet), "".join(rng.choice(norm_alphabet) for _ in range(rng.randint(2, 4)))))
        elif r < 0.93:
            segments.append(("".join(rng.choice(alphabet) for _ in range(rng.randint(2, 3))), rng.choice(norm_alphabet)))
        else:
            segments.append((rng.choice(alphabet), ""))
    original = "".join(s for s, _ in segments)
    normalized = "".join(n for _, n in segments)
    terms = []
    for _ in range(rng.choice([0, 1, 1, 2, 2, 3, 5])):
        if normalized and rng.random() < 0.9:
            a = rng.randrange(len(normalized))
            terms.append(normalized[a:a + rng.randint(1, 5)])
        else:
            terms.append("".join(rng.choice(norm_alphabet) for _ in range(rng.randint(0, 3))))
    if i % 7 == 3 and terms:  # a term and a longer one from the same start: shared starts after the translation
        terms.append(terms[0] + normalized[normalized.find(terms[0]) + len(terms[0]):][:2])
    if i % 9 == 4:
        normalized += "z"  # a normalizer that composes across segments: the map no longer fits (:342-344)
    open_tag, close_tag = TAGS[(i // 5) % len(TAGS)]
    opts = dict(snippet_length=LENGTHS[i % len(LENGTHS)], max_fragments=FRAGMENTS[(i // len(LENGTHS)) % len(FRAGMENTS)],
                open_tag=open_tag, close_tag=close_tag)
    return (original.encode(), normalized.encode(), [(s.encode(), n.encode()) for s, n in segments],
            [t.encode() for t in terms], opts)
