"""CPU differential test of the highlighter (mgx_highlight.hpp, the window / merge / clamp / render source highlight_kernel
compiles for the device) through its host build mgxt_highlight_generate / mgxt_highlight_match_positions.

tests/highlight_ref.py is the checker: a line-cited restatement of the reference's Highlighter. It is pinned first on
tests/golden/highlight.json (the reference's own unit-test vectors), then the library is compared with the golden rows
and with the restatement on seeded random cases; every generated case is compared."""
import ctypes as C
import random

import golden_util as G
import highlight_ref as R
from pkg import mg

CASES = G.load("highlight.json")["cases"]


def _terms(terms):
    arr = (C.c_char_p * max(len(terms), 1))(*terms)
    lens = (C.c_size_t * max(len(terms), 1))(*[len(t) for t in terms])
    return arr, lens


def lib_generate(text, terms, snippet_length=100, max_fragments=3, open_tag=b"<em>", close_tag=b"</em>"):
    L = mg._capi.load()
    arr, lens = _terms(terms)
    n = C.c_size_t(0)
    cap = 256
    for _ in range(2):
        buf = C.create_string_buffer(cap)
        rc = L.mgxt_highlight_generate(text, len(text), arr, lens, len(terms), snippet_length, max_fragments, open_tag,
                                       len(open_tag), close_tag, len(close_tag), buf, cap, C.byref(n))
        assert rc == 0, rc
        if n.value <= cap:
            return buf.raw[:n.value]
        cap = n.value
    raise AssertionError("length changed between calls")


def lib_positions(text, terms):
    L = mg._capi.load()
    arr, lens = _terms(terms)
    n = C.c_size_t(0)
    cap = len(text) + 1
    buf = (C.c_uint32 * (2 * cap))()
    rc = L.mgxt_highlight_match_positions(text, len(text), arr, lens, len(terms), buf, cap, C.byref(n))
    assert rc == 0, rc
    assert n.value <= cap
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n.value)]


def _options(case):
    o = case.get("options", {})
    return dict(snippet_length=o.get("snippet_length", 100), max_fragments=o.get("max_fragments", 3),
                open_tag=o.get("open_tag", "<em>").encode(), close_tag=o.get("close_tag", "</em>").encode())


def _strip(snippet, o):
    for tag in (o["open_tag"], o["close_tag"], b"..."):
        snippet = snippet.replace(tag, b"")
    return snippet


def _check_properties(case, generate, positions):
    text = case["text"].encode()
    terms = [t.encode() for t in case["terms"]]
    o = _options(case)
    snippet = generate(text, terms, **o)
    pos = positions(text, terms)
    for prop in case["properties"]:
        (name, arg), = prop.items()
        if name == "contains":
            assert arg.encode() in snippet, (case["name"], snippet)
        elif name == "not_contains":
            assert arg.encode() not in snippet, (case["name"], snippet)
        elif name == "starts_with":
            assert snippet.startswith(arg.encode()), (case["name"], snippet)
        elif name == "ends_with":
            assert snippet.endswith(arg.encode()), (case["name"], snippet)
        elif name == "count_at_least":
            assert snippet.count(arg[0].encode()) >= arg[1], (case["name"], snippet)
        elif name == "stripped_code_points_at_most":
            assert R.count_code_points(_strip(snippet, o)) <= arg, (case["name"], snippet)
        elif name == "positions_count":
            assert len(pos) == arg, (case["name"], pos)
        elif name == "position":
            assert tuple(pos[arg[0]]) == tuple(arg[1]), (case["name"], pos)
        else:
            raise AssertionError("unknown property " + name)


def _check_golden(generate, positions):
    kinds = set()
    for case in CASES:
        assert case["source"].startswith("tests/query/highlighter_test.cpp:")
        text = case["text"].encode()
        terms = [t.encode() for t in case["terms"]]
        kinds.add(case["kind"])
        if case["kind"] == "positions":
            assert [tuple(p) for p in positions(text, terms)] == [tuple(p) for p in case["expected"]], case["name"]
        elif case["kind"] == "generate":
            assert generate(text, terms, **_options(case)) == case["expected"].encode(), case["name"]
        else:
            _check_properties(case, generate, positions)
    assert kinds == {"positions", "generate", "property"}


def test_restatement_matches_the_reference_vectors():
    _check_golden(R.generate, R.find_match_positions)


def test_library_matches_the_reference_vectors():
    _check_golden(lib_generate, lib_positions)


def test_shim_highlighter_matches_the_reference_vectors():
    """query::Highlighter::Generate of the C++ shim (through its C face) on the golden's exact cases."""
    from mygram_db_amd import _shim_capi as S
    L = S.load()
    n_exact = 0
    for case in CASES:
        if case["kind"] != "generate":
            continue
        o = _options(case)
        text = case["text"].encode()
        terms = [t.encode() for t in case["terms"]]
        arr, lens = _terms(terms)
        buf = C.create_string_buffer(1024)
        n = C.c_size_t(0)
        rc = L.mgxs_highlight_generate(text, len(text), len(terms), C.cast(arr, C.c_void_p), C.cast(lens, C.c_void_p),
                                       o["open_tag"], o["close_tag"], o["snippet_length"], o["max_fragments"],
                                       C.cast(buf, C.c_void_p), 1024, C.byref(n))
        assert rc == 0
        assert buf.raw[:n.value] == case["expected"].encode(), case["name"]
        n_exact += 1
    assert n_exact == 7


def test_option_ranges_are_the_parsers():
    L = mg._capi.load()
    n = C.c_size_t(0)
    arr, lens = _terms([b"a"])
    buf = C.create_string_buffer(64)

    def rc(length, fragments, open_tag=b"<em>", close_tag=b"</em>"):
        return L.mgxt_highlight_generate(b"abc", 3, arr, lens, 1, length, fragments, open_tag, len(open_tag), close_tag,
                                         len(close_tag), buf, 64, C.byref(n))
    assert rc(1, 1) == 0 and rc(10000, 100) == 0 and rc(5, 5, b"x" * 256, b"y" * 256) == 0
    for bad in ((0, 1), (10001, 1), (1, 0), (1, 101)):
        assert rc(*bad) == 3, bad
    assert rc(5, 5, b"x" * 257) == 3 and rc(5, 5, b"<", b"y" * 257) == 3


def test_build_highlight_terms():
    # search_pipeline.cpp:712-745 without the synonym branch
    assert R.build_highlight_terms([b"hello world", b"", b"hello", b"a\tb  c"]) == \
        [b"a", b"a\tb  c", b"b", b"c", b"hello", b"hello world", b"world"]
    assert R.build_highlight_terms([b"X", b"x"], normalize=bytes.lower) == [b"x"]
    assert R.build_highlight_terms([]) == []


# ---- seeded random cases ---------------------------------------------------------------------------------------------

ASCII = "abcab "
KANJI = "東京都大阪市"
KANA = "あいうタワー"
WIDE = "\U00020000\U00020001\U0001F600"  # 4-byte UTF-8
TAGS = [(b"<em>", b"</em>"), (b"[", b"]"), ("«".encode(), "»".encode()), ("【".encode(), "】".encode()), (b"", b"")]


def _text(rng, alphabet, lo, hi):
    return "".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi)))


def _case(rng, i):
    """One (text, terms, options). The shapes cycle so that a run of any length reaches all of them."""
    shape = i % 12
    alphabet = [ASCII, KANJI + KANA, ASCII + KANJI + KANA, ASCII + WIDE + KANJI][(i // 12) % 4]
    L = rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 10, 16, 21, 100])
    F = rng.choice([1, 1, 2, 3, 5, 100])
    text = "" if shape == 11 and i % 24 == 11 else _text(rng, alphabet, 1, 120)  # (empty text: every 24th case)
    terms = []

    def piece(lo=1, hi=4):
        if not text:
            return _text(rng, alphabet, lo, hi)
        a = rng.randrange(len(text))
        return text[a:a + rng.randint(lo, hi)]
    if shape == 0:    # terms that share a start, one a prefix of another
        p = piece(2, 5)
        terms = [p, p[:1], p[:max(1, len(p) - 1)], p + rng.choice(alphabet)]
    elif shape == 1:  # terms that overlap each other
        a = rng.randrange(max(1, len(text)))
        terms = [text[a:a + 3], text[a + 1:a + 4], text[a + 2:a + 6]]
    elif shape in (2, 3, 4):  # dense matches that merge into one over-long window: left edge, middle, right edge
        unit = piece(1, 2) or "a"
        dense = (unit + rng.choice(["", " ", rng.choice(alphabet)])) * rng.randint(8, 40)
        pad = _text(rng, alphabet.replace(unit[0], "") or "z", 30, 60)
        text = [dense + pad, pad + dense + pad, pad + dense][shape - 2]
        terms = [unit]
        L = rng.choice([1, 3, 4, 7, 10])
    elif shape == 5:  # more windows than max_fragments
        unit = piece(1, 3) or "a"
        gap = alphabet.replace(unit[0], "") or "z"
        text = "".join(unit + _text(rng, gap, 6, 14) for _ in range(rng.randint(3, 9)))
        terms = [unit]
        L = rng.choice([1, 2, 3, 4, 5])
        F = rng.choice([1, 2, 3])
    elif shape == 6:  # snippet_length larger than the text
        terms = [piece(), piece()]
        L = rng.choice([200, 1000, 10000])
    elif shape == 7:  # empty terms, a term longer than the text, no term at all
        terms = rng.choice([[], [""], ["", piece()], [text + "x"], [text + "x", piece()]])
    elif shape == 8:  # no match
        terms = ["éé", "zzzzq"]
    else:             # plain mixtures
        terms = [piece(1, 6) for _ in range(rng.randint(1, 5))]
    open_tag, close_tag = TAGS[(i // 7) % len(TAGS)]
    return text.encode(), [t.encode() for t in terms], dict(snippet_length=L, max_fragments=F, open_tag=open_tag,
                                                          close_tag=close_tag)


N_RANDOM = 24000


def test_library_matches_the_restatement_on_random_cases():
    rng = random.Random(20240607)
    seen = {"clamped": 0, "truncated": 0, "multibyte4": 0, "cjk": 0, "no_match": 0, "empty_text": 0, "L1": 0, "F1": 0,
            "odd": 0, "tags_multibyte": 0, "leading": 0, "trailing": 0}
    for i in range(N_RANDOM):
        text, terms, o = _case(rng, i)
        want = R.generate(text, terms, **o)
        got = lib_generate(text, terms, **o)
        assert got == want, (i, text, terms, o, got, want)
        want_pos = R.find_match_positions(text, terms)
        assert lib_positions(text, terms) == want_pos, (i, text, terms)
        # what the generator reached (asserted below)
        total = R.count_code_points(text)
        r = o["snippet_length"] // 2
        merged = R.merge_windows([(s - r if s > r else 0, min(total, e + r)) for s, e in want_pos])
        seen["clamped"] += any(b - a > o["snippet_length"] for a, b in merged)
        seen["truncated"] += len(merged) > o["max_fragments"]
        seen["multibyte4"] += any(c >= 0xF0 for c in text)
        seen["cjk"] += any(0xE0 <= c < 0xF0 for c in text)
        seen["no_match"] += bool(text) and not want_pos
        seen["empty_text"] += not text
        seen["L1"] += o["snippet_length"] == 1
        seen["F1"] += o["max_fragments"] == 1
        seen["odd"] += o["snippet_length"] % 2 == 1
        seen["tags_multibyte"] += len(o["open_tag"]) > 1 and o["open_tag"][0] >= 0x80
        seen["leading"] += bool(want_pos) and want.startswith(b"...")
        seen["trailing"] += bool(want_pos) and want.endswith(b"...")
    for what, n in seen.items():
        assert n >= 50, (what, n)


def test_clamp_reaches_both_edges_and_the_middle():
    """The ClampWindows path with the dense run at the left edge, in the middle and at the right edge of the text."""
    for text in (b"ab" * 40 + b"z" * 60, b"z" * 60 + b"ab" * 40 + b"z" * 60, b"z" * 60 + b"ab" * 40):
        for L in (1, 5, 10, 11):
            for F in (1, 3):
                o = dict(snippet_length=L, max_fragments=F, open_tag=b"<", close_tag=b">")
                want = R.generate(text, [b"ab", b"a"], **o)
                assert lib_generate(text, [b"ab", b"a"], **o) == want
                assert R.count_code_points(_strip(want, o)) <= L
