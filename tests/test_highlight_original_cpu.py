"""CPU differential test of HIGHLIGHT over original texts: the translation of matches, the pending-range filter and the
code point -> byte walk of mgx_highlight.hpp (the source highlight_original_kernel compiles for the device) through the
host build mgxt_highlight_generate_original / mgxt_highlight_filter_ranges.

tests/highlight_original_ref.py is the checker: a line-cited restatement of Highlighter::GenerateOriginal. It is pinned
first on tests/golden/highlight_original.json (the reference's own unit-test vectors), then the library is compared with
the golden rows and with the restatement on seeded random cases whose normalizers are synthetic per-segment tables; every
generated case is compared. The same cases drive tests/cpp/highlight_original_host_check.cpp, a stand-alone program over
the header (`make highlight-original-host-asan` builds it with -fsanitize=address,undefined)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np

import golden_util as G
from highlight_original_cases import FRAGMENTS, LENGTHS, make_case
import highlight_original_ref as O
import highlight_ref as R
from pkg import mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = G.load("highlight_original.json")["cases"]


def _terms(terms):
    arr = (C.c_char_p * max(len(terms), 1))(*terms)
    lens = (C.c_size_t * max(len(terms), 1))(*[len(t) for t in terms])
    return arr, lens


def lib_generate_original(original, normalized, kind, pairs, terms, snippet_length=100, max_fragments=3,
                          open_tag=b"<em>", close_tag=b"</em>"):
    L = mg._capi.load()
    arr, lens = _terms(terms)
    flat = np.ascontiguousarray(np.asarray(pairs if pairs else [], dtype=np.uint32).reshape(-1, 2))
    n = C.c_size_t(0)
    cap = 256
    for _ in range(2):
        buf = C.create_string_buffer(cap)
        rc = L.mgxt_highlight_generate_original(original, len(original), normalized, len(normalized), kind,
                                                flat.ctypes.data if len(flat) else None, len(flat), arr, lens, len(terms),
                                                snippet_length, max_fragments, open_tag, len(open_tag), close_tag,
                                                len(close_tag), C.cast(buf, C.c_void_p), cap, C.byref(n))
        assert rc == 0, rc
        if n.value <= cap:
            return buf.raw[:n.value]
        cap = n.value
    raise AssertionError("length changed between calls")


def lib_filter(ranges):
    L = mg._capi.load()
    a = np.ascontiguousarray(np.asarray(ranges if ranges else [], dtype=np.uint32).reshape(-1, 2))
    out = np.zeros((max(len(a), 1), 2), dtype=np.uint32)
    n = C.c_size_t(0)
    assert L.mgxt_highlight_filter_ranges(a.ctypes.data if len(a) else None, len(a), out.ctypes.data, C.byref(n)) == 0
    return [tuple(int(x) for x in p) for p in out[:n.value]]


def _golden(case):
    o = case["options"]
    opts = dict(snippet_length=o.get("snippet_length", 100), max_fragments=o.get("max_fragments", 3),
                open_tag=o.get("open_tag", "<em>").encode(), close_tag=o.get("close_tag", "</em>").encode())
    segments = [(s["text"].encode(), s["normalized"].encode()) for s in case["segments"]]
    for s, (_, norm) in zip(case["segments"], segments):
        assert s["normalized_code_points"] == R.count_code_points(norm)
    return (case["original"].encode(), case["normalized"].encode(), segments, [t.encode() for t in case["terms"]], opts)


def test_restatement_matches_the_reference_vectors():
    assert [c["name"] for c in CASES] == ["empty_terms", "case_and_width", "nfd_composition", "halfwidth_kana_dakuten",
                                          "expanding_normalizer"]
    for case in CASES:
        assert case["source"].startswith("tests/query/highlighter_test.cpp:")
        original, normalized, segments, terms, opts = _golden(case)
        assert b"".join(s for s, _ in segments) == original
        assert O.generate_original(original, normalized, segments, terms, **opts) == case["expected"].encode(), case["name"]


def test_library_matches_the_reference_vectors():
    kinds = {}
    for case in CASES:
        original, normalized, segments, terms, opts = _golden(case)
        kind, pairs = O.build_map(original, normalized, segments)
        kinds[case["name"]] = kind
        got = lib_generate_original(original, normalized, kind, pairs, terms, **opts)
        assert got == case["expected"].encode(), (case["name"], got)
    assert kinds == {"empty_terms": O.ORIG_IDENTITY, "case_and_width": O.ORIG_IDENTITY, "nfd_composition": O.ORIG_MAPPED,
                     "halfwidth_kana_dakuten": O.ORIG_MAPPED, "expanding_normalizer": O.ORIG_MAPPED}


def test_kind_none_is_generate_over_the_normalized_text():
    assert lib_generate_original(b"Tokyo Tower", b"tokyo tower", O.ORIG_NONE, None, [b"tower"]) == \
        R.generate(b"tokyo tower", [b"tower"]) == b"tokyo <em>tower</em>"


# ---- the pending-range filter against the sort-based original --------------------------------------------------------

def test_filter_replaces_a_shared_start_by_the_longer_range():
    """Built by hand: the later range shares the held one's start and is longer, so it replaces it; what starts inside
    the longer one is dropped although it starts behind the shorter one's end."""
    ranges = [(0, 2), (0, 5), (3, 6), (5, 7), (5, 9), (9, 10)]
    want = O.remove_overlapping_match_positions(ranges)
    assert want == [(0, 5), (5, 9), (9, 10)]
    assert lib_filter(ranges) == want
    assert lib_filter([]) == [] and lib_filter([(4, 6)]) == [(4, 6)]
    assert lib_filter([(1, 3), (1, 3), (2, 4), (3, 4)]) == O.remove_overlapping_match_positions([(1, 3), (1, 3), (2, 4), (3, 4)])


def test_filter_equals_the_sort_on_random_monotone_ranges():
    rng = random.Random(5)
    replaced = 0
    for _ in range(4000):
        n = rng.randint(0, 12)
        s = e = 0
        ranges = []
        for _ in range(n):
            s += rng.choice([0, 0, 1, 2, 5])
            e = max(e, s + 1) + rng.choice([0, 0, 1, 3])
            ranges.append((s, e))
        want = O.remove_overlapping_match_positions(ranges)
        assert lib_filter(ranges) == want, ranges
        replaced += any(a[0] == b[0] and b[1] > a[1] for a, b in zip(ranges, ranges[1:]))
    assert replaced >= 500


# ---- seeded random cases: synthetic normalizers as per-segment tables ------------------------------------------------

N_RANDOM = 12000


def test_library_matches_the_restatement_on_random_cases():
    rng = random.Random(20250311)
    seen = {"identity": 0, "mapped": 0, "unmappable": 0, "expansion_match": 0, "contraction_match": 0, "shared_start": 0,
            "dropped_by_filter": 0, "truncated": 0, "clamped": 0, "no_terms": 0, "multibyte4": 0}
    for L in LENGTHS:
        seen["L%d" % L] = 0
    for F in FRAGMENTS:
        seen["F%d" % F] = 0
    for i in range(N_RANDOM):
        original, normalized, segments, terms, o = make_case(rng, i)
        kind, pairs = O.build_map(original, normalized, segments)
        want = O.generate_original(original, normalized, segments, terms, **o)
        got = lib_generate_original(original, normalized, kind, pairs, terms, **o)
        assert got == want, (i, original, normalized, kind, pairs, terms, o, got, want)
        seen[{O.ORIG_IDENTITY: "identity", O.ORIG_MAPPED: "mapped", O.ORIG_UNMAPPABLE: "unmappable"}[kind]] += 1
        seen["L%d" % o["snippet_length"]] += 1
        seen["F%d" % o["max_fragments"]] += 1
        seen["no_terms"] += not terms
        seen["multibyte4"] += any(c >= 0xF0 for c in original)
        if kind == O.ORIG_UNMAPPABLE or not terms:
            continue
        # the streaming filter on this case's translated ranges, against the sort-based original
        ranges = O.translated_matches(normalized, segments, terms)
        kept = O.remove_overlapping_match_positions(ranges)
        assert lib_filter(ranges) == kept, (i, ranges)
        m = O.segment_map(segments)
        matches = R.find_match_positions(normalized, terms)
        total = R.count_code_points(original)
        r = o["snippet_length"] // 2
        merged = R.merge_windows([(s - r if s > r else 0, min(total, e + r)) for s, e in kept])
        seen["expansion_match"] += any(s > 0 and m[s] == m[s - 1] and e < len(m) and m[e - 1] == m[e] for s, e in matches)
        seen["contraction_match"] += any(m[s][1] - m[s][0] > 1 for s, e in matches)
        seen["shared_start"] += any(a[0] == b[0] and b[1] > a[1] for a, b in zip(ranges, ranges[1:]))
        seen["dropped_by_filter"] += len(kept) < len(ranges)
        seen["truncated"] += len(merged) > o["max_fragments"]
        seen["clamped"] += any(b - a > o["snippet_length"] for a, b in merged)
    for what, n in seen.items():
        assert n >= 50, (what, n)


# ---- the stand-alone host program ------------------------------------------------------------------------------------

def _hex(b):
    return b.hex() if b else "-"


def host_check_lines(n_random=1500):
    """The golden rows and seeded random cases in the line format tests/cpp/highlight_original_host_check.cpp reads."""
    rows = []
    for case in CASES:
        rows.append(_golden(case))
    rng = random.Random(77)
    for i in range(n_random):
        rows.append(make_case(rng, i))
    lines = []
    for original, normalized, segments, terms, o in rows:
        kind, pairs = O.build_map(original, normalized, segments)
        want = O.generate_original(original, normalized, segments, terms, **o)
        flat = [str(x) for p in (pairs or []) for x in p]
        lines.append(" ".join(["gen", _hex(original), _hex(normalized), str(kind), str(len(pairs or []))] + flat +
                              [str(len(terms))] + [_hex(t) for t in terms] +
                              [str(o["snippet_length"]), str(o["max_fragments"]), _hex(o["open_tag"]), _hex(o["close_tag"]),
                               _hex(want)]))
        if kind != O.ORIG_UNMAPPABLE and terms:
            ranges = O.translated_matches(normalized, segments, terms)
            kept = O.remove_overlapping_match_positions(ranges)
            lines.append(" ".join(["flt", str(len(ranges))] + ["%d %d" % p for p in ranges] + [str(len(kept))] +
                                  ["%d %d" % p for p in kept]))
    return lines


def test_host_program(tmp_path):
    """mgx_highlight.hpp as a C++ host sees it, against the restatement: a stand-alone program, no GPU, no ctypes."""
    lines = host_check_lines()
    case_file = tmp_path / "highlight_original_lines.txt"
    case_file.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "highlight_original_host_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "highlight_original_host_check.cpp")], check=True)
    r = subprocess.run([str(exe), str(case_file)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d lines, 0 bad" % len(lines) in r.stdout, r.stdout


if __name__ == "__main__":  # the vectors on stdout, for the sanitizer build
    print("\n".join(host_check_lines()))
