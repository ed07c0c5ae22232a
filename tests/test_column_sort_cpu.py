"""CPU-only: SORT <filter column>. (a) the string-key model (column_sort_ref.py) reproduces the reference's own vectors
(tests/golden/column_sort.json); (b) on random columns of every class the 64-bit key (T, doc) gives the permutation the
string keys give, in both directions; (c) the collision predicate marks exactly the columns where the two differ."""
import json
import os
import random
import subprocess

import pytest

import column_sort_ref as R
from pkg import ROOT

CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "column_sort.json")))["cases"]
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
ALL_ONES = R.U64  # the double whose T is 0


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_string_key_model_reproduces_the_reference_vectors(case):
    assert case["source"].startswith("tests/query/result_sorter_test.cpp:")
    docs = list(range(1, len(case["values"]) + 1))
    values = {d: (None if v is None else tuple(v)) for d, v in zip(docs, case["values"])}
    page, err = R.sort_and_paginate(docs[::-1], values, case["order"] == "ASC", case["limit"], case["offset"],
                                    columns=case["columns"] if case["column"] else None, column=case["column"])
    if "error_code" in case:
        assert page is None
        for piece in case["error_contains"]:
            assert piece in err
        return
    assert err is None
    if "expect" in case:
        assert page == case["expect"]
    else:
        assert len(page) == case["expect_size"]
    if case.get("mixed_types"):
        return  # (one column of two types: the shim refuses to build it; the model alone answers)
    # the same page from the 64-bit key
    if case["column"] == "":
        return  # (primary-key order: doc-id pages on this layer)
    cls, ranks, bias, bits, nulls = R.column_of([values[d] for d in docs])
    keys = {d: R.key_of(cls, b, n, ranks, bias) for d, b, n in zip(docs, bits, nulls)}
    assert not R.has_key_collision(cls, bits, nulls)
    assert R.apply_offset_limit(R.sort_by_key(docs, keys, case["order"] == "DESC"), case["offset"], case["limit"]) == page


def _both_orders(values):
    """(string-key permutation, 64-bit permutation) per direction for documents 5, 6, ... with these values."""
    docs = list(range(5, 5 + len(values)))
    by_doc = dict(zip(docs, values))
    cls, ranks, bias, bits, nulls = R.column_of(values)
    keys = {d: R.key_of(cls, b, n, ranks, bias) for d, b, n in zip(docs, bits, nulls)}
    shuffled = docs[:]
    random.Random(len(values)).shuffle(shuffled)
    out = []
    for ascending in (True, False):
        out.append((R.sort_entries(shuffled, by_doc, ascending), R.sort_by_key(shuffled, keys, not ascending)))
    return out, R.has_key_collision(cls, bits, nulls)


def _column(rng, kind, n, null_rate):
    def one():
        if rng.random() < null_rate:
            return None
        if kind == "int7":  # heavy ties
            return ("int64", rng.randrange(-3, 4))
        if kind == "int64":
            return ("int64", rng.choice([I64MAX, I64MAX - 1, I64MIN + 1, -1, 0, 1, rng.randrange(I64MIN + 1, I64MAX)]))
        if kind == "int8":
            return ("int8", rng.randrange(-128, 128))
        if kind == "bool":
            return ("bool", rng.random() < 0.5)
        if kind == "time":
            return ("time", rng.randrange(-10**10, 10**10))
        if kind == "uint64":
            return ("uint64", rng.choice([0, 1, I64MAX, I64MAX + 1, I64MAX + 2, R.U64, rng.randrange(0, R.U64)]))
        if kind == "double":
            return ("double", rng.choice([0.0, -0.0, float("inf"), float("-inf"), 5e-324, -5e-324, 2.2250738585072014e-308,
                                          1.5, -1.5, rng.uniform(-1e300, 1e300), rng.uniform(-1, 1),
                                          0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000001]))  # ints: NaN bit patterns
        if kind == "string":
            return ("string", rng.choice(["", "a", "A", "ab", "b", "é", "あ", "zz", "a\x01"]))
        if kind == "string_no_empty":
            return ("string", rng.choice(["a", "A", "ab", "b", "é", "あ", "zz"]))
        raise AssertionError(kind)
    return [one() for _ in range(n)]


@pytest.mark.parametrize("kind", ["int7", "int64", "int8", "bool", "time", "uint64", "double", "string", "string_no_empty"])
@pytest.mark.parametrize("null_rate", [0.0, 0.1, 0.6])
def test_the_64_bit_key_orders_like_the_string_key(kind, null_rate):
    rng = random.Random(sum(map(ord, kind)) * 10 + int(null_rate * 10))
    for n in (1, 2, 17, 300):
        perms, marked = _both_orders(_column(rng, kind, n, null_rate))
        assert not marked
        for want, got in perms:
            assert got == want, (kind, null_rate, n)


def test_bool_keys_are_the_reference_strings():
    # "0" < "1" as strings (:193-194) and as signed values; NULL before both
    perms, _ = _both_orders([("bool", True), None, ("bool", False), ("bool", True)])
    assert perms[0][0] == [6, 7, 5, 8] and perms[0][1] == [6, 7, 5, 8]


def test_unsigned_rule_is_the_references_own():
    # 0 and 2^63 share a key (:205-212): the tie goes to the doc id, in both models
    perms, marked = _both_orders([("uint64", 1 << 63), ("uint64", 0), ("uint64", 1), ("uint64", (1 << 63) + 1)])
    assert not marked
    assert perms[0][0] == perms[0][1] == [5, 6, 7, 8]
    assert perms[1][0] == perms[1][1] == [8, 7, 6, 5]


@pytest.mark.parametrize("kind,zero", [("int64", ("int64", I64MIN)), ("double", ("double", ALL_ONES))])
def test_collision_predicate_marks_exactly_the_columns_where_the_models_differ(kind, zero):
    """A non-NULL value with T = 0 ties with NULL in 64 bits but not as strings ("000...0" > ""). The two orders differ
    as soon as a document with that value comes before a NULL document (then the doc-id tie-break puts it on the wrong
    side), which every marked column built here has; columns with one of the two ingredients are exact."""
    rng = random.Random(7)
    seen = set()
    for trial in range(60):
        with_zero, with_null = trial % 2 == 1, (trial // 2) % 2 == 1
        vals = [v for v in _column(rng, kind, 40, 0.0) if v != zero]
        if with_zero:
            vals[3] = zero
            vals[20] = zero
        if with_null:
            vals[10] = None
            vals[30] = None
        perms, marked = _both_orders(vals)
        differ = any(want != got for want, got in perms)
        assert marked == (with_zero and with_null)
        assert differ == marked, (trial, with_zero, with_null)
        seen.add(marked)
    assert seen == {False, True}
    # INT64_MIN without NULLs sorts exactly (result_sorter_test.cpp:1138)
    perms, marked = _both_orders([("int64", I64MAX), ("int64", 0), ("int64", I64MIN), ("int64", -1), ("int64", 1)])
    assert not marked and perms[0][0] == perms[0][1] == [7, 8, 6, 9, 5]


def host_check_lines():
    """Key and collision vectors from the Python model, in the line format tests/cpp/colsort_host_check.cpp reads."""
    rng = random.Random(11)
    edge = [0, 1, R.SIGN - 1, R.SIGN, R.SIGN + 1, R.U64 - 1, R.U64, R.double_bits(-0.0), R.double_bits(float("inf")),
            R.double_bits(float("-inf")), R.double_bits(5e-324), 0x7FF8000000000001]
    lines = []
    for cls in (R.SIGNED, R.UNSIGNED, R.DOUBLE):
        for ranks, bias in ((0, 0), (1, 0), (1, 1)) if cls == R.UNSIGNED else ((0, 0),):
            for bits in edge + [rng.getrandbits(64) for _ in range(40)]:
                if ranks:
                    bits &= 0xFFFFFFFF
                for nul in (0, 1):
                    for desc in (0, 1):
                        doc = rng.choice([0, 1, 5, 0xFFFFFFFF, rng.getrandbits(32)])
                        t = R.key_of(cls, bits, bool(nul), bool(ranks), bias)
                        k, d = R.pair_of(t, doc, bool(desc))
                        lines.append("key %d %d %d %x %d %d %d %x %x %x" % (cls, ranks, bias, bits, nul, desc, doc, t, k, d))
    for cls in (R.SIGNED, R.UNSIGNED, R.DOUBLE):
        zero = R.SIGN if cls == R.SIGNED else R.U64 if cls == R.DOUBLE else 0  # the value whose T is 0 (unsigned: none)
        for with_zero in (0, 1):
            for with_null in (0, 1, 2):  # 2: no NULL array at all
                vals = [(rng.getrandbits(62) + 1, 2 if with_null == 2 else 0) for _ in range(20)]
                if with_zero:
                    vals[7] = (zero, vals[7][1])
                if with_null == 1:
                    vals[3] = (zero, 1)  # (a NULL slot's value does not count, whatever it holds)
                    vals[15] = (5, 1)
                marked = R.has_key_collision(cls, [v for v, _ in vals], [n == 1 for _, n in vals])
                assert marked == (cls != R.UNSIGNED and with_zero == 1 and with_null == 1)
                lines.append("col %d %d %d " % (cls, marked, len(vals)) + " ".join("%x %d" % v for v in vals))
    return lines


def test_host_key_transform_and_collision_scan_program(tmp_path):
    """mgx_colsort.hpp's host pieces as C++ sees them, against the model: a stand-alone program, no GPU, no ctypes.
    (`make colsort-host-asan` builds the same program with -fsanitize=address,undefined.)"""
    lines = host_check_lines()
    case_file = tmp_path / "colsort_lines.txt"
    case_file.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "colsort_host_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "colsort_host_check.cpp")], check=True)
    r = subprocess.run([str(exe), str(case_file)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d lines, 0 bad" % len(lines) in r.stdout, r.stdout


if __name__ == "__main__":  # the vectors on stdout, for the sanitizer build
    print("\n".join(host_check_lines()))
