"""CPU-only: SORT by primary key. mgx_pkey.hpp's host side runs as a stand-alone program (tests/cpp/pksort_host_check.cpp)
and is compared with the string-key model (primary_key_ref.py): (a) the reference's own primary-key vectors of
tests/golden/column_sort.json, (b) key derivation on the edge cases, (c) the comparator key_merge_kernel runs on every
pair of a few hundred keys, under every pairing of the stored forms, against Python's `bytes` comparison, (d) where
column_sort_ref's older model of the same branch agrees with this one, and where it does not."""
import json
import os
import random
import subprocess

import pytest

import column_sort_ref as R
import primary_key_ref as P
from pkg import ROOT

PK_CASES = [c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "column_sort.json")))["cases"] if c["column"] == ""]
U64 = R.U64
EDGE = [b"0", b"7", b"007", b"18446744073709551615", b"18446744073709551616", b"123456789012345678901", b"", b"12a",
        "١٢".encode("utf-8"), b"\x7f", b"\x80", None]


def _hex(k):
    return k.hex() if k else "-"


def _unhex(h):
    return b"" if h == "-" else bytes.fromhex(h)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pksort") / "pksort_host_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "pksort_host_check.cpp")], check=True)

    def run(lines, tmp_path):
        case_file = tmp_path / "pksort_lines.txt"
        case_file.write_text("\n".join(lines) + "\n")
        r = subprocess.run([str(exe), str(case_file)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def sort_block(docs, descending):
    """docs: [(side, doc id, key | None)], doc ids ascending within a side."""
    return ["sort %d %d" % (descending, len(docs))] + ["%d %d %d %s" % (s, d, k is not None, _hex(k)) for s, d, k in docs]


def _run_sort(program, tmp_path, docs, descending):
    out = program(sort_block(docs, descending), tmp_path)
    assert out[0].startswith("order") and out[1].startswith("kinds ")
    return [int(x) for x in out[0].split()[1:]], [int(x) for x in out[1].split()[1:]]


@pytest.mark.parametrize("case", PK_CASES, ids=[c["name"] for c in PK_CASES])
@pytest.mark.parametrize("split", ["one_index", "two_indexes"])
def test_reference_vectors(case, split, program, tmp_path):
    """(a) derivation + comparator reproduce the reference's pages, from one key column and from two merged."""
    assert case["source"].startswith("tests/query/result_sorter_test.cpp:")
    keys = [v[1].encode("utf-8") for v in case["values"]]
    docs = [((i % 2) if split == "two_indexes" else 0, i + 1, k) for i, k in enumerate(keys)]
    order, _ = _run_sort(program, tmp_path, docs, case["order"] == "DESC")
    page = R.apply_offset_limit(order, case["offset"], case["limit"])
    by_doc = {d: k for _, d, k in docs}
    assert page == P.page(list(by_doc), by_doc.get, case["order"] == "ASC", case["offset"], case["limit"])
    if "expect" in case:
        assert page == case["expect"]
    else:
        assert len(page) == case["expect_size"]


def test_key_derivation_edge_cases(program, tmp_path):
    """(b)"""
    doc = 4_000_000_123
    out = program(["derive %d" % len(EDGE)] + ["%d %d %s" % (k is not None, doc, _hex(k)) for k in EDGE], tmp_path)
    got = {}
    for k, line in zip(EDGE, out):
        tag, numeric, value, key = line.split()
        assert tag == "key"
        got[k] = (int(numeric), int(value), _unhex(key))
        assert _unhex(key) == P.sort_key(doc, k), k
        assert bool(int(numeric)) == (k is None or P.numeric_value(k) is not None), k
    assert got[b"0"] == (1, 0, b"0" * 20)
    assert got[b"7"] == got[b"007"] == (1, 7, b"0" * 19 + b"7")  # two primary keys, one sort key
    assert got[b"18446744073709551615"] == (1, U64, b"18446744073709551615")
    assert got[b"18446744073709551616"] == (0, 0, b"18446744073709551616")  # overflows: the raw bytes
    assert got[b"123456789012345678901"][0] == 0
    assert got[b""] == (0, 0, b"") and got[b"12a"] == (0, 0, b"12a")
    assert got["١٢".encode("utf-8")] == (0, 0, "١٢".encode("utf-8"))  # digits, but not ASCII ones
    assert got[b"\x7f"][0] == 0 and got[b"\x80"][0] == 0
    assert got[None] == (1, doc, b"0000000000%d" % doc)  # no key: the doc id, padded


def _random_keys(rng, n):
    alphabet = [b"a", b"b", b"pk", b"0", b"1", b"9", b"\x00", b"\x7f", b"\x80", b"\xff", "é".encode(), b"A"]
    keys = set(k for k in EDGE if k is not None)
    keys |= {b"pk9", b"pk10", b"pk", b"p", b"00000000000000000007", b"0000000000000000000", b"000000000000000000070",
             b"9223372036854775807", b"9223372036854775808", b"18446744073709551614", b"99999999999999999999"}
    while len(keys) < n:
        r = rng.random()
        if r < 0.35:
            keys.add(b"%d" % rng.choice([rng.randrange(0, 100), rng.getrandbits(64), rng.getrandbits(30)]))
        elif r < 0.45:
            keys.add(b"0" * rng.randrange(1, 4) + b"%d" % rng.randrange(0, 50))  # leading zeros: equal sort keys
        else:
            keys.add(b"".join(rng.choice(alphabet) for _ in range(rng.randrange(1, 6))))
    return sorted(keys, key=lambda k: rng.random())


def test_comparator_on_every_pair_with_both_side_kinds(program, tmp_path):
    """(c) every pair of 300 keys; each key as a rank in two different dictionaries and, when numeric, as its number."""
    rng = random.Random(5)
    keys = _random_keys(rng, 300)
    extra = [b"", b"\x00\x00", b"5", b"zz", b"00000000000000000005", b"pk1", b"\xff\xff"] + [b"x%d" % i for i in range(20)]
    rows = program(["matrix %d %d" % (len(keys), len(extra))] + [_hex(k) for k in keys + extra], tmp_path)
    assert len(rows) == len(keys)
    sk = [P.sort_key(0, k) for k in keys]
    assert any(a == b for i, a in enumerate(sk) for b in sk[i + 1:])  # equal sort keys from different primary keys
    for i, line in enumerate(rows):
        tag, row = line.split()
        want = "".join("<" if sk[i] < sk[j] else ">" if sk[i] > sk[j] else "=" for j in range(len(keys)))
        assert tag == "row" and row == want, (i, keys[i])


@pytest.mark.parametrize("shape", ["numeric_numeric", "numeric_ranks", "ranks_ranks", "missing_keys"])
def test_two_key_columns_merge_like_one_sort(shape, program, tmp_path):
    """PairBefore over the carried pairs of two indexes (complemented in ASC) orders a table as the model does; the
    kinds and the monotone flags are what the data says."""
    rng = random.Random(sum(map(ord, shape)))
    n = 400
    numeric = [b"%d" % v for v in rng.sample(range(0, 5000), n - 6)] + [b"007", b"7", b"0", b"18446744073709551615",
                                                                       b"9223372036854775808", b"9223372036854775807"]
    mixed = _random_keys(rng, n)
    pools = {"numeric_numeric": (numeric, numeric), "numeric_ranks": (numeric, mixed), "ranks_ranks": (mixed, mixed),
             "missing_keys": (numeric, numeric)}[shape]
    docs = []
    for i in range(n):
        side = i % 2
        k = pools[side][i]
        if shape == "missing_keys" and i % 7 == 0:
            k = None
        docs.append((side, 5 + 3 * i, k))
    by_doc = {d: k for _, d, k in docs}
    for descending in (0, 1):
        order, kinds = _run_sort(program, tmp_path, docs, descending)
        assert order == P.sort_docs(list(by_doc), by_doc.get, not descending), (shape, descending)
        assert kinds[:2] == {"numeric_numeric": [0, 0], "numeric_ranks": [0, 1], "ranks_ranks": [1, 1], "missing_keys": [0, 0]}[shape]
        assert kinds[2:] == [0, 0]
    # keys that never decrease with the slot, ties included: monotone, whatever the kind
    for keys in ([b"1", b"01", b"2", b"10"], [b"a", b"a", b"ab", b"b"], [None, None, None]):
        _, kinds = _run_sort(program, tmp_path, [(0, 10 + i, k) for i, k in enumerate(keys)], 1)
        assert kinds[2] == 1, keys
    _, kinds = _run_sort(program, tmp_path, [(0, 10, b"pk9"), (0, 11, b"pk10")], 1)
    assert kinds[0] == 1 and kinds[2] == 0  # bytewise: "pk10" before "pk9"


def test_the_older_model_of_this_branch():
    """(d) column_sort_ref.get_sort_key(("pk", s)) agrees on ASCII keys that are present; it differs on a missing key (""
    there, the padded doc id in the reference) and on non-ASCII digits (str.isdigit takes them, std::isdigit does not)."""
    for k in (b"0", b"7", b"007", b"18446744073709551615", b"18446744073709551616", b"", b"12a", b"pk10"):
        assert R.get_sort_key(9, ("pk", k.decode())) == P.sort_key(9, k), k
    arabic = "١٢"
    assert R.get_sort_key(9, ("pk", arabic)) == R.zero_padded(12) != P.sort_key(9, arabic.encode("utf-8")) == arabic.encode("utf-8")
    assert R.get_sort_key(9, None) == b"" != P.sort_key(9, None) == b"00000000000000000009"


def host_check_lines():
    """Every block above once more, for the sanitizer build (`make pksort-host-asan`)."""
    rng = random.Random(6)
    keys = _random_keys(rng, 120)
    lines = ["derive %d" % len(EDGE)] + ["%d %d %s" % (k is not None, 77, _hex(k)) for k in EDGE]
    lines += ["matrix %d 3" % len(keys)] + [_hex(k) for k in keys + [b"", b"zz", b"5"]]
    for descending in (0, 1):
        lines += sort_block([(i % 2, 5 + i, None if i % 9 == 0 else keys[i]) for i in range(len(keys))], descending)
        lines += sort_block([(i % 2, 5 + i, b"%d" % (1000 - i)) for i in range(50)], descending)
        lines += sort_block([(0, 5 + i, None) for i in range(3)], descending)  # an empty side
    return lines


if __name__ == "__main__":  # the blocks on stdout, for the sanitizer build
    print("\n".join(host_check_lines()))
