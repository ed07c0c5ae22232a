"""SORT by primary key as the reference does it (GetSortKey's primary-key branch, src/query/result_sorter.cpp:239-262),
for the tests of mygram-db_amd/csrc/mgx_pkey.hpp. A primary key is `bytes`, or None for a document without one.

column_sort_ref.get_sort_key models the same branch for the reference's own vectors, with two shortcuts those vectors
never meet: a missing key is "" there (the reference falls back to the doc id, :258-261), and it asks str.isdigit, which
accepts digits outside ASCII (the reference asks std::isdigit byte by byte in the C locale, :247-248). This module wraps
it and states both exactly; where the two agree, test_primary_key_sort_cpu.py checks that they do."""
import column_sort_ref as R

U64 = R.U64


def numeric_value(pk):
    """The number of a numeric primary key (:247-253; from_chars reports out of range past 2^64 - 1), else None."""
    if pk and all(0x30 <= b <= 0x39 for b in pk) and int(pk) <= U64:
        return int(pk)
    return None


def sort_key(doc_id, pk):
    if pk is None:
        return R.zero_padded(doc_id)  # :258-261
    v = numeric_value(pk)
    return pk if v is None else R.zero_padded(v)  # :256 | :165


def sort_docs(doc_ids, pk_of, ascending):
    """CompareSortEntries (:47-54): keys compare bytewise, ties go to the doc id in the sort's own direction."""
    entries = sorted(((sort_key(d, pk_of(d)), d) for d in doc_ids), reverse=not ascending)
    return [d for _, d in entries]


def page(doc_ids, pk_of, ascending, offset, limit):
    s = sort_docs(doc_ids, pk_of, ascending)
    return R.apply_offset_limit(s, offset, limit if limit else len(s))


def pack(keys):
    """[bytes | None] by slot -> (bytes, off, has_key) as mgx_index_set_primary_keys takes them."""
    import numpy as np
    blob = b"".join(k or b"" for k in keys)
    off = np.zeros(len(keys) + 1, np.uint64)
    np.cumsum([len(k or b"") for k in keys], out=off[1:])
    has = np.asarray([k is not None for k in keys], np.uint8)
    return np.frombuffer(blob, np.uint8).copy() if blob else np.zeros(0, np.uint8), off, has
