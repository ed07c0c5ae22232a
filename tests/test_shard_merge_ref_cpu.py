"""Pins tests/shard_merge_ref.py (the numpy reference of the shard merge) to the oracle: no device needed."""
import numpy as np
import pytest

import shard_merge_ref as R
from oracle import oracle as O

SPECIALS = np.array([-np.inf, -1.7976931348623157e308, -2.5, -1.0, -2.2250738585072014e-308, -5e-324, -0.0, 0.0, 5e-324,
                     2.2250738585072014e-308, 1.0, 1.0000000000000002, 2.5, 1.7976931348623157e308, np.inf])


def test_key_round_trips_and_is_monotone_over_special_values():
    """SPECIALS is strictly increasing in the IEEE total order (-0.0 below +0.0): so must the DESC keys be, the ASC keys
    strictly decreasing, and key_score must give back every bit."""
    for desc in (True, False):
        k = R.score_key(SPECIALS, desc)
        assert k.dtype == np.uint64
        back = R.key_score(k, desc)
        assert np.array_equal(back.view(np.uint64), SPECIALS.view(np.uint64))
        d = np.diff(k.astype(object))
        assert all(x > 0 for x in d) if desc else all(x < 0 for x in d)
    assert R.score_key(np.array([0.0]), True)[0] == np.uint64(1 << 63)
    assert R.score_key(np.array([-0.0]), True)[0] == np.uint64((1 << 63) - 1)
    assert np.array_equal(R.score_key(SPECIALS, False), ~R.score_key(SPECIALS, True))


def test_key_round_trips_on_random_bit_patterns():
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 1 << 63, size=4000, dtype=np.uint64) | (rng.integers(0, 2, size=4000, dtype=np.uint64) << np.uint64(63))
    s = bits.view(np.float64)
    s = s[~np.isnan(s)]
    for desc in (True, False):
        k = R.score_key(s, desc)
        assert np.array_equal(R.key_score(k, desc).view(np.uint64), s.view(np.uint64))
        order = np.argsort(s, kind="stable")
        ks = k[order].astype(object)
        same = np.diff(s[order]) == 0  # (no +-0.0 pair among random patterns: equal doubles are equal bits)
        step = np.diff(ks)
        assert all((x == 0) if e else ((x > 0) if desc else (x < 0)) for x, e in zip(step, same))


@pytest.mark.parametrize("descending", [True, False])
@pytest.mark.parametrize("n_shards,needed_limit_offset", [(1, (10, 0)), (2, (10, 3)), (3, (37, 5)), (7, (100, 24)),
                                                           (16, (1, 0)), (5, (1000, 24))])
def test_merge_page_equals_sort_by_score_over_the_union(descending, n_shards, needed_limit_offset):
    """Heavy ties (five distinct scores, no -0.0): the page of the merged per-shard top lists is ResultSorter::SortByScore
    over everything the shards hold. A shard cuts its own list at offset + limit first, as the device does."""
    limit, offset = needed_limit_offset
    needed = limit + offset
    rng = np.random.default_rng(100 * n_shards + needed + int(descending))
    values = np.array([0.0, 0.5, 1.25, 1.25000000000001, 7.0])
    all_docs = rng.permutation(np.arange(1, 1 + 60 * n_shards * 40, dtype=np.uint32))
    lists, union_docs, union_scores = [], [], []
    at = 0
    for r in range(n_shards):
        m = int(rng.integers(0, 2 * needed + 3))
        docs = all_docs[at:at + m]
        at += m
        scores = values[rng.integers(0, len(values), size=m)]
        union_docs.append(docs)
        union_scores.append(scores)
        s, d = R.sort_list(scores, docs, descending)
        lists.append((s[:needed], d[:needed], m))
    total, page, page_scores = R.merge_page(lists, descending, limit, offset)
    ud, us = np.concatenate(union_docs), np.concatenate(union_scores)
    want = O.sort_by_score(ud, us, descending, limit, offset)
    assert total == len(ud)
    assert page.tolist() == want.tolist()
    lookup = dict(zip(ud.tolist(), us.tolist()))
    assert page_scores.tolist() == [lookup[d] for d in want.tolist()]


def test_pack_blob_layout():
    """[keys n*stride | totals n] u64 then [doc' n*stride | counts n] u32, padded to 8 bytes, poison past the counts."""
    lists = [(np.array([2.0, 1.0]), np.array([9, 4], np.uint32), 1 << 33), (np.zeros(0), np.zeros(0, np.uint32), 0),
             (np.array([1.0]), np.array([7], np.uint32), 1)]
    raw = R.pack_blob(lists, [True, True, False], stride=3)
    nbytes, off32 = R.blob_bytes(3, 3)
    assert (nbytes, off32) == (144, 96) and len(raw) == 144
    b64, b32 = raw[:off32].view(np.uint64), raw[off32:].view(np.uint32)
    assert b64[:2].tolist() == R.score_key(np.array([2.0, 1.0]), True).tolist()
    assert b64[2] == np.uint64(0xFFFFFFFFFFFFFFFF) and b64[3] == np.uint64(0xFFFFFFFFFFFFFFFF)
    assert b64[6] == R.score_key(np.array([1.0]), False)[0]
    assert b64[9:12].tolist() == [1 << 33, 0, 1]
    assert b32[:2].tolist() == [9, 4] and b32[6] == 0xFFFFFFFF - 7
    assert b32[9:12].tolist() == [2, 0, 1]
    buf, pitch = R.gather_blobs([raw, raw], pitch_pad=64)
    assert pitch == 208 and len(buf) == 416
    assert np.array_equal(buf[208:352], raw) and (buf[144:208] == 0xFF).all()
