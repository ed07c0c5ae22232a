"""Plain numpy restatement of the shard merge (mgx_batch_merge_shards) and of the exchange layout it reads
(include/mygram_gpu.h, mgx_batch_export_topk). Nothing here needs a device.

A shard's list for one query is (scores fp64, doc ids u32, total): its best-first top-(offset+limit) and how many
documents it matched in all. On the wire a score travels as its order-preserving u64 key (score_key of mgx_kernels.hip)
and a doc id d as doc' = d for DESC and ~d for ASC, so that "larger (key, doc') is better" is the
ResultSorter::SortByScore comparator in both directions."""
import numpy as np

_SIGN = np.uint64(1 << 63)


def score_key(scores, descending):
    """Order-preserving u64 of fp64 scores: larger key = better (higher score for DESC, lower for ASC)."""
    u = np.ascontiguousarray(scores, dtype=np.float64).view(np.uint64)
    u = np.where((u >> np.uint64(63)).astype(bool), ~u, u | _SIGN)
    return u if descending else ~u


def key_score(keys, descending):
    """The inverse of score_key."""
    u = np.ascontiguousarray(keys, dtype=np.uint64)
    u = u if descending else ~u
    u = np.where((u >> np.uint64(63)).astype(bool), u & ~_SIGN, ~u)
    return np.ascontiguousarray(u).view(np.float64)


def doc_prime(docs, descending):
    d = np.ascontiguousarray(docs, dtype=np.uint32)
    return d if descending else ~d


def sort_list(scores, docs, descending):
    """One shard's entries best first, as a shard exports them."""
    scores, docs = np.asarray(scores, np.float64), np.asarray(docs, np.uint32)
    order = np.lexsort((doc_prime(docs, descending), score_key(scores, descending)))[::-1]
    return scores[order], docs[order]


def merge_page(lists, descending, limit, offset):
    """lists: per shard (scores, docs, total), each best first. -> (total, page doc ids, page scores): the union of every
    shard's entries by (key, doc') descending, cut at offset + limit, page [offset, offset + limit)."""
    keys = np.concatenate([score_key(s, descending) for s, _, _ in lists]) if lists else np.zeros(0, np.uint64)
    dp = np.concatenate([doc_prime(d, descending) for _, d, _ in lists]) if lists else np.zeros(0, np.uint32)
    order = np.lexsort((dp, keys))[::-1][: offset + limit][offset:]
    return (sum(int(t) for _, _, t in lists), doc_prime(dp[order], descending).astype(np.uint32),
            key_score(keys[order], descending))


def blob_bytes(n_queries, stride):
    """Bytes of one rank's packed blob (blob64 then blob32, padded to a multiple of 8) and the offset of blob32."""
    elems = n_queries * stride + n_queries
    return (12 * elems + 7) // 8 * 8, 8 * elems


def pack_blob(lists, directions, stride, poison=0xFF):
    """One rank's blob for a batch of len(lists) queries: [keys n*stride | totals n] as u64, then
    [doc' n*stride | counts n] as u32. lists[q] = (scores, docs, total) of query q, directions[q] = its `descending`.
    Slots past a query's count hold `poison` bytes: they are not part of the list."""
    n = len(lists)
    nbytes, off32 = blob_bytes(n, stride)
    raw = np.full(nbytes, poison, dtype=np.uint8)
    b64 = raw[:off32].view(np.uint64)
    b32 = raw[off32:off32 + 4 * (n * stride + n)].view(np.uint32)
    for q, ((scores, docs, total), desc) in enumerate(zip(lists, directions)):
        c = len(docs)
        assert c == len(scores) and c <= stride
        b64[q * stride:q * stride + c] = score_key(scores, desc)
        b32[q * stride:q * stride + c] = doc_prime(docs, desc)
        b64[n * stride + q] = np.uint64(total)
        b32[n * stride + q] = c
    return raw


def gather_blobs(blobs, pitch_pad=0, poison=0xFF):
    """Rank r's blob at r * (nbytes + pitch_pad) of one buffer; the padding holds `poison` bytes."""
    assert pitch_pad % 8 == 0
    nbytes = len(blobs[0])
    pitch = nbytes + pitch_pad
    out = np.full(pitch * len(blobs), poison, dtype=np.uint8)
    for r, b in enumerate(blobs):
        assert len(b) == nbytes
        out[r * pitch:r * pitch + nbytes] = b
    return out, pitch
