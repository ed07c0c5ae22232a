"""Worker of tests/test_gpu_dist.py::test_seed_bound_exchange_world2: two ranks (gloo) share the box's GPU, each holds a
1.2M-doc shard — large enough for seed items —, and run SORT _score batches through ShardedTable.run, i.e. through
mgx_batch_execute_gather: the ranks' seed keys are all-gathered and every query's pruning bound is raised to the
(offset+limit)-th best of the union before the rest of the batch runs. Checked against the UNSHARDED index of the same
table on the same device (that path is held against the oracle by the other GPU tests): totals, pages, scores of every
query identical."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402

mg = entry.load_package()
import bench as B  # noqa: E402
from mygram_db_amd import dist as mdist  # noqa: E402

N_DOCS = 2_400_000


def main():
    os.environ["MGX_VERBOSE"] = "1"
    os.environ["MGX_SEED_EXCHANGE"] = "1"  # (by default only tables cut eight ways and more exchange their seeds)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    before, mine = mdist.shard_range(N_DOCS, rank, world)
    corpus = mg.Corpus.synthetic(mine, seed=42, global_first=before)
    table = mdist.ShardedTable(corpus, first_doc_id=1 + before, device=0, ngram_size=2, kanji_ngram_size=0,
                               dense_threshold=0.0)
    terms = B.make_queries(mg, table, 1, 384)[0]
    Q = mg.engine.Query
    qs = []
    for i, t in enumerate(terms):
        if i % 7 == 3:
            qs.append(Q(t, sort_score=True, limit=100))
        elif i % 7 == 5:
            qs.append(Q(t[:2], sort_score=True, limit=10, offset=5))
        elif i % 11 == 0:
            qs.append(Q(t, sort_score=True, limit=10, descending=False))  # ASC: no pruning, no seed keys
        else:
            qs.append(Q(t, sort_score=True, limit=10))
    batch = table.prepare(qs)
    for _ in range(2):
        table.run(batch)
        got = batch.fetch()
    whole = mg.Index(corpus=mg.Corpus.synthetic(N_DOCS, seed=42), ngram_size=2, kanji_ngram_size=0)
    want = whole.search_batch(qs)
    hits = 0
    for q, g, w in zip(qs, got, want):
        assert g.total == w.total, (q.terms, g.total, w.total)
        assert g.docs.tolist() == w.docs.tolist(), (q.terms, q.limit, q.offset, q.descending)
        assert np.array_equal(g.scores, w.scores), q.terms
        hits += w.total > 0
    assert hits > 300
    # away from the default BM25 parameters: the seeds' keys and the exchanged bounds are scores at (k1, b); the
    # unsharded index answers the same, and on rank 0 a sample is held against the oracle at those parameters too
    qs2 = [Q(q.terms, sort_score=True, limit=q.limit, offset=q.offset, descending=q.descending,
             k1=(2.0, 0.3, 20.0)[i % 3], b=(0.3, 1.0, 0.0)[i % 3]) for i, q in enumerate(qs)]
    batch2 = table.prepare(qs2)
    table.run(batch2)
    got2 = batch2.fetch()
    want2 = whole.search_batch(qs2)
    for q, g, w in zip(qs2, got2, want2):
        assert g.total == w.total, (q.terms, q.k1, q.b, g.total, w.total)
        assert g.docs.tolist() == w.docs.tolist(), (q.terms, q.k1, q.b, q.limit, q.offset, q.descending)
        assert np.array_equal(g.scores, w.scores), (q.terms, q.k1, q.b)
    if rank == 0:
        from oracle import oracle as O
        c = whole.columns
        o_idx = O.Index.from_csr(2, 0, True, c.key_bytes, c.key_off, c.offsets, c.docids)
        o_store = O.DocumentStore.from_arrays(whole.corpus.text_bytes, whole.corpus.text_off)
        for q, g in list(zip(qs2, got2))[:12]:
            total, docs, scores = O.search_scored(o_idx, o_store, [O.normalize_text(t) for t in q.terms],
                                                  whole.total_docs, whole.avg_doc_length, q.k1, q.b, q.descending,
                                                  q.limit, q.offset)
            assert g.total == total and g.docs.tolist() == docs.tolist(), (q.terms, q.k1, q.b)
            assert np.array_equal(g.scores, scores), (q.terms, q.k1, q.b)
    print("ok")


if __name__ == "__main__":
    main()
