"""An in-process sharded table: every shard of mygram_db_amd.dist.shard_range as its own mg.Index on device 0, and the
test as the transport between them. It walks the steps of dist.ShardedTable.run's non-RCCL branch through the public
entry points (count_df / df_buffer, execute / execute_gather, export_buffer / export_topk, merge_shards, fetch) without
torch.distributed, so any world size runs in one process on one GPU."""
import numpy as np
import torch

from gpu_util import OracleSide
from mygram_db_amd import dist as mdist
from pkg import mg


class SeedExchangeCalled(AssertionError):
    pass


def _no_gather(mine_ptr, all_ptr, nbytes):
    raise SeedExchangeCalled("the seed exchange ran on a small shard (gather of %d bytes)" % nbytes)


class LocalShards:
    def __init__(self, texts, world, ngram=2, kanji=0, cross=True, dense_threshold=0.0, oracle=None):
        """oracle: an OracleSide over the same texts and n-gram settings to share between world sizes (else built here)."""
        self.world = world
        self.device = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        if oracle is None:
            corpus = mg.Corpus.from_texts(texts)
            oracle = OracleSide(mg.Columns(corpus, 1, ngram, kanji, cross), corpus)
        self.oracle = oracle
        cols = oracle.columns
        assert (cols.ngram_size, cols.kanji_ngram_size, bool(cols.cross_boundary)) == (ngram, kanji, bool(cross))
        # the table-wide statistics of dist.global_table_stats, from the whole corpus' columns
        whole = {cols.gram(g): int(s) for g, s in enumerate(np.diff(cols.offsets.astype(np.int64)).tolist())}
        n, total_len = int(cols.bm25_doc_count), int(cols.bm25_total_len)
        self.ranges = [mdist.shard_range(len(texts), r, world) for r in range(world)]
        self.shards = []
        for before, mine in self.ranges:
            idx = mg.Index(corpus=mg.Corpus.from_texts(texts[before:before + mine]), first_doc_id=1 + before,
                           ngram_size=ngram, kanji_ngram_size=kanji, cross_boundary=cross, device=0,
                           dense_threshold=dense_threshold)
            c = idx.columns
            idx._global_sizes = np.asarray([whole[c.gram(g)] for g in range(c.n_grams)], dtype=np.int64)
            idx._global_dict = whole
            idx.total_docs = n
            idx.avg_doc_length = (total_len / n) if n else 0.0
            self.shards.append(idx)

    def prepare(self, queries):
        """The same queries on every shard."""
        return [idx.prepare(queries) for idx in self.shards]

    @staticmethod
    def _bytes(ptr, nbytes):
        return mdist._device_bytes(ptr, nbytes)

    def run_prepared(self, batches, pitch_pad=0, through_gather=False):
        """Executes, exchanges and merges `batches` (one per shard, from prepare) -> the fetched results of every shard.
        through_gather: execute through execute_gather(world, gather) with a gather that fails the test when called."""
        assert pitch_pad % 8 == 0
        stream = torch.cuda.current_stream().cuda_stream
        if not batches[0].n:  # (every query resolved on the host: the same on every shard, nothing to exchange)
            assert all(b.n == 0 for b in batches)
            return [b.fetch() for b in batches]
        # text-level df: the all-reduce by hand
        bufs = [b.df_buffer() for b in batches]
        n_tt = bufs[0][1]
        assert all(n == n_tt for _, n in bufs)
        if n_tt:
            for b in batches:
                b.count_df(stream)
            views = [self._bytes(ptr, 8 * n_tt).view(torch.int64) for ptr, _ in bufs]
            total = torch.stack(views).sum(dim=0)
            for v in views:
                v.copy_(total)
        for b in batches:
            if through_gather:
                b.execute_gather(self.world, _no_gather, stream)
            else:
                b.execute(stream)
        # export: every rank's blob, laid into one buffer rank after rank (the all-gather)
        blobs, off32, nbytes = [], None, None
        for b in batches:
            ptr, nb, o32 = b.export_buffer()
            if ptr:
                blob = self._bytes(ptr, nb)
            else:
                stride = b.topk_stride()
                elems = b.n * stride + b.n
                o32, nb = 8 * elems, (12 * elems + 7) // 8 * 8
                blob = torch.zeros(nb, dtype=torch.uint8, device=self.device)
                b.export_topk(blob.data_ptr(), blob.data_ptr() + o32, stream)
            assert (off32, nbytes) in ((None, None), (o32, nb)), "every rank's blob has the same layout"
            off32, nbytes = o32, nb
            blobs.append(blob)
        pitch = nbytes + pitch_pad
        gathered = torch.full((pitch * self.world,), 0xFF, dtype=torch.uint8, device=self.device)
        for r, blob in enumerate(blobs):
            gathered[r * pitch:r * pitch + nbytes].copy_(blob)
        out = []
        for b in batches:
            b.merge_shards(self.world, gathered.data_ptr(), gathered.data_ptr() + off32, stream,
                           pitch64=pitch // 8, pitch32=pitch // 4)
            out.append(b.fetch())
        return out

    def run(self, queries, pitch_pad=0):
        """prepare + run_prepared, then once more on the same batches through execute_gather: the same pages."""
        batches = self.prepare(queries)
        first = self.run_prepared(batches, pitch_pad)
        again = self.run_prepared(batches, pitch_pad, through_gather=True)
        for a, b in zip(first, again):
            for x, y in zip(a, b):
                assert x.total == y.total and x.docs.tolist() == y.docs.tolist() and np.array_equal(x.scores, y.scores)
        return again

    def check(self, queries, results, want=None):
        """Every rank's fetched results against the oracle on the whole table: total, page doc ids, fp64 scores, all
        exact. want: the oracle's answers when the caller already holds them (oracle_query per query)."""
        if want is None:
            want = [self.oracle.oracle_query(q) for q in queries]
        assert len(results) == self.world and len(want) == len(queries)
        for rank, got in enumerate(results):
            assert len(got) == len(queries)
            for q, g, (total, page, scores, _) in zip(queries, got, want):
                ctx = (self.world, rank, q.terms, q.not_terms, q.sort_score, q.limit, q.offset, q.descending)
                assert g.total == total, (ctx, g.total, total)
                assert g.docs.tolist() == page.tolist(), (ctx, g.docs.tolist()[:8], page.tolist()[:8])
                if q.sort_score:
                    assert np.array_equal(g.scores, scores), (ctx, g.scores[:8], scores[:8])
        return want
