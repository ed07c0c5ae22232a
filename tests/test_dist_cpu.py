"""world_size-2 gloo rehearsal of the doc-range sharding (CPU only; see tests/dist_worker.py)."""
import os
import subprocess
import sys

from pkg import ROOT


def _launch(mode, timeout=600):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", "29533", os.path.join(ROOT, "tests", "dist_worker.py"), mode]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2, r.stdout


def test_sharding_design_world2_gloo():
    _launch("cpu")


def test_shard_range_partitions_the_doc_range():
    """dist.shard_range for every n in 0..40 and world in 1..9: the ranges are contiguous, disjoint, in rank order and
    sum to n. What the code does with the remainder: every shard holds per = ceil(n / world) docs until the docs run out,
    then one shard holds what is left (fewer than per), and every rank after it holds an EMPTY range that starts at n.
    Empty shards therefore occur whenever n < world (n of the ranks hold one doc each), and also for some n >= world
    (n = 9, world = 4: 3 + 3 + 3 + 0); no rank is ever given a range outside [0, n)."""
    from pkg import mg  # noqa: F401  (the package under its importable name)
    from mygram_db_amd.dist import shard_range
    for n in range(41):
        for world in range(1, 10):
            per = -(-n // world)
            at = 0
            seen_short = False
            for rank in range(world):
                before, count = shard_range(n, rank, world)
                assert before == at, (n, world, rank)
                assert 0 <= count <= per and before + count <= n, (n, world, rank)
                if seen_short:
                    assert count == 0 and before == n, (n, world, rank)
                elif count < per:
                    seen_short = True
                at += count
            assert at == n, (n, world)
            assert sum(1 for r in range(world) if shard_range(n, r, world)[1] == 0) == world - (-(-n // per) if per else 0)
    assert [shard_range(9, r, 4) for r in range(4)] == [(0, 3), (3, 3), (6, 3), (9, 0)]
    assert [shard_range(2, r, 3) for r in range(3)] == [(0, 1), (1, 1), (2, 0)]
    assert [shard_range(0, r, 2) for r in range(2)] == [(0, 0), (0, 0)]
