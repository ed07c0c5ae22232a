"""bench.py's command line: --full, off by default, adds what runs after the timed steps (no device needed)."""
import bench


def test_full_is_off_by_default():
    args = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert (args.gpus, args.steps, args.warmup, args.dump_outputs, args.full) == (1, 3, 1, None, False)
    assert bench.parse_args(["--full"]).full is True
