"""bench.py's options, without a GPU: a plain run measures the headline leg alone; --full adds the extra legs and the CPU
oracle exactly where the default run of the parent did."""
import bench


def extras(argv, world=1):
    return bench.full_extras(bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"] + argv), world)


def test_plain_run_adds_nothing():
    args = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not args.full and (args.mode, args.precision, args.batch) == ("full", "mixed", 64)
    assert extras([]) == (False, False)
    assert extras(["--dump-outputs", "out"]) == (False, False)


def test_full_adds_legs_and_oracle():
    assert extras(["--full"]) == (True, True)
    assert extras(["--full", "--no-extra-legs"]) == (False, True)
    assert extras(["--full", "--no-cpu-baseline"]) == (True, False)
    assert extras(["--full"], world=2) == (False, False)                  # N > 1: neither, as before


def test_full_legs_only_on_the_plain_default_workload():
    for ab in (["--no-overlap"], ["--no-fuse-mlp"], ["--attn-variant", "0"], ["--mode", "backbone"], ["--segmentation", "grid"],
               ["--stego-reading", "patch"]):
        assert extras(["--full"] + ab) == (False, True), ab
