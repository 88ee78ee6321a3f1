"""bench.py's command line: a plain run does only the headline figure's work (no aging, no CPU
baseline); --full brings back the aged window and the CPU baseline; --dump-outputs stops the
replayed pools at the batch the run's steps reach."""
import bench


def test_plain_run_is_lean():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup) == (7, 2)
    assert a.full is False and a.age_seconds == 0.0 and a.cpu_baseline is False and a.dump_outputs is None
    # what a caller asks for explicitly still holds
    assert bench.parse(["--age-seconds", "30"]).age_seconds == 30.0


def test_full_run_ages_and_runs_the_cpu_baseline():
    a = bench.parse(["--full"])
    assert a.age_seconds == 400.0 and a.age_games == 3.0 and a.cpu_baseline is True
    assert bench.parse(["--full", "--no-cpu-baseline"]).cpu_baseline is False
    assert bench.parse(["--full", "--age-seconds", "0"]).age_seconds == 0.0
    assert bench.parse(["--no-cpu-baseline"]).cpu_baseline is False


def test_dump_pools():
    """The replayed pools fill a launch as the launcher does, and reach the large-launch kernel."""
    a = bench.parse([])                                         # 256-game pools, launches held for 1,024 rows
    assert bench.dump_pools(a, 32, 257, 32) == 4
    a = bench.parse(["--batch", "64", "--min-launch-rows", "0"])
    assert bench.dump_pools(a, 8, 257, 32) == 5                 # 5 x 64 = 320 >= 257
    assert bench.dump_pools(a, 4, 257, 32) == 4                 # no more pools than the run has
    assert bench.dump_pools(bench.parse(["--batch", "16"]), 64, 257, 32) == 32   # nor than a launch's segments


def test_dump_not_with_roll():
    import pytest
    with pytest.raises(SystemExit):
        bench.parse(["--roll", "--dump-outputs", "d"])


def test_dump_polls():
    a = bench.parse(["--steps", "2", "--warmup", "1", "--step-rows", "65536", "--dump-outputs", "d"])
    assert a.dump_outputs == "d"
    assert bench.dump_polls(a, 256) == 768          # 3 steps x 65,536 evaluations over 256 game slots
    assert bench.dump_polls(a, 64) == bench.DUMP_MAX_POLLS
    a = bench.parse(["--steps", "0", "--warmup", "0"])
    assert bench.dump_polls(a, 8192) == 1
