"""bench.py's command line: a plain run measures the headline alone; --full adds every other leg, and the --no-* flags and
--legs act on what --full adds, as they did before it existed (no GPU needed)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N1_FULL = {"roofline", "traffic", "configs", "record_shapes", "cpu_baseline"}


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _legs(bench, argv, world=1):
    return bench.extra_legs(bench.parse_args(argv), world)


@pytest.mark.parametrize("argv", [
    [],
    ["--gpus", "1", "--steps", "20", "--warmup", "5"],
    ["--dump-outputs", "out"],
    ["--no-traffic", "--no-configs", "--no-cpu-baseline", "--legs", "record_shapes"],
])
@pytest.mark.parametrize("world", [1, 2, 8])
def test_a_plain_run_has_no_extra_legs(bench, argv, world):
    assert bench.parse_args(argv).full is False
    assert _legs(bench, argv, world) == set()


def test_full_on_one_gpu_runs_every_leg(bench):
    assert _legs(bench, ["--full"]) == N1_FULL
    assert _legs(bench, ["--full", "--gpus", "1", "--steps", "20", "--warmup", "5"]) == N1_FULL


@pytest.mark.parametrize("argv,gone", [
    (["--no-traffic"], {"traffic"}),
    (["--gb", "1"], {"traffic"}),           # the counters are taken at the headline size only
    (["--algo", "3"], {"traffic"}),
    (["--no-configs"], {"configs", "record_shapes"}),
    (["--legs", "end_to_end_vcf"], {"record_shapes"}),
    (["--legs", "end_to_end_vcf,record_shapes"], set()),
    (["--no-cpu-baseline"], {"cpu_baseline"}),
    (["--no-configs", "--no-cpu-baseline", "--no-traffic"], {"traffic", "configs", "record_shapes", "cpu_baseline"}),
])
def test_full_flags_leave_out_what_they_name(bench, argv, gone):
    assert _legs(bench, ["--full"] + argv) == N1_FULL - gone


def test_full_on_several_ranks(bench):
    assert _legs(bench, ["--full", "--gpus", "2"], world=2) == {"roofline", "reader_sharded"}
    assert _legs(bench, ["--full", "--gpus", "8", "--no-configs"], world=8) == {"roofline"}
