"""bench_latency.py without a GPU: its argument parsing, the equality check that gates the timing, and the
per-cell summary (p50 / p99, the spread of the per-repeat p50s, the judged claim).  The measurement itself needs a
GPU and has no fallback."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_latency as B  # noqa: E402

from kcp_amd import gpudiff as G  # noqa: E402


def test_defaults_are_the_documented_table():
    a = B.parse_args([])
    assert a.sizes == [1, 16, 256, 4096] and a.reps >= 200 and a.reps_large >= 50 and a.repeats == 5
    assert a.populations == ["deployment", "configmap_secret", "deep_crd"]
    assert a.paths == ["resident", "submit_host", "submit_device"]
    assert max(a.sizes) == G.SMALL_PASS_MAX_PAIRS


@pytest.mark.parametrize("argv", [["--sizes", "0"], ["--populations", "pods"], ["--paths", "resident,async"],
                                  ["--reps", "0"], ["--repeats", "0"]])
def test_bad_arguments_are_refused(argv):
    with pytest.raises(SystemExit):
        B.parse_args(argv)


def _result(**over):
    r = dict(pair_flags=np.array([1, 0, 3], np.uint8), spec_dirty_ids=np.array([0, 2], np.uint32),
             status_dirty_ids=np.array([2], np.uint32), dirty_ids=np.array([0, 2], np.uint32),
             path_offsets=np.array([0, 1, 3], np.uint32), path_hashes=np.array([7, 8, 9], np.uint64),
             path_kinds=np.array([0, 0, 0x83], np.uint8))
    r.update(over)
    return G.DiffResult(**r)


def test_equality_check_names_the_array_that_differs():
    assert B.results_differ(_result(), _result()) is None
    assert B.results_differ(_result(), _result(path_kinds=np.array([0, 0, 0x80], np.uint8))) == "path_kinds"
    assert B.results_differ(_result(), _result(pair_flags=np.array([1, 0, 3, 0], np.uint8))) == "pair_flags"
    assert B.results_differ(_result(), _result(dirty_ids=np.array([0, 2], np.uint64))) == "dirty_ids"
    assert list(B.ARRAYS) == list(_result().__dataclass_fields__)[:7]  # every result array of a DiffResult


def test_summary_and_the_judged_claim():
    off = [[100.0] * 9 + [400.0], [104.0] * 10, [98.0] * 10]
    on = [[60.0] * 10, [61.0] * 10, [59.0] * 10]
    s = B.summarise(off, on)
    assert s["off"]["p50_us"] == 100.0 and s["off"]["p99_us"] == 400.0 and s["off"]["p50_spread_us"] == 6.0
    assert s["on"]["p50_us"] == 60.0 and s["on"]["p50_spread_us"] == 2.0
    assert s["p50_gain_us"] == 40.0 and s["gain_exceeds_off_spread"] is True
    s = B.summarise(off, [[97.0] * 10] * 3)  # a gain inside the baseline's own spread is no gain
    assert s["p50_gain_us"] == 3.0 and s["gain_exceeds_off_spread"] is False


def test_help_runs_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench_latency.py"), "--help"], capture_output=True,
                       text=True, timeout=60, cwd=ROOT)
    assert r.returncode == 0 and "--reps-large" in r.stdout
