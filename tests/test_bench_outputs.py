"""bench.py --dump-outputs / --full.

CPU: dump_outputs writes a diff pass's results as float32 / float64 arrays that reproduce the integers
exactly, cuts a long array to the same seeded sample every time and records full sizes and checksums.
GPU: a plain run (no --full) prints the headline line without the legs that need runs of their own, honours
--steps, and the arrays it dumps are those of a single-context diff of the same seeded population."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pair_flags", "spec_dirty_ids", "status_dirty_ids", "dirty_ids", "path_offsets", "path_hashes_lo",
         "path_hashes_hi", "path_kinds", "sizes", "checksums"]


def _load(d):
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in NAMES)
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}


def test_dump_outputs_exact_sampled_and_repeatable(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    from kcp_amd.gpudiff import DiffResult

    monkeypatch.setitem(bench.DUMP_CAP, np.float32, 1000)
    monkeypatch.setitem(bench.DUMP_CAP, np.float64, 100)
    rng = np.random.default_rng(1)
    n, nd, npth = 5000, 300, 90
    res = DiffResult(pair_flags=rng.integers(0, 8, n).astype(np.uint8),
                     spec_dirty_ids=np.unique(rng.integers(0, 1 << 32, 2 * nd, dtype=np.uint64))[:nd].astype(np.uint32),
                     status_dirty_ids=np.arange(7, dtype=np.uint32) + np.uint32(0xFFFFFFF0),
                     dirty_ids=np.arange(nd, dtype=np.uint32),
                     path_offsets=np.arange(nd + 1, dtype=np.uint32),
                     path_hashes=rng.integers(0, 1 << 63, npth, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                     path_kinds=rng.integers(0, 4, npth).astype(np.uint8))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, res)
    bench.dump_outputs(b, res)
    da, db = _load(a), _load(b)
    for k in NAMES:
        assert da[k].dtype in (np.float32, np.float64) and np.array_equal(da[k], db[k]), k
    assert da["sizes"].tolist() == [n, nd, 7, nd, nd + 1, npth, npth]
    # short arrays are whole and exact, the 64-bit hashes from their halves
    assert np.array_equal(da["status_dirty_ids"].astype(np.uint32), res.status_dirty_ids)
    assert np.array_equal(da["path_kinds"].astype(np.uint8), res.path_kinds)
    h = (da["path_hashes_hi"].astype(np.uint64) << np.uint64(32)) | da["path_hashes_lo"].astype(np.uint64)
    assert np.array_equal(h, res.path_hashes)
    # long ones are an in-order sample of the array's own elements
    assert da["pair_flags"].size == 1000 and da["spec_dirty_ids"].size == 100
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(nd, 100, replace=False))
    assert np.array_equal(da["spec_dirty_ids"].astype(np.uint32), res.spec_dirty_ids[idx])
    # checksums: the sum mod 2^64 of every full array as (low, high) halves
    cs = da["checksums"].astype(np.uint64).reshape(7, 2)
    want = [int(getattr(res, f).sum(dtype=np.uint64)) for f in
            ("pair_flags", "spec_dirty_ids", "status_dirty_ids", "dirty_ids", "path_offsets", "path_hashes",
             "path_kinds")]
    assert [int(lo) | (int(hi) << 32) for lo, hi in cs] == want
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) < 64 << 20


def test_dump_caps_fit_64_mb():
    sys.path.insert(0, ROOT)
    import bench
    # two float32 arrays, six float64 arrays at their caps, sizes and checksums, ten .npy headers
    total = 2 * 4 * bench.DUMP_CAP[np.float32] + 6 * 8 * bench.DUMP_CAP[np.float64] + 8 * (7 + 14) + 10 * 128
    assert total <= 64 * 1000 * 1000


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    return json.loads(lines[0]), r.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    from kcp_amd import gpudiff as G
    from kcp_amd import synth as S

    n, steps = 30000, 3
    common = ["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--pairs", str(n), "--clusters", "300",
              "--threads", "8"]
    a = str(tmp_path / "a")
    line, err = _bench(common + ["--dump-outputs", a])
    assert line["steps"] == steps and ("timed region: %d steps" % steps) in err
    assert line["unit"] == "pairs/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    # none of the legs that take runs of their own
    assert line["full"] is False
    assert line["roofline"] is None and line["kernels_ms"] is None and line["cpu_baseline"] is None
    assert line["json_in"] is None and line["checks"]["full_size"] is None and line["checks"]["sample"] is None
    for marker in ("full-size check", "json-in", "cpu baseline", "three-way"):
        assert marker not in err
    da = _load(a)
    assert all(da[k].dtype in (np.float32, np.float64) for k in NAMES)
    # the same population through one context
    cfg = S.make_cfg("config3", n_pairs=n, n_clusters=300)
    pop = S.Population(cfg)
    e = G.Engine(device=0, encode_threads=8)
    ch = pop.chunk(e, 0, pop.n, 8)
    dbatch = e.device_batch(ch.pool_bytes + 4096, pop.n)
    dbatch.append(ch.hb)
    res = e.wait(e.diff(dbatch))
    assert np.array_equal(da["pair_flags"].astype(np.uint8), res.pair_flags)
    assert np.array_equal(da["spec_dirty_ids"].astype(np.uint32), res.spec_dirty_ids)
    assert np.array_equal(da["status_dirty_ids"].astype(np.uint32), res.status_dirty_ids)
    assert np.array_equal(da["dirty_ids"].astype(np.uint32), res.dirty_ids)
    assert np.array_equal(da["path_offsets"].astype(np.uint32), res.path_offsets)
    h = (da["path_hashes_hi"].astype(np.uint64) << np.uint64(32)) | da["path_hashes_lo"].astype(np.uint64)
    assert np.array_equal(h, res.path_hashes)
    assert np.array_equal(da["path_kinds"].astype(np.uint8), res.path_kinds)
    assert res.dirty_ids.size > 100 and res.path_hashes.size >= res.dirty_ids.size
    dbatch.free()
    ch.hb.free()
    e.close()
