#!/usr/bin/env python3
"""Latency of small diff passes, with GPUDIFF_OPT_SMALL_PASS off and on (stand-alone; bench.py does not run it).

A syncer that replaces the reference's synchronous UpdateFunc gates flushes 1 to a few thousand events at a time,
so what it feels is the time from enqueue to results in hand, not the streaming rate.  Three populations
(kcp_amd.synth, seeded, 5% of the pairs mutated): Deployment pairs of config1's shape, ConfigMap / Secret pairs
(config2) and deep CRD pairs (config4), at 1, 16, 256 and 4096 pairs, through three paths, each a host clock around

  resident       gpudiff_diff -> gpudiff_wait on a DeviceBatch already in HBM
  submit_host    gpudiff_submit -> gpudiff_wait, encoded on the host
  submit_device  gpudiff_submit -> gpudiff_wait, encoded by K0 (GPUDIFF_OPT_DEVICE_ENCODE)

Two engines per path in one process, option off (the ordinary pass) and on, alternate rep by rep after a warm-up of
every shape; before timing, every cell's result arrays from the two engines must be equal.  The whole table is
measured --repeats times: per cell the line carries p50 / p99 over all samples and the spread (max - min) of the
per-repeat p50s.  One JSON line with build_id; needs a GPU and has no fallback.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

POPULATIONS = {"deployment": "config1", "configmap_secret": "config2", "deep_crd": "config4"}
PATHS = ("resident", "submit_host", "submit_device")
ARRAYS = ("pair_flags", "spec_dirty_ids", "status_dirty_ids", "dirty_ids", "path_offsets", "path_hashes", "path_kinds")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[1, 16, 256, 4096])
    ap.add_argument("--populations", type=lambda s: s.split(","), default=list(POPULATIONS))
    ap.add_argument("--paths", type=lambda s: s.split(","), default=list(PATHS))
    ap.add_argument("--reps", type=int, default=200, help="timed reps per cell and repeat, sizes up to 256")
    ap.add_argument("--reps-large", type=int, default=50, help="the same above 256 pairs")
    ap.add_argument("--repeats", type=int, default=5, help="measurements of the whole table")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args(argv)
    if not a.sizes or min(a.sizes) < 1:
        ap.error("--sizes: positive pair counts")
    for p in a.populations:
        if p not in POPULATIONS:
            ap.error("--populations: one of %s" % ", ".join(POPULATIONS))
    for p in a.paths:
        if p not in PATHS:
            ap.error("--paths: one of %s" % ", ".join(PATHS))
    if a.reps < 1 or a.reps_large < 1 or a.repeats < 1:
        ap.error("--reps / --reps-large / --repeats: at least 1")
    return a


def results_differ(a, b):
    """Name of the first result array in which two DiffResults differ, or None."""
    for name in ARRAYS:
        x, y = getattr(a, name), getattr(b, name)
        if x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(x, y):
            return name
    return None


def percentile(xs, q):
    s = sorted(xs)
    return s[min(len(s) - 1, int(q * len(s)))]


def summarise(samples_off, samples_on):
    """samples_*: one list of microseconds per repeat of the table."""
    def side(samples):
        flat = [x for r in samples for x in r]
        p50s = [statistics.median(r) for r in samples]
        return dict(p50_us=round(statistics.median(flat), 2), p99_us=round(percentile(flat, 0.99), 2),
                    p50_per_repeat_us=[round(x, 2) for x in p50s], p50_spread_us=round(max(p50s) - min(p50s), 2))
    off, on = side(samples_off), side(samples_on)
    return dict(off=off, on=on, p50_gain_us=round(off["p50_us"] - on["p50_us"], 2),
                gain_exceeds_off_spread=bool(off["p50_us"] - on["p50_us"] > off["p50_spread_us"]))


class Cell:
    """One (population, path, size): a closure per engine that runs the pass once and returns a DiffResult
    (check) or nothing (timed)."""

    def __init__(self, G, pop, path, n, eng, arr, threads):
        self.G, self.eng, self.path = G, eng, path
        lib = G.lib()
        self.res = G.Result()
        self.t = C.c_uint64()
        if path == "resident":
            ch = pop.chunk(eng, 0, n, threads)
            self.hb = ch.hb
            self.db = eng.device_batch(ch.pool_bytes + 4096, n)
            self.db.append(ch.hb)
            eng.sync()
            self.enqueue = lambda: lib.gpudiff_diff(eng.ctx, self.db.h, C.byref(self.t))
        else:
            sub = np.ascontiguousarray(arr[:n])
            self.sub = sub
            ptr = sub.ctypes.data_as(C.POINTER(G.JsonPair))
            self.enqueue = lambda: lib.gpudiff_submit(eng.ctx, ptr, n, C.byref(self.t))

    def result(self):
        self.G._chk(self.enqueue(), "enqueue")
        return self.eng.wait(self.t.value)

    def timed_us(self):
        lib, G = self.G.lib(), self.G
        t0 = time.perf_counter()
        rc = self.enqueue()
        rc2 = lib.gpudiff_wait(self.eng.ctx, self.t.value, C.byref(self.res)) if rc == 0 else 0
        t1 = time.perf_counter()
        G._chk(rc, "enqueue")
        G._chk(rc2, "gpudiff_wait")
        lib.gpudiff_result_release(self.eng.ctx, C.byref(self.res))
        return (t1 - t0) * 1e6

    def close(self):
        if self.path == "resident":
            self.db.free()
            self.hb.free()


def main(argv=None):
    a = parse_args(argv)
    from kcp_amd import gpudiff as G
    from kcp_amd import synth as S
    if G.device_count() < 1:
        sys.exit("bench_latency.py needs a GPU")
    n_max = max(a.sizes)
    engines = {}
    for dev in (False, True):
        base = G.OPT_DEVICE_ENCODE if dev else 0
        engines[dev] = {"off": G.Engine(device=0, encode_threads=a.threads, flags=base),
                        "on": G.Engine(device=0, encode_threads=a.threads, flags=base | G.OPT_SMALL_PASS)}
    cells = []  # (population, path, n, {"off": Cell, "on": Cell})
    keep = []
    for pname in a.populations:
        pop = S.Population(S.make_cfg(POPULATIONS[pname], n_pairs=n_max, n_clusters=max(1, n_max // 100)))
        buf, offs, _truth = pop.json_range(0, pop.n, a.threads)
        arr = G.json_pair_array(buf, offs)
        keep.append((pop, buf, arr))
        for path in a.paths:
            for n in a.sizes:
                engs = engines[path == "submit_device"]
                cells.append((pname, path, n, {m: Cell(G, pop, path, min(n, pop.n), engs[m], arr, a.threads)
                                               for m in ("off", "on")}))
    # every cell's results equal between the two engines, and every shape warm, before anything is timed
    for pname, path, n, c in cells:
        for _ in range(max(1, a.warmup)):
            bad = results_differ(c["off"].result(), c["on"].result())
            if bad:
                sys.exit("results differ (%s) for %s / %s / %d pairs" % (bad, pname, path, n))
    samples = {i: {"off": [], "on": []} for i in range(len(cells))}
    for _rep in range(a.repeats):
        for i, (pname, path, n, c) in enumerate(cells):
            reps = a.reps if n <= 256 else a.reps_large
            off, on = [], []
            for _ in range(reps):
                off.append(c["off"].timed_us())
                on.append(c["on"].timed_us())
            samples[i]["off"].append(off)
            samples[i]["on"].append(on)
        print("repeat %d of %d done" % (_rep + 1, a.repeats), file=sys.stderr, flush=True)
    table = []
    for i, (pname, path, n, c) in enumerate(cells):
        row = dict(population=pname, path=path, n_pairs=n, reps=a.reps if n <= 256 else a.reps_large)
        row.update(summarise(samples[i]["off"], samples[i]["on"]))
        table.append(row)
    stats = {("device_encode" if dev else "host_encode"): {m: e.pass_stats().as_dict() for m, e in engs.items()}
             for dev, engs in engines.items()}
    claim = {str(r["n_pairs"]): r["gain_exceeds_off_spread"] for r in table
             if r["population"] == "deployment" and r["path"] == "resident" and r["n_pairs"] in (1, 16)}
    line = dict(bench="latency", repeats=a.repeats, small_pass_max_pairs=G.SMALL_PASS_MAX_PAIRS,
                small_pass_max_paths=G.SMALL_PASS_MAX_PATHS, cells=table, pass_stats=stats,
                claim_resident_deployment_gain_exceeds_spread=claim, build_id=G.BUILD_ID)
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    for _p, _path, _n, c in cells:
        for cell in c.values():
            cell.close()
    for engs in engines.values():
        for e in engs.values():
            e.close()
    for pop, _b, _a in keep:
        pop.close()


if __name__ == "__main__":
    main()
