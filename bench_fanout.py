#!/usr/bin/env python3
"""What the per-cluster index of a pass's dirty IDs costs (gpudiff_cluster_index_get, kernels K23 - K25; stand-alone,
bench.py does not run it).

A config3-like resident population (kcp_amd.synth; default 1M pairs over 10k clusters, --pairs / --clusters scale it
up to 10M / 100k where the box allows) in two variants, one JSON line each:

  ordered    the batch as the generator lays it out, pairs in cluster order: the dirty list ascends by cluster and
             no sort runs (sorted_on_device == 0)
  permuted   the same pairs with the cluster ids relabelled by a random permutation, so the dirty list does not
             ascend: the radix sort runs

Per variant, after one warm-up pass + call, over --reps waited passes:

  get_ms          host clock around gpudiff_cluster_index_get + gpudiff_cluster_index_release, the stream drained
                  first: median, min and max
  kernel_ms       K23, the sort + K24 + scan, and K25 by HIP events (GPUDIFF_OPT_TIMING), per call
  host_ms         the same index by gpudiff_cluster_index_host on one core from the waited result's flags and the
                  batch's pair and cluster ids (the baseline, not the code under test)
  numpy_ms        the same index by numpy (argsort(kind="stable")) from the same arrays
  entries, d2h_bytes, syncs_per_call, sorted_on_device, n_listed (clusters in the index)

The device index is checked against the host routine's, array for array, before anything is timed."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

from kcp_amd import gpudiff as G
from kcp_amd import synth as S

ARRAYS = ("cluster_ids", "spec_off", "status_off", "spec_ids", "status_ids")


def _rows_view(hb):
    inf = hb.info()
    return np.ctypeslib.as_array((C.c_uint8 * (inf.n_pairs * 64)).from_address(inf.rows)).view(G.ROW_DTYPE)


def _numpy_index(flags, ids, clusters):
    pos = np.flatnonzero(flags & 3)
    pos = pos[np.argsort(clusters[pos], kind="stable")]
    key = clusters[pos]
    head = np.ones(pos.size, dtype=bool)
    head[1:] = key[1:] != key[:-1]
    f = flags[pos]
    s, t = (f & 1) != 0, (f & 2) != 0
    hs = np.flatnonzero(head)
    cs, ct = np.cumsum(s), np.cumsum(t)
    so = np.append(cs[hs] - s[hs], cs[-1] if pos.size else 0).astype(np.uint32)
    to = np.append(ct[hs] - t[hs], ct[-1] if pos.size else 0).astype(np.uint32)
    return key[hs], so, to, ids[pos[s]], ids[pos[t]]


def _stat(ms):
    return dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3))


def run(variant, a):
    eng = G.Engine(device=0, encode_threads=a.threads, timing=True)
    cfg = S.make_cfg("config3", n_pairs=a.pairs, n_clusters=a.clusters)
    pop = S.Population(cfg)
    rng = np.random.default_rng(20211004)
    relabel = rng.permutation(max(a.clusters, 1)).astype(np.uint32)  # one relabelling: a cluster stays one cluster
    ids, clusters = np.zeros(pop.n, np.uint32), np.zeros(pop.n, np.uint32)
    db, stage, pos, k = None, [None, None], 0, 0
    while pos < pop.n:  # two pinned staging batches in turn, as bench.py ingests
        m = min(a.chunk, pop.n - pos)
        ch = pop.chunk(eng, pos, m, a.threads, reuse=stage[k & 1])
        stage[k & 1] = ch.hb
        rows = _rows_view(ch.hb)
        if variant == "permuted":
            rows["cluster_id"] = relabel[rows["cluster_id"] % relabel.size]
        ids[pos:pos + m], clusters[pos:pos + m] = rows["pair_id"], rows["cluster_id"]
        if db is None:  # sized from the first chunk's bytes per pair
            db = eng.device_batch(int(ch.pool_bytes / m * pop.n * 1.15) + (64 << 20), pop.n)
        db.append(ch.hb)
        pos += m
        k += 1
    eng.sync()
    for hb in stage:
        if hb is not None:
            hb.free()
    lib = G.lib()

    def timed_get(ticket):
        ci = G.ClusterIndexC()
        eng.sync()
        t0 = time.perf_counter()
        G._chk(lib.gpudiff_cluster_index_get(eng.ctx, ticket, C.byref(ci)), "gpudiff_cluster_index_get")
        srt = int(ci.sorted_on_device)
        lib.gpudiff_cluster_index_release(eng.ctx, C.byref(ci))
        return (time.perf_counter() - t0) * 1e3, srt

    # warm-up, and the check: the device's index is the host routine's
    t = eng.diff(db)
    res = eng.wait(t)
    flags = res.pair_flags
    dev, host = eng.cluster_index(t), G.cluster_index_host(flags, ids, clusters)
    for k in ARRAYS:
        if not np.array_equal(getattr(dev, k), getattr(host, k)):
            sys.exit("bench_fanout: the device index differs from the host routine's in %s (%s)" % (k, variant))
    npi = _numpy_index(flags, ids, clusters)
    for k, x in zip(ARRAYS, npi):
        if not np.array_equal(getattr(host, k), x):
            sys.exit("bench_fanout: the numpy index differs from the host routine's in %s (%s)" % (k, variant))
    st0 = eng.cluster_index_stats().as_dict()
    get_ms, host_ms, numpy_ms, sorted_flags = [], [], [], []
    for _ in range(a.reps):
        t = eng.diff(db)
        res = eng.wait(t)
        ms, srt = timed_get(t)
        get_ms.append(ms)
        sorted_flags.append(srt)
        ci = G.ClusterIndexC()
        t0 = time.perf_counter()
        G._chk(lib.gpudiff_cluster_index_host(res.pair_flags.ctypes.data, ids.ctypes.data, clusters.ctypes.data,
                                              ids.size, C.byref(ci)), "gpudiff_cluster_index_host")
        lib.gpudiff_cluster_index_release(None, C.byref(ci))
        host_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        _numpy_index(res.pair_flags, ids, clusters)
        numpy_ms.append((time.perf_counter() - t0) * 1e3)
    st1 = eng.cluster_index_stats().as_dict()
    calls = st1["calls"] - st0["calls"]
    line = dict(variant=variant, n_pairs=int(pop.n), n_clusters=int(a.clusters), n_dirty=int(res.dirty_ids.size),
                n_spec=int(res.spec_dirty_ids.size), n_status=int(res.status_dirty_ids.size),
                n_listed=int(dev.cluster_ids.size), reps=a.reps, build_id=G.BUILD_ID,
                sorted_on_device=sorted(set(sorted_flags)), get_ms=_stat(get_ms),
                kernel_ms=round((st1["kernel_ms"] - st0["kernel_ms"]) /
                                max(st1["timed_calls"] - st0["timed_calls"], 1), 4),
                host_ms=_stat(host_ms), numpy_ms=_stat(numpy_ms),
                entries=int((st1["entries"] - st0["entries"]) // calls),
                d2h_bytes=int((st1["d2h_bytes"] - st0["d2h_bytes"]) // calls),
                syncs_per_call=round((st1["syncs"] - st0["syncs"]) / calls, 2))
    # what is required of the numbers: the generator's layout takes the fast path, and no call spends more than three
    # synchronisations
    if variant == "ordered" and line["sorted_on_device"] != [0]:
        sys.exit("bench_fanout: the cluster-ordered variant sorted: %s" % json.dumps(line))
    if line["syncs_per_call"] > 3:
        sys.exit("bench_fanout: more than three synchronisations a call: %s" % json.dumps(line))
    print(json.dumps(line), flush=True)
    db.free()
    pop.close()
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--clusters", type=int, default=10_000)
    ap.add_argument("--chunk", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--variants", default="ordered,permuted")
    a = ap.parse_args()
    if G.device_count() < 1:
        sys.exit("bench_fanout.py needs a GPU")
    for v in a.variants.split(","):
        run(v, a)


if __name__ == "__main__":
    main()
