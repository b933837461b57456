#!/usr/bin/env python3
"""What the cluster index under a batch's final flags costs (gpudiff_cluster_index_get_final: kernels K26 - K28 in
front of K23 - K25; stand-alone, bench.py does not run it), for the batches gpudiff_cluster_index_get refuses.

Two workloads of config3-like objects (kcp_amd.synth), one JSON line each.  About --escaped (1 %) of the objects get
an escaped key (`"k\\u0065y"`) spliced into both versions: K0 defers those events, the device lists them dirty in both
kinds, and the host resolves them to their true flags -- most of them clean, so the call patches and compacts.

  store    a device-encode object store: --batch (65,536, config 5's batch) objects listed, then one batch that
           updates every one of them; that batch's ticket is indexed
  submit   one device-encoded gpudiff_submit of --pairs pairs

Per workload, after the waited batch and one warm-up call, over --reps calls on the waited ticket:

  get_ms     host clock around gpudiff_cluster_index_get_final + gpudiff_cluster_index_release: median, min and max
  kernel_ms  K26 + K27 + scan, K28, K23, the sort + K24 + scan, and K25 by HIP events (GPUDIFF_OPT_TIMING), per call
  host_ms    the baseline, what a consumer does today: gpudiff_cluster_index_host on one core over the waited result's
             flags and the batch's pair and cluster ids
  entries_in / entries_live / patch_rows / h2d_bytes / d2h_bytes per call, syncs_per_call, n_listed, deferred

The device index is checked against the baseline's, array for array, before anything is timed."""
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
TAIL = b',"k\\u0065y":"v"}'


def _stat(ms):
    return dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3))


def documents(n, clusters, threads, frac):
    """-> old objects, new objects (bytes), cluster ids, how many got the escaped key"""
    pop = S.Population(S.make_cfg("config3", n_pairs=n, n_clusters=clusters))
    buf, offs, _ = pop.json_range(0, pop.n, threads)
    raw, o = buf.tobytes(), offs.astype(np.int64)
    esc = np.random.default_rng(20211004).random(pop.n) < frac
    a, b = [], []
    for i in range(pop.n):
        x, y = raw[o[2 * i]:o[2 * i + 1]], raw[o[2 * i + 1]:o[2 * i + 2]]
        if esc[i]:
            x, y = x[:-1] + TAIL, y[:-1] + TAIL
        a.append(x)
        b.append(y)
    cl = (np.arange(pop.n, dtype=np.uint32) % np.uint32(max(clusters, 1))).astype(np.uint32)
    pop.close()
    return a, b, cl, int(esc.sum())


def measure(eng, ticket, res, ids, clusters, reps, line):
    lib = G.lib()
    dev, host = eng.cluster_index_final(ticket), G.cluster_index_host(res.pair_flags, ids, clusters)  # the warm-up
    for k in ARRAYS:
        if not np.array_equal(getattr(dev, k), getattr(host, k)):
            sys.exit("bench_fanout_final: the device index differs from the host routine's in %s (%s)" % (
                k, line["workload"]))
    st0 = eng.cluster_index_final_stats().as_dict()
    get_ms, host_ms = [], []
    for _ in range(reps):
        ci = G.ClusterIndexC()
        eng.sync()
        t0 = time.perf_counter()
        G._chk(lib.gpudiff_cluster_index_get_final(eng.ctx, ticket, C.byref(ci)), "gpudiff_cluster_index_get_final")
        lib.gpudiff_cluster_index_release(eng.ctx, C.byref(ci))
        get_ms.append((time.perf_counter() - t0) * 1e3)
        ci = G.ClusterIndexC()
        t0 = time.perf_counter()
        G._chk(lib.gpudiff_cluster_index_host(res.pair_flags.ctypes.data, ids.ctypes.data, clusters.ctypes.data,
                                              ids.size, C.byref(ci)), "gpudiff_cluster_index_host")
        lib.gpudiff_cluster_index_release(None, C.byref(ci))
        host_ms.append((time.perf_counter() - t0) * 1e3)
    st1 = eng.cluster_index_final_stats().as_dict()
    calls = st1["calls"] - st0["calls"]
    per = lambda k: int((st1[k] - st0[k]) // calls)
    line.update(n_pairs=int(ids.size), n_dirty=int(res.dirty_ids.size), n_spec=int(res.spec_dirty_ids.size),
                n_status=int(res.status_dirty_ids.size), n_listed=int(dev.cluster_ids.size), reps=reps,
                build_id=G.BUILD_ID, sorted_on_device=int(dev.sorted_on_device), get_ms=_stat(get_ms),
                kernel_ms=round((st1["kernel_ms"] - st0["kernel_ms"]) / max(st1["timed_calls"] - st0["timed_calls"], 1),
                                4),
                host_ms=_stat(host_ms), entries_in=per("entries_in"), entries_live=per("entries_live"),
                patch_rows=per("patch_rows"), h2d_bytes=per("h2d_bytes"), d2h_bytes=per("d2h_bytes"),
                patched_calls=st1["patched_calls"] - st0["patched_calls"],
                compacted_calls=st1["compacted_calls"] - st0["compacted_calls"],
                syncs_per_call=round((st1["syncs"] - st0["syncs"]) / calls, 2))
    if line["syncs_per_call"] > 4:
        sys.exit("bench_fanout_final: more than four synchronisations a call: %s" % json.dumps(line))
    print(json.dumps(line), flush=True)


def run_store(a):
    old, new, cl, n_esc = documents(a.batch, a.clusters, a.threads, a.escaped)
    n = len(new)
    eng = G.Engine(device=0, encode_threads=a.threads, timing=True)
    per_obj = sum(len(x) for x in new) / n * 2.2 + 256
    st = eng.object_store(n, int(per_obj * n * 4) + (256 << 20), n, device_encode=True)
    ids = (np.arange(n, dtype=np.uint32) * 2 + 1).astype(np.uint32)
    eng.wait(st.submit([(i, old[i], None, int(ids[i]), int(cl[i])) for i in range(n)]))  # the initial list
    d0 = st.stats().deferred
    t = st.submit([(i, new[i], old[i], int(ids[i]), int(cl[i])) for i in range(n)])
    res = eng.wait(t)
    measure(eng, t, res, ids, cl, a.reps, dict(workload="store", n_clusters=int(a.clusters), escaped=n_esc,
                                               deferred=int(st.stats().deferred - d0)))
    st.free()
    eng.close()


def run_submit(a):
    old, new, cl, n_esc = documents(a.pairs, a.clusters, a.threads, a.escaped)
    n = len(new)
    eng = G.Engine(device=0, encode_threads=a.threads, timing=True, device_encode=True)
    ids = (np.arange(n, dtype=np.uint32) * 2 + 1).astype(np.uint32)
    t = eng.submit(list(zip(old, new)), ids.tolist(), cl.tolist())
    res = eng.wait(t)
    measure(eng, t, res, ids, cl, a.reps, dict(workload="submit", n_clusters=int(a.clusters), escaped=n_esc,
                                               deferred=int(eng.submit_stats().deferred)))
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=65536, help="store: events of the indexed batch")
    ap.add_argument("--pairs", type=int, default=262144, help="submit: pairs of the indexed batch")
    ap.add_argument("--clusters", type=int, default=1000)
    ap.add_argument("--escaped", type=float, default=0.01, help="share of objects with an escaped key")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--workloads", default="store,submit")
    a = ap.parse_args()
    if G.device_count() < 1:
        sys.exit("bench_fanout_final.py needs a GPU")
    for w in a.workloads.split(","):
        {"store": run_store, "submit": run_submit}[w](a)


if __name__ == "__main__":
    main()
