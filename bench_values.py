#!/usr/bin/env python3
"""What GPUDIFF_OPT_PATH_VALUES costs next to GPUDIFF_OPT_PATH_STRINGS (stand-alone; bench.py does not run it).

Two populations (kcp_amd.synth): a config3-like batch and a config4-like batch of deep pairs, each through
device-encoded submit / wait on three engines -- strings only (what the engine could say before), values only, both
-- alternating rep by rep after a warm-up round, on one GPU.  Per population one JSON line; per engine:

  wait_ms            host clock around gpudiff_wait + gpudiff_result_release, the stream drained first
                     (gpudiff_sync), so it is the readback and the finisher alone: median, min and max over --reps
  strings_kernel_ms  K15 + scan + K16 by HIP events (gpudiff_path_strings_stats_get), per batch
  values_kernel_ms   K21 + scan and offsets + K22 by HIP events (gpudiff_path_values_stats_get), per batch
  value_bytes, values_per_s   the texts' bytes, and texts (two per changed path) per second of values_kernel_ms
  n_host             entries of pairs the host resolved (K0's deferrals), per batch
  syncs_per_wait     stream synchronisations the finisher spent on rendering (gpudiff_render_syncs_get): two for one
                     renderer and two for both -- the sizing read-back is shared
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

from kcp_amd import gpudiff as G
from kcp_amd import synth as S

ENGINES = (("strings", G.OPT_PATH_STRINGS), ("values", G.OPT_PATH_VALUES),
           ("both", G.OPT_PATH_STRINGS | G.OPT_PATH_VALUES))


def _wait_ms(eng, ticket):
    """(ms of wait + release, n_paths, value bytes or None)"""
    eng.sync()
    r = G.Result()
    t0 = time.perf_counter()
    G._chk(G.lib().gpudiff_wait(eng.ctx, ticket, C.byref(r)), "gpudiff_wait")
    pv = G.PathValuesC()
    rc = G.lib().gpudiff_result_path_values(eng.ctx, C.byref(r), C.byref(pv))
    n_paths = int(r.n_paths)
    nbytes = None
    if rc == G.OK:
        nbytes = int(np.ctypeslib.as_array(C.cast(pv.offsets, C.POINTER(C.c_uint64)), (2 * n_paths + 1,))[-1])
        if pv.n_unresolved:
            raise RuntimeError("%d unresolved values" % pv.n_unresolved)
    G.lib().gpudiff_result_release(eng.ctx, C.byref(r))
    return (time.perf_counter() - t0) * 1e3, n_paths, nbytes


def _counters(eng, flags):
    ps = eng.path_stats() if flags & G.OPT_PATH_STRINGS else None
    vs = eng.path_values_stats()
    return dict(pk=ps.kernel_ms if ps else 0.0, vk=vs.kernel_ms, vt=vs.timed_batches, vh=vs.host_paths,
                syncs=eng.render_syncs())


def run(name, n_pairs, reps, threads):
    cfg = S.make_cfg(name, n_pairs=n_pairs, n_clusters=max(1, n_pairs // 100))
    pop = S.Population(cfg)
    buf, offs, _truth = pop.json_range(0, pop.n, threads)
    arr = G.json_pair_array(buf, offs)
    base = G.OPT_DEVICE_ENCODE | G.OPT_TIMING
    engs = {k: G.Engine(device=0, encode_threads=threads, flags=base | f) for k, f in ENGINES}
    ms = {k: [] for k, _f in ENGINES}
    c0 = {}
    n_paths = nbytes = 0
    for rep in range(reps + 1):  # the first round warms every engine (buffers grow, code objects load)
        for k, f in ENGINES:
            if rep == 1:
                c0[k] = _counters(engs[k], f)
            t, n_paths, nb = _wait_ms(engs[k], engs[k].submit_array(arr))
            if rep:
                ms[k].append(t)
            if nb is not None:
                nbytes = nb
    line = dict(population=name, n_pairs=int(pop.n), json_bytes=int(offs[-1]), n_paths=n_paths, value_bytes=nbytes,
                reps=reps, build_id=G.BUILD_ID)
    for k, f in ENGINES:
        c1 = _counters(engs[k], f)
        vk = (c1["vk"] - c0[k]["vk"]) / reps
        line[k] = dict(wait_ms=round(statistics.median(ms[k]), 3), wait_ms_min=round(min(ms[k]), 3),
                       wait_ms_max=round(max(ms[k]), 3), strings_kernel_ms=round((c1["pk"] - c0[k]["pk"]) / reps, 4),
                       values_kernel_ms=round(vk, 4),
                       values_per_s=round(2 * n_paths / (vk * 1e-3)) if vk > 0 else None,
                       n_host=int((c1["vh"] - c0[k]["vh"]) // reps),
                       syncs_per_wait=round((c1["syncs"] - c0[k]["syncs"]) / reps, 2))
    print(json.dumps(line), flush=True)
    for e in engs.values():
        e.close()
    pop.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config3-pairs", type=int, default=200_000)
    ap.add_argument("--config4-pairs", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    if G.device_count() < 1:
        sys.exit("bench_values.py needs a GPU")
    if a.config3_pairs:
        run("config3", a.config3_pairs, a.reps, a.threads)
    if a.config4_pairs:
        run("config4", a.config4_pairs, a.reps, a.threads)


if __name__ == "__main__":
    main()
