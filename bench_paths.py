#!/usr/bin/env python3
"""What GPUDIFF_OPT_PATH_STRINGS costs, and what it replaces (stand-alone; bench.py does not run it).

Two populations (kcp_amd.synth): a config3-like batch and a config4-like batch of deep pairs, each through
device-encoded submit / wait with the option off and on, alternating, on one GPU.  Per population one JSON line:

  wait_ms_off / wait_ms_on   host clock around gpudiff_wait + gpudiff_result_release, the stream drained first
                             (gpudiff_sync), so it is the readback and the finisher alone: median over --reps
  added_wait_ms              their difference: what the option adds to wait
  kernel_ms, paths_per_s     K15 + scan + K16 by HIP events (gpudiff_path_strings_stats_get), per batch
  resolve_us_per_path        the host helper the strings replace: gpudiff_resolve_path over a sample of the same
                             batch's (hash, kind) entries, each call decoding both documents again
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


def _wait_ms(eng, ticket):
    """(ms of wait + release, n_paths, string bytes or None)"""
    eng.sync()
    r = G.Result()
    t0 = time.perf_counter()
    G._chk(G.lib().gpudiff_wait(eng.ctx, ticket, C.byref(r)), "gpudiff_wait")
    ps = G.PathStringsC()
    rc = G.lib().gpudiff_result_path_strings(eng.ctx, C.byref(r), C.byref(ps))
    n_paths = int(r.n_paths)
    nbytes = None
    if rc == G.OK:
        nbytes = int(np.ctypeslib.as_array(C.cast(ps.offsets, C.POINTER(C.c_uint64)), (n_paths + 1,))[-1])
        if ps.n_unresolved:
            raise RuntimeError("%d unresolved paths" % ps.n_unresolved)
    G.lib().gpudiff_result_release(eng.ctx, C.byref(r))
    return (time.perf_counter() - t0) * 1e3, n_paths, nbytes


def _sample(eng, arr, k):
    """Up to k (pair index, hash, kind) entries of the batch, spread over its dirty pairs."""
    res = eng.wait(eng.submit_array(arr))
    dirty = np.nonzero(res.pair_flags & (G.SPEC_DIRTY | G.STATUS_DIRTY))[0]
    out = []
    step = max(1, len(res.path_hashes) // k)
    for kd in range(len(dirty)):
        b, e = int(res.path_offsets[kd]), int(res.path_offsets[kd + 1])
        for q in range(b + (-b % step), e, step):
            out.append((int(dirty[kd]), int(res.path_hashes[q]), int(res.path_kinds[q])))
    return out[:k]


def run(name, n_pairs, reps, sample, threads):
    cfg = S.make_cfg(name, n_pairs=n_pairs, n_clusters=max(1, n_pairs // 100))
    pop = S.Population(cfg)
    buf, offs, _truth = pop.json_range(0, pop.n, threads)
    arr = G.json_pair_array(buf, offs)
    base = G.OPT_DEVICE_ENCODE | G.OPT_TIMING
    engs = {"off": G.Engine(device=0, encode_threads=threads, flags=base),
            "on": G.Engine(device=0, encode_threads=threads, flags=base | G.OPT_PATH_STRINGS)}
    ms = {"off": [], "on": []}
    n_paths = nbytes = 0
    for rep in range(reps + 1):  # the first round warms both engines (buffers grow, code objects load)
        for mode, eng in engs.items():
            if rep == 1 and mode == "on":
                k0 = eng.path_stats()
                k0 = (k0.kernel_ms, k0.timed_batches, k0.host_paths)
            t, n_paths, nb = _wait_ms(eng, eng.submit_array(arr))
            if rep:
                ms[mode].append(t)
            if nb is not None:
                nbytes = nb
    st = engs["on"].path_stats()
    kernel_ms = (st.kernel_ms - k0[0]) / max(1, st.timed_batches - k0[1])
    host_paths = (st.host_paths - k0[2]) // max(1, st.timed_batches - k0[1])
    smp = _sample(engs["off"], arr, sample)
    out = C.create_string_buffer(1 << 16)
    olen = C.c_size_t()
    t0 = time.perf_counter()
    for i, h, kd in smp:
        p = arr[i]
        rc = G.lib().gpudiff_resolve_path(C.c_char_p(int(p["old_json"])), int(p["old_len"]),
                                          C.c_char_p(int(p["new_json"])), int(p["new_len"]), h, kd,
                                          G.PATH_HASH_BITS, out, len(out), C.byref(olen))
        if rc != G.OK:
            raise RuntimeError("gpudiff_resolve_path: %d" % rc)
    resolve_us = (time.perf_counter() - t0) * 1e6 / max(1, len(smp))
    off, on = statistics.median(ms["off"]), statistics.median(ms["on"])
    line = dict(population=name, n_pairs=int(pop.n), json_bytes=int(offs[-1]), n_paths=n_paths, string_bytes=nbytes,
                host_paths=int(host_paths), reps=reps, wait_ms_off=round(off, 3), wait_ms_on=round(on, 3),
                wait_ms_off_all=[round(x, 3) for x in ms["off"]], wait_ms_on_all=[round(x, 3) for x in ms["on"]],
                added_wait_ms=round(on - off, 3), kernel_ms=round(kernel_ms, 4),
                paths_per_s=round(n_paths / (kernel_ms * 1e-3)) if kernel_ms > 0 else None,
                resolve_sample=len(smp), resolve_us_per_path=round(resolve_us, 2), build_id=G.BUILD_ID)
    print(json.dumps(line), flush=True)
    for e in engs.values():
        e.close()
    pop.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config3-pairs", type=int, default=200_000)
    ap.add_argument("--config4-pairs", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    if G.device_count() < 1:
        sys.exit("bench_paths.py needs a GPU")
    if a.config3_pairs:
        run("config3", a.config3_pairs, a.reps, a.sample, a.threads)
    if a.config4_pairs:
        run("config4", a.config4_pairs, a.reps, a.sample, a.threads)


if __name__ == "__main__":
    main()
