#!/usr/bin/env python3
"""Update bodies per second, by two routes (stand-alone; bench.py does not run it).

Every steady-state write of the syncer sets the live object's resourceVersion on the body it sends
(pkg/syncer/statussyncer.go:50-57, specsyncer.go:116-124).  For the write-path benchmark's population
(bench_upsert.py: the config3 mix's new versions with kcp-shaped owner references), one JSON line with

  (a) splice   the engine's bodies -- one K10 launch over the resident batch, gpudiff_wbatch_fetch (the copy back
               and the host path for K10's deferrals), gpudiff_bodies_rv_splice -- then one
               gpudiff_splice_resource_version per body: two copies around the member
  (b) remarshal  what a caller without the descriptor does: gpudiff_update_body_host per document (decode,
               transform, SetResourceVersion, marshal)

both spread over --threads host threads (default 16; the calls release the GIL), each thread writing into one
reused buffer, every call through ctypes -- so both routes carry the same per-call binding cost, which bounds (a)
from above long before the copies do.  Reported: bodies/s of each route (median, min, max over --reps), the
ratio of the medians, the split of (a) into its engine part and its splice part, and a check that both routes
give the same bytes for every document.  one_thread_us_per_call is the cost of one call of each kind on a single
thread (best of three sweeps over the first 16,384 documents): without the threads' contention for the interpreter
lock it is the closer reading of what the two C functions cost.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from bench_upsert import add_owner_refs
from kcp_amd import gpudiff as G
from kcp_amd import synth as S

SPLICE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t, C.c_void_p,
                     C.c_size_t, C.POINTER(C.c_size_t))


def log(*a):
    print("[update-bodies]", *a, file=sys.stderr, flush=True)


def _shares(n, threads):
    return [(n * t // threads, n * (t + 1) // threads) for t in range(threads)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--rv", default="987654321")
    args = ap.parse_args()
    N, T, rv = args.docs, args.threads, args.rv.encode()
    pop = S.Population(S.make_cfg("config3"), 1, 0)
    buf, offs, _truth = pop.json_range(0, N, T)
    docs = [add_owner_refs(bytes(buf[int(offs[2 * i + 1]):int(offs[2 * i + 2])]), i) for i in range(N)]
    del buf
    log("%d documents, %.2f GB of JSON" % (N, sum(len(d) for d in docs) / 1e9))
    L = G.lib()
    splice = C.cast(L.gpudiff_splice_resource_version, SPLICE)
    cap = 4 * max(len(d) for d in docs) + 1024
    outs = [C.create_string_buffer(cap) for _ in range(T)]
    pool = ThreadPoolExecutor(T)
    eng = G.Engine(device=0, encode_threads=T)
    wb = eng.wbatch(docs, G.UPSERT_SPEC)

    def route_a(keep=None, single=0):
        """(seconds of the engine part, seconds of the splices); single: the first `single` bodies on one thread"""
        t0 = time.perf_counter()
        wb.run()
        b = G.Bodies()
        G._chk(L.gpudiff_wbatch_fetch(eng.ctx, wb.h, C.byref(b)), "gpudiff_wbatch_fetch")
        r = G.RvSpliceC()
        G._chk(L.gpudiff_bodies_rv_splice(eng.ctx, C.byref(b), C.byref(r)), "gpudiff_bodies_rv_splice")
        t1 = time.perf_counter()
        bo = np.ctypeslib.as_array(C.cast(b.offsets, C.POINTER(C.c_uint64)), (N + 1,)).tolist()
        ro = np.ctypeslib.as_array(C.cast(r.off, C.POINTER(C.c_uint32)), (N,)).tolist()
        rf = np.ctypeslib.as_array(C.cast(r.form, C.POINTER(C.c_uint8)), (N,)).tolist()
        base = b.bytes

        def work(t):
            out, n = outs[t], C.c_size_t()
            lo, hi = (0, single) if single else _shares(N, T)[t]
            for i in range(lo, hi):
                if splice(base + bo[i], bo[i + 1] - bo[i], ro[i], rf[i], rv, len(rv), out, cap, C.byref(n)):
                    raise RuntimeError("splice %d" % i)
                if keep is not None:
                    keep[i] = out.raw[:n.value]
        if single:
            t1 = time.perf_counter()
            work(0)
        else:
            list(pool.map(work, range(T)))
        t2 = time.perf_counter()
        stats = (int(r.n_device), int(r.n_host))
        L.gpudiff_bodies_release(eng.ctx, C.byref(b))
        return t1 - t0, t2 - t1, stats

    def route_b(keep=None, single=0):
        t0 = time.perf_counter()

        def work(t):
            out, n = outs[t], C.c_size_t()
            outp = C.cast(out, C.c_void_p)
            lo, hi = (0, single) if single else _shares(N, T)[t]
            for i in range(lo, hi):
                d = docs[i]
                if L.gpudiff_update_body_host(d, len(d), G.UPSERT_SPEC, rv, len(rv), outp, cap, C.byref(n)):
                    raise RuntimeError("update_body_host %d" % i)
                if keep is not None:
                    keep[i] = out.raw[:n.value]
        if single:
            work(0)
        else:
            list(pool.map(work, range(T)))
        return time.perf_counter() - t0

    # the warm-up round is the check: both routes give the same bytes for every document
    ka, kb = [None] * N, [None] * N
    _, _, (n_dev, n_host) = route_a(ka)
    route_b(kb)
    mism = sum(1 for x, y in zip(ka, kb) if x != y)
    del ka, kb
    log("device descriptors %d, host %d, mismatches %d" % (n_dev, n_host, mism))
    a_eng, a_spl, b_all = [], [], []
    for _ in range(args.reps):  # alternating
        e, s, _st = route_a()
        a_eng.append(e)
        a_spl.append(s)
        b_all.append(route_b())
    a_all = [e + s for e, s in zip(a_eng, a_spl)]
    # one thread, no contention for the interpreter lock: what one call of each kind costs through the binding
    n1 = min(N, 16384)
    us_splice = min(route_a(single=n1)[1] for _ in range(3)) / n1 * 1e6
    us_remarshal = min(route_b(single=n1) for _ in range(3)) / n1 * 1e6

    def rate(ts):
        return dict(median=N / statistics.median(ts), min=N / max(ts), max=N / min(ts))
    line = dict(metric="Update bodies/s: engine bodies + resourceVersion splice (a) vs per-document re-marshal (b)",
                docs=N, threads=T, reps=args.reps, rv=args.rv, device_descriptors=n_dev, host_descriptors=n_host,
                mismatches=mism, a_splice=rate(a_all), b_remarshal=rate(b_all),
                ratio_a_over_b=statistics.median(b_all) / statistics.median(a_all),
                a_engine_s=statistics.median(a_eng), a_splice_s=statistics.median(a_spl),
                b_s=statistics.median(b_all),
                one_thread_us_per_call=dict(docs=n1, splice=us_splice, remarshal=us_remarshal),
                build_id=G.BUILD_ID)
    wb.close()
    eng.close()
    print(json.dumps(line), flush=True)
    return 1 if mism else 0


if __name__ == "__main__":
    sys.exit(main())
