#!/usr/bin/env python3
"""The request target (namespace, name) per write, by two routes (stand-alone; bench.py does not run it).

Controller.process needs meta.GetNamespace() and meta.GetName() for every write (pkg/syncer/syncer.go:310).  For the
write-path benchmark's population (bench_upsert.py: the config3 mix's new versions with kcp-shaped owner references),
one JSON line with

  (a) descriptor  the engine's bodies -- one K10 launch over the resident batch, gpudiff_wbatch_fetch,
                  gpudiff_bodies_targets -- then per write the two spans of the body: a slice where the span renders
                  clean, gpudiff_target_decode where the encoder escaped something (a_always_decode: two
                  gpudiff_target_decode calls per write whatever the flags say)
  (b) decode      what a consumer without the descriptor does: gpudiff_target_host per document (a full decode)

Reported: one_thread_us_per_write -- each route's per-write cost on a single thread over the first 16,384 documents,
every call through ctypes (best of three sweeps), the engine part of (a) left out, since the bodies are rendered
for the write anyway; writes_per_s -- the whole batch by both routes (median, min, max over --reps), (a) including
the K10 launch, the copy back and the descriptor fetch, the per-write part spread over --threads host threads.  The
warm-up round is the check: both routes give the same strings for every document.
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


# the body's address instead of a bytes object: the spans are decoded where gpudiff_wbatch_fetch left the bodies
DECODE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                     C.POINTER(C.c_size_t))


def log(*a):
    print("[targets]", *a, file=sys.stderr, flush=True)


def _shares(n, threads):
    return [(n * t // threads, n * (t + 1) // threads) for t in range(threads)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    N, T = args.docs, args.threads
    pop = S.Population(S.make_cfg("config3"), 1, 0)
    buf, offs, _truth = pop.json_range(0, N, T)
    docs = [add_owner_refs(bytes(buf[int(offs[2 * i + 1]):int(offs[2 * i + 2])]), i) for i in range(N)]
    del buf
    log("%d documents, %.2f GB of JSON" % (N, sum(len(d) for d in docs) / 1e9))
    L = G.lib()
    decode = C.cast(L.gpudiff_target_decode, DECODE)
    pool = ThreadPoolExecutor(T)
    eng = G.Engine(device=0, encode_threads=T)
    wb = eng.wbatch(docs, G.UPSERT_SPEC)
    cap = 1024

    def route_a(keep=None, single=0, always=False):
        """(seconds of the engine part, seconds of the per-write part, (n_device, n_host))"""
        t0 = time.perf_counter()
        wb.run()
        b = G.Bodies()
        G._chk(L.gpudiff_wbatch_fetch(eng.ctx, wb.h, C.byref(b)), "gpudiff_wbatch_fetch")
        r = G.TargetsC()
        G._chk(L.gpudiff_bodies_targets(eng.ctx, C.byref(b), C.byref(r)), "gpudiff_bodies_targets")
        t1 = time.perf_counter()
        bo = np.ctypeslib.as_array(C.cast(b.offsets, C.POINTER(C.c_uint64)), (N + 1,)).tolist()
        to = np.ctypeslib.as_array(C.cast(r.off, C.POINTER(C.c_uint32)), (2 * N,)).tolist()
        tl = np.ctypeslib.as_array(C.cast(r.len, C.POINTER(C.c_uint32)), (2 * N,)).tolist()
        tf = np.ctypeslib.as_array(C.cast(r.flags, C.POINTER(C.c_uint8)), (N,)).tolist()
        raw = C.string_at(b.bytes, bo[N])
        base = b.bytes

        def work(t):
            out, n = C.create_string_buffer(cap), C.c_size_t()
            outp = C.cast(out, C.c_void_p)
            lo, hi = (0, single) if single else _shares(N, T)[t]
            for i in range(lo, hi):
                pair = []
                for k, esc in ((1, G.TGT_NS_ESC), (0, G.TGT_NAME_ESC)):
                    o, ln = to[2 * i + k], tl[2 * i + k]
                    if always or tf[i] & esc:
                        if decode(base + bo[i], bo[i + 1] - bo[i], o, ln, outp, cap, C.byref(n)):
                            raise RuntimeError("target_decode %d" % i)
                        pair.append(out.raw[:n.value])
                    else:
                        pair.append(raw[bo[i] + o:bo[i] + o + ln])
                if keep is not None:
                    keep[i] = tuple(pair)
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
            name, ns = C.create_string_buffer(cap), C.create_string_buffer(cap)
            namep, nsp = C.cast(name, C.c_void_p), C.cast(ns, C.c_void_p)
            nn, sn = C.c_size_t(), C.c_size_t()
            lo, hi = (0, single) if single else _shares(N, T)[t]
            for i in range(lo, hi):
                d = docs[i]
                if L.gpudiff_target_host(d, len(d), namep, cap, C.byref(nn), nsp, cap, C.byref(sn)):
                    raise RuntimeError("target_host %d" % i)
                pair = (ns.raw[:sn.value], name.raw[:nn.value])
                if keep is not None:
                    keep[i] = pair
        if single:
            work(0)
        else:
            list(pool.map(work, range(T)))
        return time.perf_counter() - t0

    # the warm-up round is the check: both routes give the same strings for every document
    ka, kc, kb = [None] * N, [None] * N, [None] * N
    _, _, (n_dev, n_host) = route_a(ka)
    route_a(kc, always=True)
    route_b(kb)
    mism = sum(1 for x, y, z in zip(ka, kb, kc) if x != y or z != y)
    named = sum(1 for x in kb if x[1])
    spaced = sum(1 for x in kb if x[0])
    del ka, kb, kc
    log("device descriptors %d, host %d, mismatches %d, with a name %d, with a namespace %d"
        % (n_dev, n_host, mism, named, spaced))
    a_eng, a_per, b_all = [], [], []
    for _ in range(args.reps):  # alternating
        e, s, _st = route_a()
        a_eng.append(e)
        a_per.append(s)
        b_all.append(route_b())
    a_all = [e + s for e, s in zip(a_eng, a_per)]
    n1 = min(N, 16384)
    us_desc = min(route_a(single=n1)[1] for _ in range(3)) / n1 * 1e6
    us_always = min(route_a(single=n1, always=True)[1] for _ in range(3)) / n1 * 1e6
    us_host = min(route_b(single=n1) for _ in range(3)) / n1 * 1e6

    def rate(ts):
        return dict(median=N / statistics.median(ts), min=N / max(ts), max=N / min(ts))
    line = dict(metric="(namespace, name) per write: descriptor + gpudiff_target_decode (a) vs gpudiff_target_host (b)",
                docs=N, threads=T, reps=args.reps, device_descriptors=n_dev, host_descriptors=n_host,
                mismatches=mism, with_name=named, with_namespace=spaced,
                one_thread_us_per_write=dict(docs=n1, a_descriptor=us_desc, a_always_decode=us_always,
                                             b_target_host=us_host),
                writes_per_s=dict(a_descriptor=rate(a_all), b_target_host=rate(b_all)),
                ratio_a_over_b=statistics.median(b_all) / statistics.median(a_all),
                a_engine_s=statistics.median(a_eng), a_per_write_s=statistics.median(a_per),
                b_s=statistics.median(b_all), build_id=G.BUILD_ID)
    wb.close()
    eng.close()
    print(json.dumps(line), flush=True)
    return 1 if mism else 0


if __name__ == "__main__":
    sys.exit(main())
