"""The host path inside gpudiff_wbatch_fetch: every document carries a duplicate key, so K10 defers all of them and
the fetch marshals each on the context's encode threads (go_marshal.cpp).  bench.py --config upsert has no deferred
document in its population, so its fetch_s does not show this cost.  Reported: fetch seconds (median, min, max) and
host bodies/s.

usage: python bench_host_bodies.py
"""
import ctypes as C
import json
import statistics
import sys
import time

from bench_upsert import add_owner_refs
from kcp_amd import gpudiff as G
from kcp_amd import synth as S

N, T, REPS = 32768, 16, 7
pop = S.Population(S.make_cfg("config3"), 1, 0)
buf, offs, _truth = pop.json_range(0, N, T)
docs = [add_owner_refs(bytes(buf[int(offs[2 * i + 1]):int(offs[2 * i + 2])]), i) for i in range(N)]
docs = [b'{"zz":1,"zz":2,' + d[1:] for d in docs]
L = G.lib()
eng = G.Engine(device=0, encode_threads=T)
wb = eng.wbatch(docs, G.UPSERT_SPEC)
ts, n_host, nbytes = [], 0, 0
for rep in range(REPS + 1):
    wb.run()
    b = G.Bodies()
    t0 = time.perf_counter()
    G._chk(L.gpudiff_wbatch_fetch(eng.ctx, wb.h, C.byref(b)), "gpudiff_wbatch_fetch")
    dt = time.perf_counter() - t0
    n_host = int(b.n_host)
    nbytes = int(C.cast(b.offsets, C.POINTER(C.c_uint64))[N])
    L.gpudiff_bodies_release(eng.ctx, C.byref(b))
    if rep:
        ts.append(dt)
wb.close()
eng.close()
print(json.dumps(dict(metric="gpudiff_wbatch_fetch with every document deferred to the host path", docs=N, threads=T,
                      host_docs=n_host, body_bytes=nbytes, fetch_s=dict(median=statistics.median(ts), min=min(ts), max=max(ts)),
                      host_bodies_per_s=n_host / statistics.median(ts), build_id=G.BUILD_ID)), flush=True)
sys.exit(0 if n_host == N else 1)
