#!/usr/bin/env python3
"""What the write plan of a watch-replay batch costs, and what it replaces (stand-alone; bench.py does not run it).

One config5-like batch on a device-encode store: --events objects (kcp_amd.synth, config3 mix) are made resident
(version A, untimed), then ONE batch advances every object to version B (5% of them mutated) and is waited.  Then,
--reps times after a warm-up, on that waited ticket:

  plan_ms            host clock around gpudiff_store_write_plan_get + gpudiff_write_plan_release
  fold_ms/k10_ms/pack_ms   HIP events inside it (gpudiff_store_plan_stats_get): final flags + K17 + scans + K18; K10,
                     both kinds; the lengths' scan + K19
  d2h_bytes, h2d_bytes, body_bytes, arena_bytes   the call's counters: what crossed the link, what stayed in HBM
  upsert_ms          the same bodies the way a replay user gets them without the plan: gpudiff_upsert_bodies over
                     the dirty last versions, re-uploaded from host memory (one call per kind), + release
  upsert_h2d_bytes   the JSON those calls upload again

Medians with min / max over the repetitions, one JSON line, with the library's build_id.
"""
import argparse
import ctypes as C
import json
import statistics
import time

import numpy as np

from bench_replay import EVENT_DTYPE
from kcp_amd import gpudiff as G
from kcp_amd import synth as S


def _spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    M = args.events
    cfg = S.make_cfg("config3", n_pairs=M, n_clusters=max(1, M // 100))
    pop = S.Population(cfg)
    buf, offs, _truth = pop.json_range(0, M, args.threads)
    starts = offs[:-1].astype(np.uint64) + np.uint64(buf.ctypes.data)
    lens = np.diff(offs).astype(np.uint64)
    a_ptr, b_ptr, a_len, b_len = starts[0::2], starts[1::2], lens[0::2], lens[1::2]

    eng = G.Engine(device=0, encode_threads=args.threads, timing=True)
    per_obj = float(lens.mean()) * 2.2 + 256
    st = eng.object_store(M, int(per_obj * M * 4) + (256 << 20), M, device_encode=True)

    def submit(new_ptr, new_len, old_ptr=None, old_len=None):
        ev = np.zeros(M, dtype=EVENT_DTYPE)
        ev["slot"] = ev["pair_id"] = np.arange(M, dtype=np.uint32)
        ev["new_json"], ev["new_len"] = new_ptr, new_len
        if old_ptr is not None:
            ev["old_json"], ev["old_len"] = old_ptr, old_len
        return st.submit_raw((G.Event * M).from_buffer(ev), M, ev)

    eng.wait(submit(a_ptr, a_len))                       # the initial list
    ticket = submit(b_ptr, b_len, a_ptr, a_len)          # the replay batch: every object A -> B
    res = eng.wait(ticket)
    lib = G.lib()

    def plan_once():
        wp = G.WritePlanC()
        t0 = time.perf_counter()
        G._chk(lib.gpudiff_store_write_plan_get(eng.ctx, st.h, ticket, G.PLAN_INFORMER, C.byref(wp)), "plan")
        n = int(wp.n)
        idx = G._arr(wp.pair_index, n, np.uint32)
        kind = G._arr(wp.kind, n, np.uint8)
        noop = G._arr(wp.noop, n, np.uint8)
        total = int(np.ctypeslib.as_array(C.cast(wp.bodies.offsets, C.POINTER(C.c_uint64)), (n + 1,))[-1])
        lib.gpudiff_write_plan_release(eng.ctx, C.byref(wp))
        return (time.perf_counter() - t0) * 1e3, idx, kind, noop, total

    def upsert_once(idx, kind, noop):
        """gpudiff_upsert_bodies over the plan's non-no-op last versions, from host memory; (ms, bytes uploaded)."""
        ms, up = 0.0, 0
        for mode in (G.UPSERT_SPEC, G.UPSERT_STATUS):
            sel = idx[(kind == mode) & (noop == 0)].astype(np.int64)
            if not sel.size:
                continue
            ptrs = np.ascontiguousarray(b_ptr[sel])
            ls = np.ascontiguousarray(b_len[sel].astype(np.uint64))
            out = G.Bodies()
            t0 = time.perf_counter()
            G._chk(lib.gpudiff_upsert_bodies(eng.ctx, ptrs.ctypes.data_as(C.POINTER(C.c_void_p)),
                                             ls.ctypes.data_as(C.POINTER(C.c_size_t)), sel.size, mode, C.byref(out)),
                   "gpudiff_upsert_bodies")
            lib.gpudiff_bodies_release(eng.ctx, C.byref(out))
            ms += (time.perf_counter() - t0) * 1e3
            up += int(ls.sum())
        return ms, up

    plan_ms, upsert_ms, fold, k10, pack = [], [], [], [], []
    stats = up_bytes = total = None
    for rep in range(args.reps + 1):  # the first round warms both paths (buffers grow, code objects load)
        ms, idx, kind, noop, total = plan_once()
        s = st.plan_stats()
        ums, up_bytes = upsert_once(idx, kind, noop)
        if rep:
            plan_ms.append(ms)
            upsert_ms.append(ums)
            fold.append(s.fold_ms)
            k10.append(s.k10_ms)
            pack.append(s.pack_ms)
            stats = s
    dirty = int(np.count_nonzero(res.pair_flags & (G.SPEC_DIRTY | G.STATUS_DIRTY)))
    med = statistics.median(plan_ms)
    print(json.dumps({
        "bench": "store_plan", "build_id": G.BUILD_ID, "events": M, "dirty_events": dirty, "reps": args.reps,
        "json_bytes_batch": int(b_len.sum()), "docs": int(stats.docs), "writes": int(stats.writes),
        "noops": int(stats.noops), "bodies": int(stats.bodies), "host_bodies": int(stats.host_bodies),
        "plan_ms": _spread(plan_ms), "fold_ms": _spread(fold), "k10_ms": _spread(k10), "pack_ms": _spread(pack),
        "writes_per_s": round(stats.writes / (med / 1e3)), "bodies_per_s": round(stats.bodies / (med / 1e3)),
        "body_bytes": int(stats.body_bytes), "d2h_bytes": int(stats.d2h_bytes), "h2d_bytes": int(stats.h2d_bytes),
        "arena_bytes": int(stats.arena_bytes), "upsert_ms": _spread(upsert_ms), "upsert_h2d_bytes": up_bytes,
    }))
    assert total == stats.body_bytes or stats.host_bodies
    st.free()
    eng.close()


if __name__ == "__main__":
    main()
