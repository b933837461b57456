"""The write plan of a watch-replay batch (gpudiff_store_write_plan_get): for a waited batch of a
device-encode store, one write per dirty slot and kind, rendering the slot's last version of the batch with K10 from
the JSON staged in HBM -- K17 folds each slot chain's final flags, K18 compacts the write list and K10's table,
K19 packs the bodies to dense offsets.  Every plan is compared with tests/store_plan_model.py byte for byte:
pair_index, kind, noop, body and status (None = undecodable).  Path hashes are full width and first sightings carry
old_json, so no conservative collision result enters."""
import json

import pytest

from kcp_amd import gpudiff as G
from tests import store_plan_cases as C
from tests.golden.kat_cases import cases
from tests.store_plan_model import StoreModel, plan_of, plan_tuples
from tests.test_gpu_store import _stream

pytestmark = pytest.mark.gpu

LAYOUTS = pytest.mark.parametrize("zc", [False, True], ids=["staged", "zero_copy"])


def _flags(r):
    if r["decode_error"]:
        return G.SPEC_DIRTY | G.STATUS_DIRTY | G.DECODE_ERROR
    return ((G.SPEC_DIRTY if r["spec_dirty"] else 0) | (G.STATUS_DIRTY if r["status_dirty"] else 0) |
            (G.SPEC_NOOP if r["spec_noop"] else 0) | (G.STATUS_NOOP if r["status_noop"] else 0))


def _submit(st, events, zc=False):
    return st.submit([(s, nj, oj, i, s % 7) for i, (s, nj, oj) in enumerate(events)], zero_copy=zc)


def _compare(st, ticket, events, results, chains, modes=(G.PLAN_INFORMER,)):
    plan = None
    for mode in modes:
        plan = st.write_plan(ticket, mode)
        got, want = plan_tuples(plan), plan_of(events, results, chains, mode)
        assert len(got) == len(want), (mode, len(got), len(want))
        for g, w in zip(got, want):
            assert g == w, (mode, g[:3], w[:3], (g[3] or b"")[:200], (w[3] or b"")[:200])
        assert plan.n_host == int((plan.source == G.BODY_HOST).sum())
    return plan


def _check(eng, st, model, events, modes=(G.PLAN_INFORMER,), zc=False):
    """Submits, waits, and compares the batch's flags and plans with the model; returns the last plan."""
    t = _submit(st, events, zc)
    res = eng.wait(t)
    results, chains = model.replay(events)
    assert res.pair_flags.tolist() == [_flags(r) for r in results]
    return _compare(st, t, events, results, chains, modes), t


@LAYOUTS
def test_replay_stream_plans(zc):
    """60 slots, 4 batches of 150 events: many chains per batch, the plan after each wait."""
    eng = G.Engine(device=0, encode_threads=4)
    st = eng.object_store(max_slots=60, space_bytes=64 << 20, max_events=256, device_encode=True)
    model = StoreModel()
    n_writes = 0
    for evs, _pairs in _stream(11, 60, 4, 150):
        plan, t = _check(eng, st, model, evs, (G.PLAN_INFORMER, G.PLAN_SPEC, G.PLAN_STATUS,
                                               G.PLAN_SPEC | G.PLAN_STATUS), zc)
        n_writes += len(plan.bodies)
        with pytest.raises(G.GpuDiffError) as ei:  # store events are informer events
            st.write_plan(t, G.PLAN_UPSTREAM_DOWNSTREAM)
        assert ei.value.code == G.E_INVAL
    assert n_writes > 100
    s = st.plan_stats()
    assert s.calls == 16 and s.events == 150 and s.writes == len(plan.bodies)
    st.free()
    eng.close()


def _cm(i, v):
    # with a status member: an object without one is status-dirty (a no-op write) against any old version, and the
    # last batch below has to be clean in both regions
    return json.dumps({"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": "c%d" % i, "namespace": "d"},
                       "data": {"k": "v%d" % v}, "status": {"seen": 1}}, separators=(",", ":")).encode()


@LAYOUTS
def test_scan_and_wave_boundaries(zc):
    """1,100 spec-dirty first sightings (2,200 staged documents: three 1,024 tiles, writes past one tile, dozens of
    64-document waves); then 1,100 events round-robin on 9 slots (chains of ~122 documents that cross every wave
    and tile boundary); then an all-clean batch (no writes: nothing is launched after the counts)."""
    eng = G.Engine(device=0, encode_threads=4)
    st = eng.object_store(max_slots=1100, space_bytes=64 << 20, max_events=1100, device_encode=True)
    model = StoreModel()
    plan, _ = _check(eng, st, model, [(i, _cm(i, 1), _cm(i, 0)) for i in range(1100)], zc=zc)
    assert plan.pair_index.tolist() == list(range(1100)) and not plan.noop.any() and plan.n_host == 0
    s = st.plan_stats()
    assert (s.docs, s.writes, s.bodies) == (2200, 1100, 1100)
    assert s.body_bytes == sum(len(b) for b in plan.bodies)
    # only the bodies (and 22 B a write of list) come back, not K10's arena
    assert s.d2h_bytes <= s.body_bytes + 22 * s.writes + 96 and s.arena_bytes > 3 * s.body_bytes
    plan, _ = _check(eng, st, model, [(k % 9, _cm(k % 9, 2 + k // 9 % 3), None) for k in range(1100)], zc=zc)
    assert plan.pair_index.tolist() == list(range(1091, 1100))
    plan, _ = _check(eng, st, model, [(i, model.resident[i], None) for i in range(0, 1100, 7)], zc=zc)
    assert len(plan.bodies) == 0 and st.plan_stats().writes == 0
    st.free()
    eng.close()


@LAYOUTS
def test_body_packing_every_offset_residue(zc):
    """17 adjacent bodies of consecutive lengths L .. L + 16 (L = 96: with it the 18 dense offsets behind the first
    body take every residue mod 16, and so mod 4, the copy's granule), between two 3-byte bodies ({} renders as
    '{}' and a newline)."""
    eng = G.Engine(device=0, encode_threads=2)
    st = eng.object_store(max_slots=32, space_bytes=8 << 20, max_events=64, device_encode=True)
    model = StoreModel()
    old = b'{"spec":{"s":"?"}}'
    events = [(0, b"{}", old)]
    events += [(1 + k, b'{"spec":{"s":"' + b"x" * (78 + k) + b'"}}', old) for k in range(17)]
    events += [(20, b"{}", old)]
    plan, _ = _check(eng, st, model, events, (G.PLAN_INFORMER, G.PLAN_SPEC), zc)
    lens = [len(b) for b in plan.bodies]
    assert lens[0] == 3 and lens[18] == 3 and lens[1:18] == list(range(96, 96 + 17))
    assert len({sum(lens[:k]) % 16 for k in range(1, 19)}) == 16
    st.free()
    eng.close()


def test_noops_and_host_paths():
    """The write-path no-op KATs (x31 - x35) and the hand-made chains as slot chains; last versions K10 leaves to
    the host (a float beyond its exact conversion, a duplicate key) come back with the host's identical bytes; an
    undecodable last version is listed with GPUDIFF_E_DECODE; an event K0 defers (an escaped key) reaches the plan
    with its host-resolved flags."""
    eng = G.Engine(device=0, encode_threads=2)
    st = eng.object_store(max_slots=64, space_bytes=16 << 20, max_events=128, device_encode=True)
    model = StoreModel()
    kats = [(a, b) for n, a, b, _, _ in cases() if n[:3] in ("x31", "x32", "x33", "x34", "x35")]
    assert len(kats) == 5
    # batch 1: each KAT's old version becomes resident (clean against its own old_json); the chains
    chain_events, _want = C.chain_batch()
    base = 1 + max(s for s, _n, _o in chain_events)
    events = chain_events + [(base + k, a, a) for k, (a, _b) in enumerate(kats)]
    plan, _ = _check(eng, st, model, events)
    assert plan.noop.sum() >= 3 and (plan.noop == 0).any()
    # batch 2: the KATs' new versions, each followed by metadata churn of nothing (the same bytes: clean)
    events = []
    for k, (_a, b) in enumerate(kats):
        events += [(base + k, b, None), (base + k, b, None)]
    plan, _ = _check(eng, st, model, events)
    assert plan.noop.tolist().count(1) >= 3  # x31 spec, x33 status, x35 spec
    # batch 3: host paths.  slot 40: a float K10 leaves to the host; 41: a duplicate key (K0 defers the event too);
    # 42: an escaped key (K0 defers, its flags are host-resolved); 43: undecodable last version after a good one
    dup = C.V0[:-1] + b',"zz":1,"zz":2}'
    esc = C.V0[:-1] + b',"k\\u0065y":"v"}'
    flo = C.spec_edit(C.V0).replace(b'"revisionHistoryLimit":11', b'"revisionHistoryLimit":1.5e300,"tiny":5e-324')
    events = [(40, flo, C.V0), (41, dup, C.V0), (42, C.V0, C.V0), (42, esc, None), (43, C.spec_edit(C.V0), C.V0),
              (43, b'{"spec": ', None)]
    plan, _ = _check(eng, st, model, events)
    got = {(int(i), int(k)): (b, int(src)) for i, k, b, src in zip(plan.pair_index, plan.kind, plan.bodies, plan.source)}
    assert got[(1, 0)][1] == G.BODY_HOST and b'"zz":2' in got[(1, 0)][0] and b'"zz":1' not in got[(1, 0)][0]
    assert got[(0, 0)][0].count(b"1.5e+300") == 1
    assert got[(3, 0)][0] is not None and b'"key":"v"' in got[(3, 0)][0]
    assert got[(5, 0)] == (None, G.BODY_HOST) and got[(5, 1)] == (None, G.BODY_HOST)
    assert st.stats().deferred >= 2 and plan.n_host >= 3
    st.free()
    eng.close()


def test_state_errors_two_in_flight_and_read_marker():
    eng = G.Engine(device=0, encode_threads=4)
    st = eng.object_store(max_slots=50, space_bytes=32 << 20, max_events=200, device_encode=True)
    model = StoreModel()
    stream = [evs for evs, _p in _stream(5, 50, 5, 120)]
    want = []
    for evs in stream:
        results, chains = model.replay(evs)
        want.append((results, chains))

    def state_error(store, ticket):
        with pytest.raises(G.GpuDiffError) as ei:
            store.write_plan(ticket)
        assert ei.value.code == G.E_STATE

    t0 = _submit(st, stream[0])
    t1 = _submit(st, stream[1])
    state_error(st, t0)  # not waited yet
    state_error(st, t1)
    state_error(st, 0)
    state_error(st, t1 + 1000)  # unknown
    r0 = eng.wait(t0)
    _compare(st, t0, stream[0], *want[0])  # batch 1 still in flight behind it
    state_error(st, t1)
    r1 = eng.wait(t1)
    # two waited batches on the ring: either order, and again
    _compare(st, t1, stream[1], *want[1])
    _compare(st, t0, stream[0], *want[0], modes=(G.PLAN_STATUS, G.PLAN_INFORMER))
    _compare(st, t1, stream[1], *want[1], modes=(G.PLAN_SPEC,))
    assert r0.pair_flags.tolist() == [_flags(r) for r in want[0][0]]
    assert r1.pair_flags.tolist() == [_flags(r) for r in want[1][0]]
    # the submit after a plan call reuses the ring slot the plan just read (its upload waits for the read marker):
    # its diff results and its own plan are still the model's
    t2 = _submit(st, stream[2])
    state_error(st, t0)  # t0's ring slot holds batch 2 now
    _compare(st, t1, stream[1], *want[1])  # t1's is untouched while batch 2 runs
    r2 = eng.wait(t2)
    assert r2.pair_flags.tolist() == [_flags(r) for r in want[2][0]]
    _compare(st, t2, stream[2], *want[2])
    t3 = _submit(st, stream[3])
    state_error(st, t1)
    t4_events = stream[4]
    r3 = eng.wait(t3)
    assert r3.pair_flags.tolist() == [_flags(r) for r in want[3][0]]
    t4 = _submit(st, t4_events)
    _compare(st, t3, stream[3], *want[3])  # while batch 4 is in flight
    eng.wait(t4)
    _compare(st, t4, t4_events, *want[4])
    # the plan does not look at forget: a slot forgotten after the wait is still listed
    plan_before = plan_tuples(st.write_plan(t4))
    st.forget(stream[4][-1][0])
    assert plan_tuples(st.write_plan(t4)) == plan_before
    st.free()
    # a host-encode store keeps no JSON in HBM
    host = eng.object_store(max_slots=50, space_bytes=32 << 20, max_events=200, device_encode=False)
    th = _submit(host, stream[0])
    eng.wait(th)
    state_error(host, th)
    host.free()
    eng.close()
