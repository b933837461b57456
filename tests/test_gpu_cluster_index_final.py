"""gpudiff_cluster_index_get_final (kernels K26 - K28, kcp_amd/csrc/fanout_live.hip, in front of K23 - K25) on the GPU:
the cluster index of the tickets gpudiff_cluster_index_get refuses -- device-encoded submits and store tickets, whose
deferred rows the host resolved -- and of the ones it serves.

Expected flags are the oracle's decisions on the JSON pairs; the expected index is tests/cluster_index_model.py over
those flags.  Every case also holds the index to cluster_index_host over the waited result's pair_flags."""
import numpy as np
import pytest

from kcp_amd import gpudiff as G
from tests.cluster_index_model import assert_index_equals, model
from tests.parity import expected_flags, oracle_batch

pytestmark = pytest.mark.gpu

SPEC, STATUS, DECODE = 0x1, 0x2, 0x4
ARRAYS = ("cluster_ids", "spec_off", "status_off", "spec_ids", "status_ids")
ST = b',"status":{"x":0}}'
ST1 = b',"status":{"x":1}}'
# regular pairs: K0 encodes them, the device's flags are final
BOTH = (b'{"a":0}', b'{"a":1}')
CLEAN = (b'{"a":0' + ST, b'{"a":0' + ST)
SPEC_ONLY = (b'{"a":0' + ST, b'{"a":1' + ST)
STATUS_ONLY = (b'{"a":0' + ST, b'{"a":0' + ST1)
# pairs K0 defers to the host (the triggers of tests/test_gpu_store.py): the device lists them dirty in both kinds
ESC = b'{"a":0,"k\\u0065y":"v"'
D_CLEAN = (ESC + ST, ESC + ST)                                   # an escaped key, identical objects: final clean
D_SPEC = (ESC + ST, b'{"a":1,"k\\u0065y":"v"' + ST)              # final dirty in spec only
D_STATUS = (ESC + ST, ESC + ST1)                                 # final dirty in status only
D_BIG = (b'{"a":0,"big":123456789012345678901234567' + ST,) * 2  # more than 19 digits, identical: final clean
D_DUP = (b'{"a":0,"zz":1,"zz":2' + ST,) * 2                      # a duplicate key, identical: final clean
BROKEN = (b'{"a":', b'{"a":0}')                                  # undecodable: dirty in both, by its flags
_oracle = {}


def oracle_flags(pairs):
    """The oracle's flags of each pair (a pure function of the pair: decided once per distinct pair)."""
    new = [p for p in dict.fromkeys(pairs) if p not in _oracle]
    for p, r in zip(new, oracle_batch(new)):
        _oracle[p] = expected_flags(r)
    return np.array([_oracle[p] for p in pairs], dtype=np.uint8)


def test_the_pairs_are_what_their_names_say():
    want = {BOTH: SPEC | STATUS, CLEAN: 0, SPEC_ONLY: SPEC, STATUS_ONLY: STATUS, D_CLEAN: 0, D_SPEC: SPEC,
            D_STATUS: STATUS, D_BIG: 0, D_DUP: 0, BROKEN: SPEC | STATUS | DECODE}
    got = oracle_flags(list(want))
    assert [int(f) & 7 for f in got] == list(want.values())


@pytest.fixture(scope="module")
def dev():
    """One device-encoding context for the module: its pair store's two spaces are allocated once."""
    e = G.Engine(device=0, encode_threads=4, device_encode=True)
    yield e
    e.close()


def deferred(e):
    """pairs the context's device-encoding submits have left to the host so far"""
    try:
        return e.submit_stats().deferred
    except G.GpuDiffError:  # no device-encoded submit yet
        return 0


def interleave(dirty_pairs, dirty_clusters, seed=0):
    """Clean pairs between the listed ones (every third, and two in front), so dirty_idx is not the identity."""
    rng = np.random.default_rng(seed)
    pairs, clusters = [CLEAN, CLEAN], [0xFFFFFFFE, 3]
    for k, (p, c) in enumerate(zip(dirty_pairs, dirty_clusters)):
        if k % 3 == 0:
            pairs.append(CLEAN)
            clusters.append(int(rng.integers(0, 2 ** 32)))
        pairs.append(p)
        clusters.append(int(c))
    ids = (np.arange(len(pairs), dtype=np.uint32) * 3 + 1000).tolist()  # pair ids are not positions
    return pairs, ids, clusters


def check_final(e, ticket, pairs, ids, clusters, what="", res=None):
    """wait (unless the result is given) + the final index, held to the model over the oracle's flags and to the host
    routine over the result's own.  -> (result, index, the statistics' deltas)"""
    if res is None:
        res = e.wait(ticket)
    exp = oracle_flags(pairs)
    assert np.array_equal(res.pair_flags & 3, exp & 3), (what, np.flatnonzero((res.pair_flags & 3) != (exp & 3))[:8])
    old = e.cluster_index_stats().as_dict()
    before = e.cluster_index_final_stats().as_dict()
    ci = e.cluster_index_final(ticket)
    after = e.cluster_index_final_stats().as_dict()
    assert e.cluster_index_stats().as_dict() == old  # the old call's statistics are not the new call's
    assert_index_equals(ci, model(exp, ids, clusters), what)
    host = G.cluster_index_host(res.pair_flags, ids, clusters)
    for k in ARRAYS:
        assert np.array_equal(getattr(ci, k), getattr(host, k)), (what, k)
    assert ci.spec_ids.size == res.spec_dirty_ids.size and ci.status_ids.size == res.status_dirty_ids.size
    d = {k: after[k] - before[k] for k in after}
    assert d["calls"] == 1 and d["sorted_calls"] == ci.sorted_on_device and d["timed_calls"] == 0
    assert d["entries_live"] == res.dirty_ids.size and d["entries_in"] >= d["entries_live"]
    assert d["patched_calls"] == (1 if d["patch_rows"] else 0)
    assert d["compacted_calls"] == (1 if d["patch_rows"] and 0 < d["entries_live"] < d["entries_in"] else 0)
    assert d["h2d_bytes"] == (8 * d["patch_rows"] if d["entries_live"] else 0)
    if res.dirty_ids.size == 0:
        assert d["syncs"] == 0 and d["d2h_bytes"] == 0
    else:  # at most four synchronisations, three without host-resolved rows
        assert d["syncs"] == (4 if d["patch_rows"] else 3), d
        assert d["d2h_bytes"] == 4 * (3 * ci.cluster_ids.size + 2 + ci.spec_ids.size + ci.status_ids.size)
    return res, ci, d


# ---------------------------------------------------------------- 1. deferred rows resolved by the host, one batch
def test_deferred_rows_resolved_by_the_host(dev):
    pairs = [D_CLEAN, BOTH, D_SPEC, D_STATUS, BROKEN, CLEAN, D_BIG, D_DUP, SPEC_ONLY, D_CLEAN]
    clusters = [40, 41, 42, 43, 44, 45, 41, 46, 46, 47]  # 40, 45 and 47 hold no final-dirty row
    ids = list(range(100, 100 + len(pairs)))
    d0 = deferred(dev)
    res, ci, d = check_final(dev, dev.submit(pairs, ids, clusters), pairs, ids, clusters, "resolved rows")
    assert deferred(dev) - d0 >= 6  # the six escaped-key, long-integer and duplicate-key pairs at least
    assert [int(f) & 3 for f in res.pair_flags] == [0, 3, 1, 2, 3, 0, 0, 0, 1, 0]
    assert int(res.pair_flags[4]) & DECODE
    assert ci.cluster_ids.tolist() == [41, 42, 43, 44, 46]
    assert [s.tolist() for s in ci.of(42)] == [[102], []] and [s.tolist() for s in ci.of(43)] == [[], [103]]
    assert [s.tolist() for s in ci.of(44)] == [[104], [104]]  # the undecodable pair: both kinds
    assert [s.tolist() for s in ci.of(46)] == [[108], []]     # the duplicate-key pair of 46 resolved clean
    assert d["patch_rows"] >= 6 and d["entries_in"] == 9 and d["compacted_calls"] == 1


# ---------------------------------------------------------------- 2. device-encoded submits at the kernels' edges
EDGES = [1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049]  # the 16-byte load's, the wave's and the tile's edges
DROPS = (0, 1023, 1024)  # and the last


def layout(kind, n):
    if kind == "ascending":
        return list(range(5, 5 + n))
    if kind == "descending":
        return list(range(4_000_000_000, 4_000_000_000 - n, -1))
    rng = np.random.default_rng(n)
    if kind == "shuffled":
        return rng.integers(0, 40, n).tolist()
    return rng.choice(np.array([0, 2 ** 32 - 1], np.uint64), size=n).tolist()  # "extremes"


def listed_pairs(n, drop):
    """n pairs the device lists dirty.  Those at list positions 0, 1023, 1024 and the last are deferred: final clean
    (dropped from the list) when `drop`, else final dirty in spec alone.  The rest mix the kinds, with a deferred
    status-only pair every seventh."""
    cycle = [BOTH, SPEC_ONLY, STATUS_ONLY, BOTH, SPEC_ONLY]
    out = [D_STATUS if k % 7 == 6 else cycle[k % 5] for k in range(n)]
    for k in DROPS + (n - 1,):
        if k < n:
            out[k] = D_CLEAN if drop else D_SPEC
    return out


@pytest.mark.parametrize("kind,drop", [("ascending", True), ("descending", True), ("shuffled", True),
                                       ("extremes", True), ("shuffled", False)])
@pytest.mark.parametrize("n", EDGES)
def test_device_submit_edges(dev, n, kind, drop):
    lp, cl = listed_pairs(n, drop), layout(kind, n)
    pairs, ids, clusters = interleave(lp, cl, seed=n)
    d0 = deferred(dev)
    res, ci, d = check_final(dev, dev.submit(pairs, ids, clusters), pairs, ids, clusters, "%s n=%d" % (kind, n))
    assert deferred(dev) - d0 > 0
    assert d["entries_in"] == n  # the device's list: every listed pair, no interleaved clean one
    n_drop = len({k for k in DROPS + (n - 1,) if k < n}) if drop else 0
    assert d["entries_live"] == n - n_drop and d["patched_calls"] == 1
    # patches with nothing dropped: a patched call that did not compact
    assert d["compacted_calls"] == (1 if 0 < n - n_drop < n else 0)
    live_cl = [c for p, c in zip(lp, cl) if p is not D_CLEAN]
    assert ci.cluster_ids.tolist() == sorted(set(live_cl))
    if kind == "ascending" or n - n_drop <= 1:
        assert ci.sorted_on_device == 0
    elif kind == "descending":
        assert ci.sorted_on_device == 1


# ---------------------------------------------------------------- 3. heads, whole clusters and whole lists dropped
@pytest.mark.parametrize("descending", [False, True])
def test_dropped_head_and_dropped_cluster(dev, descending):
    # cluster 5's first listed entry is dropped: its second becomes the head; every entry of cluster 6 is dropped
    lp = [D_CLEAN, BOTH, SPEC_ONLY, D_CLEAN, D_BIG, D_DUP, STATUS_ONLY, D_CLEAN, D_STATUS]
    cl = [5, 5, 5, 6, 6, 6, 7, 8, 8]
    if descending:
        cl = [100 - c for c in cl]
    pairs, ids, clusters = interleave(lp, cl, seed=1)
    res, ci, d = check_final(dev, dev.submit(pairs, ids, clusters), pairs, ids, clusters, "heads")
    want = [5, 7, 8]
    assert ci.cluster_ids.tolist() == sorted((100 - c) if descending else c for c in want)
    assert ci.sorted_on_device == int(descending)
    first = ci.of(95 if descending else 5)
    assert first[0].tolist() == [ids[pairs.index(BOTH)], ids[pairs.index(SPEC_ONLY)]]
    assert first[1].tolist() == [ids[pairs.index(BOTH)]]
    assert d["entries_in"] == 9 and d["entries_live"] == 4 and d["compacted_calls"] == 1


def test_every_entry_dropped(dev):
    lp = [D_CLEAN, D_BIG, D_DUP, D_CLEAN, D_CLEAN]
    pairs, ids, clusters = interleave(lp, [9, 8, 7, 7, 9])
    res, ci, d = check_final(dev, dev.submit(pairs, ids, clusters), pairs, ids, clusters, "all dropped")
    assert res.dirty_ids.size == 0 and ci.cluster_ids.size == 0
    assert ci.spec_off.tolist() == [0] and ci.status_off.tolist() == [0]
    assert d["entries_in"] == 5 and d["patch_rows"] == 5 and d["syncs"] == 0 and d["patched_calls"] == 1


def test_batch_without_a_deferral(dev):
    n = 1500
    pairs, ids, clusters = interleave([BOTH, SPEC_ONLY, STATUS_ONLY] * (n // 3), layout("shuffled", n), seed=5)
    d0 = deferred(dev)
    res, ci, d = check_final(dev, dev.submit(pairs, ids, clusters), pairs, ids, clusters, "no deferral")
    assert deferred(dev) == d0
    assert d["patch_rows"] == 0 and d["patched_calls"] == 0 and d["compacted_calls"] == 0 and d["h2d_bytes"] == 0
    assert d["syncs"] == 3 and d["entries_in"] == d["entries_live"] == n
    # the ring's two batches and the first again, two tickets in flight, each indexed after its own wait
    t1 = dev.submit(pairs[:400], ids[:400], clusters[:400])
    lp = listed_pairs(70, True)
    p2, i2, c2 = interleave(lp, layout("descending", 70), seed=6)
    t2 = dev.submit(p2, i2, c2)
    check_final(dev, t1, pairs[:400], ids[:400], clusters[:400], "two in flight, first")
    r2, ci2, d2 = check_final(dev, t2, p2, i2, c2, "two in flight, second")
    assert d2["compacted_calls"] == 1
    t3 = dev.submit(pairs[:10], ids[:10], clusters[:10])  # t1's ring slot again
    with pytest.raises(G.GpuDiffError) as ei:
        dev.cluster_index_final(t1)
    assert ei.value.code == G.E_STATE
    again = dev.cluster_index_final(t2)  # the other slot's batch is still the waited one
    for k in ARRAYS:
        assert np.array_equal(getattr(again, k), getattr(ci2, k))
    check_final(dev, t3, pairs[:10], ids[:10], clusters[:10], "the slot's next batch")


# ---------------------------------------------------------------- 4. stores, host- and device-encoded
def _state(call):
    with pytest.raises(G.GpuDiffError) as ei:
        call()
    assert ei.value.code == G.E_STATE


@pytest.mark.parametrize("device_encode", [False, True], ids=["host_encode", "device_encode"])
def test_store_tickets(device_encode):
    e = G.Engine(device=0, encode_threads=2)
    st = e.object_store(64, 8 << 20, 64, device_encode=device_encode)
    cur = {}

    def submit(events):
        """events: [(slot, new, cluster)] -> ticket, the (old, new) pairs the store diffs, ids, clusters"""
        items, pairs, ids, clusters = [], [], [], []
        for k, (slot, new, cluster) in enumerate(events):
            old = cur.get(slot, b"{}")
            items.append((slot, new, cur.get(slot), 500 + 2 * k, cluster))
            pairs.append((old, new))
            ids.append(500 + 2 * k)
            clusters.append(cluster)
            cur[slot] = new
        return st.submit(items), pairs, ids, clusters

    try:
        # first sightings on distinct slots (each diffs against {}), two clusters
        t, pairs, ids, clusters = submit([(0, CLEAN[0], 2), (1, ESC + ST, 1), (2, BOTH[0], 2), (3, CLEAN[0], 1)])
        check_final(e, t, pairs, ids, clusters, "first sightings")
        # distinct slots over two clusters: one event deferred and final clean, one deferred and status-dirty
        t, pairs, ids, clusters = submit([(0, SPEC_ONLY[1], 2), (1, ESC + ST, 1), (2, BOTH[1], 2), (3, CLEAN[0], 1)])
        res, ci, d = check_final(e, t, pairs, ids, clusters, "distinct slots")
        assert [int(f) & 3 for f in res.pair_flags] == [1, 0, 3, 0] and ci.cluster_ids.tolist() == [2]
        if device_encode:
            assert st.stats().deferred > 0 and d["patch_rows"] >= 1 and d["compacted_calls"] == 1
        else:
            assert d["patch_rows"] == 0
        # a slot with two events in one batch: they chain
        t, pairs, ids, clusters = submit([(1, ESC + ST1, 1), (0, CLEAN[0], 2), (1, ESC + ST1, 1), (3, STATUS_ONLY[1], 7)])
        res, ci, d = check_final(e, t, pairs, ids, clusters, "two events on a slot")
        assert [int(f) & 3 for f in res.pair_flags] == [2, 1, 0, 2] and ci.cluster_ids.tolist() == [1, 2, 7]
        # two tickets in flight, each indexed after its own wait
        ta, pa, ia, ca = submit([(4, BOTH[0], 9), (5, ESC + ST, 8)])
        tb, pb, ib, cb = submit([(4, BOTH[1], 9), (5, ESC + ST, 8), (6, CLEAN[0], 8)])
        _state(lambda: e.cluster_index_final(ta))  # not waited yet
        check_final(e, ta, pa, ia, ca, "in flight, first")
        _state(lambda: e.cluster_index_final(tb))
        rb, cib, db = check_final(e, tb, pb, ib, cb, "in flight, second")
        assert cib.cluster_ids.tolist() == [8, 9]
        again = e.cluster_index_final(ta)  # both ring slots hold their waited batch
        assert again.cluster_ids.tolist() == [8, 9]
        # the ring slot's next submit ends a ticket's window
        tc, pc, ic, cc = submit([(6, CLEAN[0], 8)])
        _state(lambda: e.cluster_index_final(ta))
        check_final(e, tb, pb, ib, cb, "the other slot", res=rb)
        rc, cic, dc = check_final(e, tc, pc, ic, cc, "nothing dirty")
        assert cic.cluster_ids.size == 0
        _state(lambda: e.cluster_index(tb))  # the old call still refuses every store ticket
        assert e.cluster_index_stats().as_dict()["calls"] == 0
    finally:
        st.free()
        e.close()


# ---------------------------------------------------------------- 5. tickets the old call serves
def test_resident_batch_and_host_encoded_submit_equal_the_old_call():
    e = G.Engine(device=0, encode_threads=4)
    n = 1500
    pairs, ids, clusters = interleave([BOTH, SPEC_ONLY, STATUS_ONLY, BROKEN, D_SPEC] * (n // 5),
                                      layout("shuffled", n), seed=2)
    hb = e.encode(pairs, ids, clusters)
    db = e.device_batch(hb.info().pool_bytes + 4096, len(pairs))
    db.append(hb)
    try:
        for what, ticket in (("resident", e.diff(db)), ("submit", e.submit(pairs, ids, clusters))):
            res, ci, d = check_final(e, ticket, pairs, ids, clusters, what)
            assert d["patch_rows"] == 0 and d["syncs"] == 3 and d["entries_in"] == d["entries_live"]
            old = e.cluster_index(ticket)
            for k in ARRAYS:
                assert np.array_equal(getattr(ci, k), getattr(old, k)), (what, k)
            assert ci.sorted_on_device == old.sorted_on_device == 1
        hb2 = e.encode([CLEAN] * 5, list(range(5)), [1] * 5)  # nothing dirty: nothing launched
        db.reset()
        db.append(hb2)
        res, ci, d = check_final(e, e.diff(db), [CLEAN] * 5, list(range(5)), [1] * 5, "clean")
        assert ci.cluster_ids.size == 0 and d["syncs"] == 0
        hb2.free()
    finally:
        db.free()
        hb.free()
        e.close()


# ---------------------------------------------------------------- 6. call order, statistics, timing
def test_call_order_and_statistics():
    e = G.Engine(device=0, encode_threads=2, device_encode=True)
    try:
        assert e.cluster_index_final_stats().as_dict()["calls"] == 0
        _state(lambda: e.cluster_index_final(0))
        _state(lambda: e.cluster_index_final(12345))  # unknown
        pairs, ids, clusters = interleave(listed_pairs(100, True), layout("descending", 100))
        t = e.submit(pairs, ids, clusters)
        _state(lambda: e.cluster_index_final(t))  # between submit and wait
        res = e.wait(t)
        r, a, da = check_final(e, t, pairs, ids, clusters, "first call", res=res)
        r, b, db_ = check_final(e, t, pairs, ids, clusters, "second call", res=res)  # two calls: equal indexes
        for k in ARRAYS:
            assert np.array_equal(getattr(a, k), getattr(b, k))
        assert da["syncs"] == db_["syncs"] == 4 and da["compacted_calls"] == 1
        t2 = e.submit(pairs, ids, clusters)
        t3 = e.submit(pairs, ids, clusters)  # t's ring slot: superseded
        _state(lambda: e.cluster_index_final(t))
        _state(lambda: e.cluster_index_final(t3))  # and its successor not waited yet
        check_final(e, t2, pairs, ids, clusters, "the other slot")
        check_final(e, t3, pairs, ids, clusters, "the successor")
        st = e.cluster_index_final_stats().as_dict()
        assert st["calls"] == 4 and st["patched_calls"] == 4 and st["compacted_calls"] == 4 and st["syncs"] == 16
        assert st["entries_in"] == 400 and st["entries_live"] == 4 * 98 and st["sorted_calls"] == 4
        assert st["timed_calls"] == 0 and st["kernel_ms"] == 0.0  # the context does not time
        assert e.cluster_index_stats().as_dict()["calls"] == 0  # the old call's statistics are unmoved
    finally:
        e.close()


def test_timing_context_counts_kernel_time():
    e = G.Engine(device=0, encode_threads=2, device_encode=True, timing=True)
    try:
        pairs, ids, clusters = interleave(listed_pairs(300, True), layout("descending", 300))
        t = e.submit(pairs, ids, clusters)
        res = e.wait(t)
        ci = e.cluster_index_final(t)
        st = e.cluster_index_final_stats().as_dict()
        assert st["calls"] == 1 and st["timed_calls"] == 1 and st["kernel_ms"] > 0.0 and st["compacted_calls"] == 1
        host = G.cluster_index_host(res.pair_flags, ids, clusters)
        for k in ARRAYS:
            assert np.array_equal(getattr(ci, k), getattr(host, k)), k
    finally:
        e.close()
