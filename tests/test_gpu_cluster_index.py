"""gpudiff_cluster_index_get (kernels K23 - K25, kcp_amd/csrc/fanout.hip) on the GPU: Engine.cluster_index held to
the model of tests/cluster_index_model.py over the waited result's own flags, and to cluster_index_host, at the wave
and tile edges, on both paths (dirty list in cluster order / sorted on the device), for every kind of ticket the call
serves, and the call-order errors for the ones it does not."""
import numpy as np
import pytest

from kcp_amd import gpudiff as G
from tests.cluster_index_model import assert_index_equals, model

pytestmark = pytest.mark.gpu

SPEC, STATUS, DECODE = 0x1, 0x2, 0x4
# the smallest objects that decide anything
BOTH = (b'{"a":0}', b'{"a":1}')  # no status on either side: dirty in both kinds
CLEAN = (b'{"a":0,"status":{"x":0}}', b'{"a":0,"status":{"x":0}}')
SPEC_ONLY = (b'{"a":0,"status":{"x":0}}', b'{"a":1,"status":{"x":0}}')
STATUS_ONLY = (b'{"a":0,"status":{"x":0}}', b'{"a":0,"status":{"x":1}}')
BROKEN = (b'{"a":', b'{"a":0}')  # a decode error: dirty in both, by its flags
EDGES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049]  # the wave's and the tile's (kScanTile = 1024) edges


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(device=0, encode_threads=8)
    yield e
    e.close()


def interleave(dirty_pairs, dirty_clusters, seed=0):
    """Clean pairs between the dirty ones (every third, and two in front), so dirty_idx is not the identity; the clean
    pairs' clusters are arbitrary, they are never listed.  -> pairs, ids, clusters"""
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


def check_ticket(e, ticket, ids, clusters, what="", res=None):
    """wait (unless the result is given) + index: the index equals the model and the host routine over the result's
    own flags.  -> (result, index)"""
    if res is None:
        res = e.wait(ticket)
    before = e.cluster_index_stats().as_dict()
    ci = e.cluster_index(ticket)
    after = e.cluster_index_stats().as_dict()
    assert res.pair_flags.size == len(ids)
    assert_index_equals(ci, model(res.pair_flags, ids, clusters), what)
    host = G.cluster_index_host(res.pair_flags, ids, clusters)
    for k in ("cluster_ids", "spec_off", "status_off", "spec_ids", "status_ids"):
        assert np.array_equal(getattr(ci, k), getattr(host, k)), (what, k)
    assert ci.spec_ids.size == res.spec_dirty_ids.size and ci.status_ids.size == res.status_dirty_ids.size
    # the statistics: one call, at most three synchronisations, none when nothing is dirty
    assert after["calls"] == before["calls"] + 1
    assert after["sorted_calls"] == before["sorted_calls"] + ci.sorted_on_device
    syncs = after["syncs"] - before["syncs"]
    assert syncs == (3 if res.dirty_ids.size else 0), syncs
    assert after["entries"] == before["entries"] + res.dirty_ids.size
    if not ci.sorted_on_device:  # the dirty list ascends by cluster: the result's flat lists, element for element
        assert np.array_equal(ci.spec_ids, res.spec_dirty_ids) and np.array_equal(ci.status_ids, res.status_dirty_ids)
    return res, ci


def run(e, pairs, ids, clusters, what=""):
    hb = e.encode(pairs, ids, clusters)
    db = e.device_batch(hb.info().pool_bytes + 4096, max(len(pairs), 1))
    db.append(hb)
    try:
        return check_ticket(e, e.diff(db), ids, clusters, what)
    finally:
        db.free()
        hb.free()


# ---------------------------------------------------------------- 1. the wave and tile edges, four cluster layouts
def layout(kind, n):
    if kind == "equal":
        return [77] * n
    if kind == "ascending":
        return list(range(5, 5 + n))
    if kind == "descending":
        return list(range(4_000_000_000, 4_000_000_000 - n, -1))
    rng = np.random.default_rng(n)
    return rng.choice(np.array([0, 1, 9, 4096, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1], np.uint64), size=n).tolist()


@pytest.mark.parametrize("kind", ["equal", "ascending", "descending", "seven_shuffled"])
@pytest.mark.parametrize("n", EDGES)
def test_edges(eng, n, kind):
    cl = layout(kind, n)
    pairs, ids, clusters = interleave([BOTH] * n, cl, seed=n)
    res, ci = run(eng, pairs, ids, clusters, "%s n=%d" % (kind, n))
    assert res.dirty_ids.size == n and res.spec_dirty_ids.size == n and res.status_dirty_ids.size == n
    assert ci.cluster_ids.tolist() == sorted(set(cl))
    if kind in ("equal", "ascending"):
        assert ci.sorted_on_device == 0
    elif kind == "descending":
        assert ci.sorted_on_device == (1 if n > 1 else 0)
    else:
        ascends = all(a <= b for a, b in zip(cl, cl[1:]))
        assert ci.sorted_on_device == (0 if ascends else 1)
        if n >= 63:
            assert 0 in ci.cluster_ids.tolist() and 0xFFFFFFFF in ci.cluster_ids.tolist()


# ---------------------------------------------------------------- 2. heads on both sides of a tile edge
def test_runs_changing_at_the_tile_edge(eng):
    n = 2049
    cl = [10] * 1023 + [11, 12] + [13] * (n - 1025)  # the cluster changes exactly at dirty entries 1023, 1024, 1025
    pairs, ids, clusters = interleave([BOTH] * n, cl)
    res, ci = run(eng, pairs, ids, clusters, "runs at the tile edge")
    assert ci.sorted_on_device == 0
    assert ci.cluster_ids.tolist() == [10, 11, 12, 13] and ci.spec_off.tolist() == [0, 1023, 1024, 1025, n]
    assert ci.status_off.tolist() == ci.spec_off.tolist()


def test_one_entry_out_of_order_at_1024_takes_the_sort_path(eng):
    n = 2049
    cl = [5] * n
    cl[1024] = 4  # the first entry of the second tile, below its predecessor in the first
    pairs, ids, clusters = interleave([BOTH] * n, cl)
    res, ci = run(eng, pairs, ids, clusters, "one entry out of order")
    assert ci.sorted_on_device == 1
    assert ci.cluster_ids.tolist() == [4, 5] and ci.spec_off.tolist() == [0, 1, n]
    assert ci.spec_ids[0] == res.dirty_ids[1024]


# ---------------------------------------------------------------- 3. one kind only, and a decode error
@pytest.mark.parametrize("shuffled", [False, True])
def test_clusters_dirty_in_one_kind_only(eng, shuffled):
    kinds = [SPEC_ONLY, STATUS_ONLY, BOTH, BROKEN, CLEAN]
    rng = np.random.default_rng(11)
    pairs, clusters = [], []
    for c in range(40):  # cluster c holds pairs of one kind only: 5 c + 4 holds none that is dirty
        for _ in range(1 + c % 4):
            pairs.append(kinds[c % 5])
            clusters.append(100 + c)
    if shuffled:
        order = rng.permutation(len(pairs))
        pairs, clusters = [pairs[i] for i in order], [clusters[i] for i in order]
    ids = list(range(500, 500 + len(pairs)))
    res, ci = run(eng, pairs, ids, clusters, "one kind only")
    assert ci.sorted_on_device == int(shuffled)
    want = {SPEC_ONLY: SPEC, STATUS_ONLY: STATUS, BOTH: SPEC | STATUS, BROKEN: SPEC | STATUS | DECODE, CLEAN: 0}
    assert [int(f) & 7 for f in res.pair_flags] == [want[p] for p in pairs]  # the pairs are what their names say
    assert ci.cluster_ids.tolist() == [100 + c for c in range(40) if c % 5 != 4]
    for c in range(40):
        s, t = ci.of(100 + c)
        n_c = 1 + c % 4
        assert s.size == (n_c if c % 5 in (0, 2, 3) else 0), c   # status-only clusters: an empty spec slice
        assert t.size == (n_c if c % 5 in (1, 2, 3) else 0), c   # spec-only clusters: an empty status slice


# ---------------------------------------------------------------- 4. the top scan's second trip
def test_more_than_256_tiles(eng):
    """256 x 1024 + 1025 dirty entries: launch_scan64_top scans 256 tile sums a trip, so this is its second trip with
    a running total (tests/test_gpu_store.py uses the same bound for the same reason)."""
    n = 256 * 1024 + 1025
    rng = np.random.default_rng(3)
    clusters = rng.integers(0, 5000, n).astype(np.uint32)
    clusters[rng.integers(0, n, 50)] = 0xFFFFFFFF
    clusters[rng.integers(0, n, 50)] = 0
    ids = rng.permutation(n).astype(np.uint32)
    res, ci = run(eng, [BOTH] * n, ids.tolist(), clusters.tolist(), "more than 256 tiles")
    assert ci.sorted_on_device == 1 and res.dirty_ids.size == n
    assert ci.cluster_ids.size == np.unique(clusters).size


# ---------------------------------------------------------------- 5. a base and a view, two contexts; result slots
def test_base_and_view_from_two_contexts_and_result_slots(eng):
    eng2 = G.Engine(device=0, encode_threads=2)
    n = 1500
    cl = layout("seven_shuffled", n)
    pairs, ids, clusters = interleave([BOTH, SPEC_ONLY, STATUS_ONLY] * (n // 3), cl, seed=2)
    hb = eng.encode(pairs, ids, clusters)
    db = eng.device_batch(hb.info().pool_bytes + 4096, len(pairs))
    db.append(hb)
    eng.sync()  # the base's append before the view's diff
    view = db.view(eng2)
    try:
        t1, t2 = eng.diff(db), eng2.diff(view)  # both in flight
        r1, c1 = check_ticket(eng, t1, ids, clusters, "base")
        r2, c2 = check_ticket(eng2, t2, ids, clusters, "view")
        assert c1.sorted_on_device == c2.sorted_on_device == 1
        # a ticket belongs to its context
        with pytest.raises(G.GpuDiffError) as ei:
            eng2.cluster_index(max(t1, t2) + 100)
        assert ei.value.code == G.E_STATE
        # the same pass under result slot 1: the same index
        db.result_slot(1)
        t3 = eng.diff(db)
        r3, c3 = check_ticket(eng, t3, ids, clusters, "slot 1")
        db.result_slot(0)  # selecting a slot launches nothing: the ticket's index is still the waited pass's
        c4 = eng.cluster_index(t3)
        for c in (c3, c4):
            for k in ("cluster_ids", "spec_off", "status_off", "spec_ids", "status_ids"):
                assert np.array_equal(getattr(c, k), getattr(c1, k)), k
    finally:
        view.free()  # the view before its base
        db.free()
        hb.free()
        eng2.close()


# ---------------------------------------------------------------- 6. finalised K20 passes
@pytest.mark.parametrize("n", [1, 64, 4096])
def test_small_pass_context(n):
    e = G.Engine(device=0, encode_threads=8, small_pass=True)
    try:
        rng = np.random.default_rng(n)
        kinds = [BOTH, CLEAN, SPEC_ONLY, STATUS_ONLY, BOTH]
        pairs = [kinds[i % 5] for i in range(n)]
        clusters = rng.integers(0, 9, n).tolist()
        ids = (np.arange(n) + 70).tolist()
        before = e.pass_stats().as_dict()
        res, ci = run(e, pairs, ids, clusters, "small pass n=%d" % n)
        after = e.pass_stats().as_dict()
        assert after["small_passes"] == before["small_passes"] + 1 and after["small_redone"] == before["small_redone"]
        assert res.dirty_ids.size == sum(1 for p in pairs if p is not CLEAN)
    finally:
        e.close()


# ---------------------------------------------------------------- 7. a host-encoded gpudiff_submit ticket
def test_host_encoded_submit(eng):
    n = 700
    cl = layout("seven_shuffled", n)
    pairs, ids, clusters = interleave([BOTH, STATUS_ONLY] * (n // 2), cl, seed=4)
    for _ in range(3):  # the submit ring's two batches, and the first again
        t = eng.submit(pairs, ids, clusters)
        res, ci = check_ticket(eng, t, ids, clusters, "submit")
        assert ci.sorted_on_device == 1
    t_old = t
    t = eng.submit(pairs[:10], ids[:10], clusters[:10])
    t2 = eng.submit(pairs[:10], ids[:10], clusters[:10])  # the ring's other batch: t stays valid
    check_ticket(eng, t, ids[:10], clusters[:10], "submit, two in flight")
    check_ticket(eng, t2, ids[:10], clusters[:10], "submit, two in flight")
    with pytest.raises(G.GpuDiffError) as ei:  # t_old's batch was submitted again
        eng.cluster_index(t_old)
    assert ei.value.code == G.E_STATE


# ---------------------------------------------------------------- 8. one batch, two populations in turn
def test_alternating_populations(eng):
    """One batch reset and refilled in turn with two populations of equal shapes and complementary dirty sets, the
    index taken after each wait: a read of the previous pass's arrays (keys, tile sums, the block, the cached pinned
    buffer) would list the other population's pairs."""
    n = 3000
    rng = np.random.default_rng(8)
    clusters = rng.choice(np.array([0, 2, 3, 50, 51, 2 ** 32 - 1], np.uint64), size=n).tolist()
    ids = (np.arange(n) * 2 + 9).tolist()
    dirty = (CLEAN[0], b'{"a":1,"status":{"x":1}}')  # CLEAN's shape, one digit changed in each region
    pops = [[(dirty if i % 2 == par else CLEAN) for i in range(n)] for par in (0, 1)]
    hbs = [eng.encode(p, ids, clusters) for p in pops]
    assert hbs[0].info().pool_bytes == hbs[1].info().pool_bytes
    db = eng.device_batch(hbs[0].info().pool_bytes + 4096, n)
    try:
        for it in range(6):
            db.reset()
            db.append(hbs[it % 2])
            res, ci = check_ticket(eng, eng.diff(db), ids, clusters, "population %d" % (it % 2))
            assert res.spec_dirty_ids.tolist() == res.status_dirty_ids.tolist() == ids[it % 2::2]
    finally:
        db.free()
        for hb in hbs:
            hb.free()


# ---------------------------------------------------------------- 9. call order
def _state(call):
    with pytest.raises(G.GpuDiffError) as ei:
        call()
    assert ei.value.code == G.E_STATE


def test_call_order():
    e = G.Engine(device=0, encode_threads=2)
    pairs, ids, clusters = interleave([BOTH] * 100, layout("descending", 100))
    hb = e.encode(pairs, ids, clusters)
    db = e.device_batch(hb.info().pool_bytes + 4096, len(pairs))
    db.append(hb)
    try:
        assert e.cluster_index_stats().as_dict()["calls"] == 0
        _state(lambda: e.cluster_index(1))  # before the first diff
        _state(lambda: e.cluster_index(0))
        t = e.diff(db)
        _state(lambda: e.cluster_index(t))  # between diff and wait
        res = e.wait(t)
        r, a = check_ticket(e, t, ids, clusters, "first call", res=res)
        r, b = check_ticket(e, t, ids, clusters, "second call", res=res)  # two calls on one ticket: equal indexes
        for k in ("cluster_ids", "spec_off", "status_off", "spec_ids", "status_ids"):
            assert np.array_equal(getattr(a, k), getattr(b, k))
        t2 = e.diff(db)
        _state(lambda: e.cluster_index(t))   # superseded
        _state(lambda: e.cluster_index(t2))  # and its successor not waited yet
        check_ticket(e, t2, ids, clusters, "the successor")
        st = e.cluster_index_stats().as_dict()
        assert st["calls"] == 3 and st["sorted_calls"] == 3 and st["syncs"] == 9 and st["entries"] == 300
        assert st["timed_calls"] == 0 and st["kernel_ms"] == 0.0  # the context does not time
    finally:
        db.free()
        hb.free()
        e.close()


def test_tickets_whose_flags_the_host_may_patch():
    e = G.Engine(device=0, encode_threads=2, device_encode=True)
    try:
        t = e.submit([BOTH, CLEAN, BROKEN], [1, 2, 3], [9, 8, 7])
        res = e.wait(t)
        assert res.dirty_ids.tolist() == [1, 3]
        _state(lambda: e.cluster_index(t))  # a device-encoded submit
        assert e.cluster_index_stats().as_dict()["calls"] == 0
    finally:
        e.close()
    e = G.Engine(device=0, encode_threads=2)
    try:
        for dev in (False, True):
            st = e.object_store(16, 1 << 20, 16, device_encode=dev)
            t = st.submit([(0, BOTH[1], BOTH[0], 5, 1), (1, CLEAN[1], CLEAN[0], 6, 2)])
            assert e.wait(t).dirty_ids.tolist() == [5]
            _state(lambda: e.cluster_index(t))  # a store ticket, host- or device-encoded
            st.free()
        assert e.cluster_index_stats().as_dict()["calls"] == 0
    finally:
        e.close()


def test_timing_context_counts_kernel_time():
    e = G.Engine(device=0, encode_threads=2, timing=True)
    try:
        pairs, ids, clusters = interleave([BOTH] * 300, layout("descending", 300))
        run(e, pairs, ids, clusters, "timing")
        st = e.cluster_index_stats().as_dict()
        assert st["timed_calls"] == 1 and st["kernel_ms"] > 0.0 and st["d2h_bytes"] == 4 * (3 * 300 + 2 + 600)
    finally:
        e.close()
