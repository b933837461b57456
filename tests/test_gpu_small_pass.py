"""GPUDIFF_OPT_SMALL_PASS on the GPU: the fused pass K20 (kcp_amd/csrc/smallpass.hip) gives the ordinary pass's
results byte for byte -- against the oracle and against an engine with the option off -- at every size and
population edge, through its redo paths (arena, deep joins, path count), on a warm consumer, and for everything
downstream that reads the batch's device arrays (path strings, write plans, the object store)."""
import copy
import json
import random

import numpy as np
import pytest

from kcp_amd import gpudiff as G
from tests.golden import fixtures as F
from tests.golden.kat_cases import BASE, J, cases
from tests.parity import assert_matches, oracle_batch
from tests.test_gpu_store import _stream
from tests.workload import deep_pairs, make_pairs

pytestmark = pytest.mark.gpu

ON = G.OPT_SMALL_PASS
ARRAYS = ("pair_flags", "spec_dirty_ids", "status_dirty_ids", "dirty_ids", "path_offsets", "path_hashes", "path_kinds")


def same(a, b):
    for name in ARRAYS:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), name
    return True


def stats(e):
    return e.pass_stats().as_dict()


@pytest.fixture(scope="module")
def on():
    e = G.Engine(device=0, encode_threads=8, small_pass=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def off():
    e = G.Engine(device=0, encode_threads=8)
    yield e
    e.close()


# ---------------------------------------------------------------- 1. KATs and goldens
@pytest.mark.parametrize("dev", [False, True], ids=["host_encode", "device_encode"])
def test_kat_and_golden_fixtures(dev):
    e = G.Engine(device=0, encode_threads=4, small_pass=True, device_encode=dev)
    before = stats(e)
    pairs = [(G.to_json_bytes(a), G.to_json_bytes(b)) for _n, a, b, _se, _st in cases()]
    assert_matches(e.diff_pairs(pairs), pairs)
    for name in ("config1", "config2"):
        fx = F.load(name)
        res = e.diff_pairs([(a, b) for _n, a, b, _e in fx])
        want = np.array([F.expected_flags(x) for *_, x in fx], dtype=np.uint8)
        assert np.array_equal(res.pair_flags & 7, want), name
        dirty = [i for i, (*_, x) in enumerate(fx) if x["spec_dirty"] or x["status_dirty"]]
        assert res.dirty_ids.tolist() == dirty
        for k, p in enumerate(dirty):
            assert res.paths_of(k) == [(h, kd) for h, kd, _s in fx[p][3]["paths"]], fx[p][0]
    after = stats(e)
    assert after["small_passes"] >= before["small_passes"] + 3
    assert after["small_redone"] == 0
    e.close()


# ---------------------------------------------------------------- 2. size edges
@pytest.fixture(scope="module")
def population():
    pairs, cl, _ = make_pairs(4097, seed=7)  # make_pairs(n, 7) is its first n pairs
    return pairs, cl


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096])
def test_size_edges(on, off, population, n):
    pairs, cl = population[0][:n], population[1][:n]
    ids = [1000 + 3 * i for i in range(n)]
    before = stats(on)
    a = on.diff_pairs(pairs, ids=ids, clusters=cl)
    b = off.diff_pairs(pairs, ids=ids, clusters=cl)
    same(a, b)
    after = stats(on)
    assert after["small_passes"] == before["small_passes"] + 1 and after["small_redone"] == before["small_redone"]
    if n <= 257:
        assert_matches(a, pairs, ids=ids)


def test_one_pair_past_the_limit_takes_the_ordinary_pass(on, off, population):
    n = G.SMALL_PASS_MAX_PAIRS + 1
    pairs = population[0][:n]
    before = stats(on)
    same(on.diff_pairs(pairs), off.diff_pairs(pairs))
    after = stats(on)
    assert after["small_passes"] == before["small_passes"] and after["passes"] == before["passes"] + 1


# ---------------------------------------------------------------- 3. population edges (130 pairs: two chunk edges)
def _populations():
    n = 130
    clean, _, _ = make_pairs(n, seed=21, mix=(("deploy", 0.6), ("crd", 0.4)), mutate_frac=0.0)
    alld, _, _ = make_pairs(n, seed=22, mutate_frac=1.0)
    und, _, _ = make_pairs(n, seed=23, mutate_frac=0.3)
    und = [(a, b"{\"spec\": [1, 2") if i % 5 == 0 else (a, b) for i, (a, b) in enumerate(und)]
    cms, _, _ = make_pairs(n, seed=24, mix=(("cm", 0.5), ("secret", 0.5)), mutate_frac=0.0)
    return {"clean": clean, "all_dirty": alld, "empty_objects": [(b"{}", b"{}")] * n, "undecodable": und,
            "sentinel_only": cms}


@pytest.mark.parametrize("name", ["clean", "all_dirty", "empty_objects", "undecodable", "sentinel_only"])
def test_population_edges(on, off, name):
    pairs = _populations()[name]
    before = stats(on)
    res = on.diff_pairs(pairs)
    exp = assert_matches(res, pairs)
    same(res, off.diff_pairs(pairs))
    after = stats(on)
    assert after["small_passes"] == before["small_passes"] + 1 and after["small_redone"] == before["small_redone"]
    nd = sum(1 for r in exp if r["spec_dirty"] or r["status_dirty"])
    if name == "clean":
        assert nd == 0 and res.path_hashes.size == 0
    if name == "empty_objects":  # no "status" key in the new object: status-dirty by the reference's rule, a no-op write
        assert nd == len(pairs) and res.pair_flags.tolist() == [G.STATUS_DIRTY | G.STATUS_NOOP] * nd
    if name == "all_dirty":
        assert nd == len(pairs)
    if name == "undecodable":
        assert sum(1 for r in exp if r["decode_error"]) == 26
    if name == "sentinel_only":
        assert nd == len(pairs) and res.path_kinds.tolist() == [G.PATH_REGION_STATUS | G.PATH_STATUS_ABSENT] * nd


@pytest.mark.parametrize("dev", [False, True], ids=["host_encode", "device_encode"])
@pytest.mark.parametrize("bits", [16, 8])
def test_forced_collisions(bits, dev):
    """16 bits: ConfigMaps and Deployments alone (some 25 paths a pair) collide too rarely for a seed to occur in
    130 pairs, so a fifth of the pairs are CRDs of 200 leaves; 8 bits: test_forced_collisions' population, where
    most pairs are re-seeded, the sentinel-only ones included."""
    mix = (("cm", 0.4), ("deploy", 0.4), ("crd", 0.2)) if bits == 16 else (("cm", 0.5), ("deploy", 0.5))
    pairs, _, _ = make_pairs(130, seed=5, mix=mix, mutate_frac=0.5)
    e = G.Engine(device=0, path_hash_bits=bits, device_encode=dev, small_pass=True)
    res = e.diff_pairs(pairs)
    exp = assert_matches(res, pairs, hash_bits=bits)
    n_seeded = sum(1 for r in exp if r["seed"])
    print("pairs with a non-zero seed:", n_seeded)
    assert n_seeded >= 1  # the kernel's F_SEED / seeded-sentinel path ran
    st = stats(e)
    assert st["small_passes"] >= 1 and st["small_redone"] == 0
    e.close()


# ---------------------------------------------------------------- 4. long values and list shifts
def test_long_values_and_list_shift(on, off):
    rnd = random.Random(4)
    pairs = []
    for i in range(200):
        a = json.loads(J(BASE))
        a["spec"]["blob"] = "".join(rnd.choice("ab") for _ in range(rnd.randint(9, 300)))
        a["spec"]["items"] = ["item-%03d-%s" % (k, "x" * rnd.randint(0, 40)) for k in range(rnd.randint(60, 200))]
        b = json.loads(json.dumps(a))
        c = i % 4
        if c == 0:
            b["spec"]["blob"] = b["spec"]["blob"][:-1] + ("a" if b["spec"]["blob"][-1] == "b" else "b")
        elif c == 1:
            del b["spec"]["items"][len(b["spec"]["items"]) // 2]
        elif c == 2:
            b["spec"]["items"].insert(3, "new")
        pairs.append((J(a), J(b)))
    before = stats(on)
    res = on.diff_pairs(pairs)
    assert_matches(res, pairs)
    same(res, off.diff_pairs(pairs))
    after = stats(on)
    assert after["small_passes"] == before["small_passes"] + 1 and after["small_redone"] == before["small_redone"]


# ---------------------------------------------------------------- 5. deep joins: the redo path is exact
def test_deep_joins_are_redone(on):
    pairs = deep_pairs()
    before = stats(on)
    res = on.diff_pairs(pairs)
    assert_matches(res, pairs)
    after = stats(on)
    assert after["redo_deep"] >= before["redo_deep"] + 1
    assert after["small_redone"] == before["small_redone"] + 1


# ---------------------------------------------------------------- 6. redo by arena
@pytest.fixture(scope="module")
def arena_case():
    pairs, _, _ = make_pairs(300, seed=14, mutate_frac=0.4, crd_leaves=300, pretty_frac=0)
    return pairs, oracle_batch(pairs)


@pytest.mark.parametrize("shrink", [10, 14])
def test_arena_redo(arena_case, shrink):
    pairs, exp = arena_case
    e = G.Engine(device=0, flags=(shrink << G.OPT_ARENA_SHIFT) | ON)
    res = e.diff_pairs(pairs)
    assert_matches(res, pairs, exp=exp)
    st = stats(e)
    print("shrink", shrink, st)
    assert st["small_passes"] == 1
    if shrink == 14:
        assert st["redo_arena"] >= 1 and st["small_redone"] == 1
    e.close()


# ---------------------------------------------------------------- 7. redo by path count, the second read-back round
# The issue sketches maps of 1000 leaves; a pair's join then covers 2 x (1000 + the base object's leaves) keys, more
# than one wave takes (the deep-join limit of 2048), and the pass would be redone for that reason instead.  900
# leaves keep every join under the limit; the pair count follows from the header's constants.
LEAVES = 900


def _map_pairs(n, n_changed):
    rnd = random.Random(77)
    pairs = []
    for i in range(n):
        a = json.loads(J(BASE))
        a["spec"]["m"] = {"k%04d" % k: rnd.randint(0, 1 << 40) for k in range(LEAVES)}
        b = copy.deepcopy(a)
        if i < n_changed:
            b["spec"]["m"] = {k: v + 1 for k, v in b["spec"]["m"].items()}
        pairs.append((J(a), J(b)))
    return pairs


def test_path_count_redo_and_readback_rounds(on):
    n = G.SMALL_PASS_MAX_PATHS // LEAVES + 1
    n += n % 2
    half = n // 2
    assert half * LEAVES <= G.SMALL_PASS_MAX_PATHS < n * LEAVES  # finalised / over the limit
    assert half * LEAVES > max(64, 4 * n)                         # over the first read-back round's budget
    # half the pairs changed: finalised, two rounds
    pairs = _map_pairs(n, half)
    before = stats(on)
    res = on.diff_pairs(pairs)
    after = stats(on)
    assert res.path_hashes.size == half * LEAVES
    assert_matches(res, pairs)
    assert after["readback_rounds"] == before["readback_rounds"] + 2
    assert after["small_redone"] == before["small_redone"] and after["small_passes"] == before["small_passes"] + 1
    # every pair changed: over GPUDIFF_SMALL_PASS_MAX_PATHS, redone
    pairs = _map_pairs(n, n)
    before = stats(on)
    res = on.diff_pairs(pairs)
    after = stats(on)
    assert res.path_hashes.size == n * LEAVES
    assert_matches(res, pairs)
    assert after["redo_paths"] == before["redo_paths"] + 1 and after["small_redone"] == before["small_redone"] + 1
    # a 100-pair batch, one changed leaf per dirty pair: one round
    pairs = []
    for i in range(100):
        a = json.loads(J(BASE))
        a["spec"]["replicas"] = 3
        b = copy.deepcopy(a)
        if i % 3 == 0:
            b["spec"]["replicas"] = 4 + i
        pairs.append((J(a), J(b)))
    before = stats(on)
    res = on.diff_pairs(pairs)
    after = stats(on)
    exp = assert_matches(res, pairs)
    assert all(len(r["paths"]) == 1 for r in exp if r["spec_dirty"]) and res.path_hashes.size == 34
    assert after["readback_rounds"] == before["readback_rounds"] + 1
    assert after["small_redone"] == before["small_redone"]


# ---------------------------------------------------------------- 8. warm consumer
@pytest.mark.parametrize("n", [8, 1024])
def test_warm_consumer_alternating_populations(on, off, n):
    """One batch reset and refilled 16 times with two populations of identical shapes whose dirty sets are
    complementary: a finishing block that read a stale line of the previous pass (flags, counts, arena entries)
    would report the other population's pairs."""
    base = []
    for i in range(n):
        a = json.loads(J(BASE))
        a["spec"]["replicas"] = 100 + i
        a["spec"]["note"] = "pair-%05d-" % i + "x" * (i % 23)
        base.append(a)

    def population(parity):
        out = []
        for i, a in enumerate(base):
            b = copy.deepcopy(a)
            if i % 2 == parity:
                b["spec"]["replicas"] = 5000 + i           # an int for an int: the blobs keep their shape
                b["spec"]["note"] = a["spec"]["note"][::-1]  # same length
            out.append((J(a), J(b)))
        return out

    pops = [population(0), population(1)]
    want = [off.diff_pairs(p) for p in pops]
    assert want[0].dirty_ids.tolist() == list(range(0, n, 2)) and want[1].dirty_ids.tolist() == list(range(1, n, 2))
    if n == 8:
        for p, w in zip(pops, want):
            assert_matches(w, p)
    hbs = [on.encode(p) for p in pops]
    assert hbs[0].info().pool_bytes == hbs[1].info().pool_bytes
    db = on.device_batch(hbs[0].info().pool_bytes + 4096, n)
    before = stats(on)
    for it in range(16):
        db.reset()
        db.append(hbs[it % 2])
        same(on.wait(on.diff(db)), want[it % 2])
    after = stats(on)
    assert after["small_passes"] == before["small_passes"] + 16 and after["small_redone"] == before["small_redone"]
    db.free()
    for hb in hbs:
        hb.free()


# ---------------------------------------------------------------- 9. downstream readers of the device arrays
def _plan_tuple(wp):
    return (wp.pair_index.tolist(), wp.kind.tolist(), wp.noop.tolist(), wp.bodies, wp.source.tolist(), wp.n_host)


def test_downstream_readers_see_the_same_device_arrays():
    flags = G.OPT_DEVICE_ENCODE | G.OPT_PATH_STRINGS
    got = []
    for opt in (ON, 0):
        e = G.Engine(device=0, encode_threads=4, flags=flags | opt)
        st = e.object_store(max_slots=20, space_bytes=32 << 20, max_events=64, device_encode=True)
        out = []
        for evs, pairs in _stream(3, 20, 3, 50):
            t = st.submit([(s, nj, oj, i, s % 7) for i, (s, nj, oj) in enumerate(evs)])
            res = e.wait(t)
            if opt:
                assert_matches(res, pairs)
            out.append((res, res.path_strings, _plan_tuple(st.write_plan(t))))
        pairs, _, _ = make_pairs(100, seed=31, mutate_frac=0.5)
        t = e.submit(pairs)
        res = e.wait(t)
        if opt:
            assert_matches(res, pairs)
        out.append((res, res.path_strings, _plan_tuple(e.write_plan(t))))
        ps = stats(e)
        assert (ps["small_passes"] >= 4) if opt else (ps["small_passes"] == 0)
        got.append(out)
        st.free()
        e.close()
    for (ra, sa, pa), (rb, sb, pb) in zip(*got):
        same(ra, rb)
        assert sa is not None and sa == sb
        assert pa == pb
    assert sum(len(s) for _r, s, _p in got[0]) > 50 and sum(len(p[0]) for _r, _s, p in got[0]) > 20


# ---------------------------------------------------------------- 10. drop-ins and timing
@pytest.mark.parametrize("dev", [False, True], ids=["host_encode", "device_encode"])
def test_single_pair_dropins_and_timing(dev):
    e = G.Engine(device=0, encode_threads=2, timing=True, device_encode=dev, small_pass=True)
    a = json.loads(J(BASE))
    b = copy.deepcopy(a)
    assert e.spec_equal(a, b) and e.status_equal(a, b)
    b["spec"]["replicas"] = 99
    assert not e.spec_equal(a, b) and e.status_equal(a, b)
    c = copy.deepcopy(a)
    c["status"] = {"readyReplicas": 7}
    assert e.spec_equal(a, c) and not e.status_equal(a, c)
    st = stats(e)
    assert st["passes"] == 6 and st["small_passes"] == 6 and st["small_redone"] == 0
    assert st["readback_rounds"] == 6  # one host synchronisation per pass (the ordinary pass takes two)
    t = e.timings()
    print("timings", t.compare_ms, t.compact_ms, t.join_ms, t.emit_ms, t.total_ms, t.n_passes)
    assert t.n_passes == 6 and t.compare_ms > 0 and t.total_ms >= t.compare_ms
    # the whole kernel lies between the first two events; nothing is enqueued between the other four, so what
    # separates them is the cost of recording an event (a few microseconds), far below any launch chain
    assert max(t.compact_ms, t.join_ms, t.emit_ms) < 0.02
    e.close()
