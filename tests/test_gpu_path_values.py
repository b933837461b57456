"""GPUDIFF_OPT_PATH_VALUES on the GPU: kernels K21 / K22 (kcp_amd/csrc/values.hip) render, for every changed path of
a device-encoded batch, A's and B's leaf as JSON text from the segments in HBM; the events K0 defers get theirs from
the resolution batch by the same kernels; the values ride with the result (gpudiff_result_path_values).  Every
comparison is exact equality with the model (tests/path_values_model.py), in result order."""
import ctypes as C
import functools

import numpy as np
import pytest

from kcp_amd import gpudiff as G
from tests import path_values_cases as VC
from tests import path_values_model as M
from tests.golden import fixtures as F
from tests.golden.kat_cases import cases as kat_cases
from tests.parity import assert_matches, oracle_batch
from tests.test_gpu_path_strings import _items, _one_path_pair, _stream

pytestmark = pytest.mark.gpu

ON = G.OPT_DEVICE_ENCODE | G.OPT_PATH_VALUES
BOTH = G.OPT_PATH_STRINGS | G.OPT_PATH_VALUES


def _check_values(res, pairs, exp, hash_bits=32):
    """exp: the oracle's per-pair results (what tests.parity.assert_matches returns).  Returns the entries per pair."""
    assert res.path_values is not None and len(res.path_values) == len(res.path_hashes)
    assert res.values_unresolved == 0
    dirty = [i for i, r in enumerate(exp) if r["spec_dirty"] or r["status_dirty"]]
    assert len(dirty) == len(res.dirty_ids)
    for k, p in enumerate(dirty):
        a, b = G.to_json_bytes(pairs[p][0]), G.to_json_bytes(pairs[p][1])
        want = [] if exp[p]["decode_error"] else M.values_of(a, b, r=exp[p], hash_bits=hash_bits)
        got = res.changed_values_of(k)
        assert got == want, "values differ for pair %d:\n got %s\nwant %s" % (
            p, [g for g, w in zip(got, want) if g != w][:3], [w for g, w in zip(got, want) if g != w][:3])
    for ot, o, nt, nw in res.path_values:  # a present text is never empty, an absent one is None
        assert (o is None) == (ot == G.VALUE_ABSENT) and (nw is None) == (nt == G.VALUE_ABSENT)
        assert o != b"" and nw != b""
    return {p: len(exp[p]["paths"]) for p in dirty}


def _k0_deferred(eng, pairs):
    """The pairs K0 leaves to the host: a document of theirs is outside its exact subset (its own status says so)."""
    docs = [G.to_json_bytes(d) for ab in pairs for d in ab]
    st = [info["status"] for info, _blob in eng.encode_objects(docs)]
    return [i for i in range(len(pairs)) if st[2 * i] != G.TOK_OK or st[2 * i + 1] != G.TOK_OK]


# ---------------------------------------------------------------- 1. KAT cases and golden fixtures, pair mode
@pytest.mark.parametrize("name", F.NAMES)
def test_fixtures_pair_mode(name):
    pairs = [(a, b) for _n, a, b, _e in F.load(name)]
    eng = G.Engine(device=0, encode_threads=4, flags=ON)
    res = eng.wait(eng.submit(pairs))
    per_pair = _check_values(res, pairs, assert_matches(res, pairs))
    deferred = _k0_deferred(eng, pairs)
    assert eng.submit_stats().deferred == len(deferred)
    assert res.values_host == sum(per_pair.get(p, 0) for p in deferred)
    if name != "manifests":  # (the reference's manifests hold a few floats / keys K0 leaves to the host)
        assert deferred == [] and res.values_host == 0  # every value came from K21 / K22 over K0's blobs
    assert eng.path_values_stats().paths == len(res.path_values) > 0
    eng.close()


def test_kat_cases_pair_mode():
    pairs = [(G.to_json_bytes(a), G.to_json_bytes(b)) for _n, a, b, _se, _st in kat_cases()]
    eng = G.Engine(device=0, encode_threads=4, flags=ON)
    res = eng.wait(eng.submit(pairs))
    exp = assert_matches(res, pairs)
    per_pair = _check_values(res, pairs, exp)
    assert any(r["decode_error"] for r in exp)  # no values for those
    deferred = _k0_deferred(eng, pairs)
    assert eng.submit_stats().deferred == len(deferred) > 0  # the designed deferrals: the host-resolved path
    assert res.values_host == sum(per_pair.get(p, 0) for p in deferred) > 0
    eng.close()


# ---------------------------------------------------------------- 2. the edge cases, pair mode
def test_edge_cases_on_the_device():
    pairs = [(a, b) for _n, a, b in VC.DEVICE_CASES]
    pairs += [(b, a) for _n, a, b in VC.DEVICE_CASES]  # and backwards: ADDED <-> REMOVED, the other side's arena
    eng = G.Engine(device=0, encode_threads=2, flags=ON)
    res = eng.wait(eng.submit(pairs))
    _check_values(res, pairs, assert_matches(res, pairs))
    assert res.values_host == 0 and eng.submit_stats().deferred == 0  # inside K0's exact subset
    texts = {t for ot, o, nt, nw in res.path_values for t in (o, nw)}
    for want in (b"null", b"[]", b"-9223372036854775808", b"1e+21", b"123456789012345680000", b"0.000001", b"1e-7",
                 b'""', b'"aaaaaa\\u2028z"', b'"aaaaaaa\\u2029z"', b'"aaaaaaaa\\u0001zz"'):
        assert want in texts, want
    assert (G.TAG_INT, b"3", G.TAG_FLOAT, b"3") in res.path_values
    assert max(len(t) for t in texts if t) == 70002
    eng.close()


@pytest.mark.parametrize("name,a,b", VC.HOST_CASES, ids=[c[0] for c in VC.HOST_CASES])
def test_edge_cases_the_host_resolves(name, a, b):
    pairs = [(a, b), (b, a)]
    eng = G.Engine(device=0, encode_threads=2, flags=ON)
    res = eng.wait(eng.submit(pairs))
    _check_values(res, pairs, assert_matches(res, pairs))
    assert eng.submit_stats().deferred == 2
    assert res.values_host == len(res.path_values) > 0
    eng.close()


# ---------------------------------------------------------------- 3. the store
@pytest.mark.parametrize("drop_old", [False, True], ids=["old_json", "no_old_json"])
def test_store_replay_with_chains(drop_old):
    eng = G.Engine(device=0, encode_threads=4, flags=BOTH)
    st = eng.object_store(max_slots=60, space_bytes=64 << 20, max_events=256, device_encode=True)
    n_paths = n_host = 0
    for evs, pairs in _stream(1, 60, 3, 150):
        res = eng.wait(st.submit(_items(evs, drop_old)))
        _check_values(res, pairs, assert_matches(res, pairs))
        assert res.values_host == res.paths_host  # the entries of the events the host resolved, for both renderers
        n_paths += len(res.path_values)
        n_host += res.values_host
    assert n_paths > 100
    vs = eng.path_values_stats()
    assert vs.batches == 3 and vs.paths == n_paths and vs.host_paths == n_host
    st.free()
    eng.close()


def test_compaction_with_two_submits_in_flight():
    """tests/test_gpu_path_strings.py's schedule with only the values on: they are rendered at gpudiff_wait from the
    space the batch was written to, after a later submit's compaction and before the batch's own resolution."""
    eng = G.Engine(device=0, encode_threads=4, flags=G.OPT_PATH_VALUES)
    st = eng.object_store(max_slots=40, space_bytes=512 << 10, max_events=128, device_encode=True)
    stream = _stream(2, 40, 12, 60)
    for t in range(0, len(stream), 2):
        t0 = st.submit(_items(stream[t][0]))
        t1 = st.submit(_items(stream[t + 1][0]))
        for ticket, (_evs, pairs) in ((t0, stream[t]), (t1, stream[t + 1])):
            res = eng.wait(ticket)
            _check_values(res, pairs, assert_matches(res, pairs))
    assert st.stats().compactions >= 3, st.stats().compactions
    st.free()
    eng.close()


# ---------------------------------------------------------------- 4. forced collisions
def test_forced_collisions_16_bits():
    eng = G.Engine(device=0, encode_threads=4, path_hash_bits=16, flags=BOTH)
    st = eng.object_store(max_slots=40, space_bytes=64 << 20, max_events=256, device_encode=True)
    n_host = 0
    for evs, pairs in _stream(9, 40, 4, 120):
        res = eng.wait(st.submit(_items(evs)))
        _check_values(res, pairs, assert_matches(res, pairs, hash_bits=16), hash_bits=16)
        assert res.values_host == res.paths_host
        n_host += res.values_host
    s = st.stats()
    assert s.reseeded > 0 and s.collisions_unresolved == 0 and n_host > 0
    st.free()
    eng.close()


# ---------------------------------------------------------------- 5. text counts at the scan's edges
_EDGE_MAX = 1025


@functools.lru_cache(maxsize=None)
def _edge_pairs():
    """The pairs and the oracle's results, computed once for every case below (a case takes a prefix)."""
    pairs = [_one_path_pair(i) for i in range(_EDGE_MAX)]
    return pairs, oracle_batch(pairs)


@pytest.mark.parametrize("n", [1, 511, 512, 513, 1024, 1025])
def test_path_counts_at_scan_edges(n):
    """2n texts with 2n at the scan tile's edges (scan64: tiles of 1024)."""
    pairs, exp = _edge_pairs()
    pairs, exp = pairs[:n], exp[:n]
    eng = G.Engine(device=0, encode_threads=4, flags=ON)
    res = eng.wait(eng.submit(pairs))
    _check_values(res, pairs, assert_matches(res, pairs, exp=exp))
    assert len(res.path_values) == n and res.values_host == 0
    assert res.path_values[n - 1][3] == b'"' + b"a" * ((n - 1) % 13) + b'x"'
    eng.close()


# ---------------------------------------------------------------- 6. options
def _raw_wait(eng, ticket):
    """(rc of gpudiff_result_path_values, n_paths, offsets[0]) of a waited ticket."""
    r = G.Result()
    assert G.lib().gpudiff_wait(eng.ctx, ticket, C.byref(r)) == G.OK
    pv = G.PathValuesC()
    rc = G.lib().gpudiff_result_path_values(eng.ctx, C.byref(r), C.byref(pv))
    first = C.cast(pv.offsets, C.POINTER(C.c_uint64))[0] if rc == G.OK else None
    n = pv.n_paths
    G.lib().gpudiff_result_release(eng.ctx, C.byref(r))
    return rc, n, first


@functools.lru_cache(maxsize=None)
def _option_pairs():
    return [(a, b) for _n, a, b, _e in F.load("manifests")[:80]]


def test_strings_and_values_together():
    pairs = _option_pairs()
    got = {}
    for flags in (G.OPT_PATH_STRINGS, G.OPT_PATH_VALUES, BOTH):
        eng = G.Engine(device=0, encode_threads=2, flags=G.OPT_DEVICE_ENCODE | flags)
        res = eng.wait(eng.submit(pairs))
        exp = assert_matches(res, pairs)
        assert (res.path_strings is not None) == bool(flags & G.OPT_PATH_STRINGS)
        assert (res.path_values is not None) == bool(flags & G.OPT_PATH_VALUES)
        if flags & G.OPT_PATH_VALUES:
            _check_values(res, pairs, exp)
        # one sizing read-back and one final one per rendered batch, for one renderer or both
        # (and the same two for the resolution batch's values, when the deferred events have changed paths)
        n_resolved = 1 if (flags & G.OPT_PATH_VALUES) and res.values_host else 0
        assert eng.render_syncs() == 2 + 2 * n_resolved
        got[flags] = res
        eng.close()
    assert got[BOTH].path_strings == got[G.OPT_PATH_STRINGS].path_strings
    assert got[BOTH].paths_host == got[G.OPT_PATH_STRINGS].paths_host
    assert got[BOTH].path_values == got[G.OPT_PATH_VALUES].path_values
    assert got[BOTH].values_host == got[G.OPT_PATH_VALUES].values_host == got[BOTH].paths_host


def test_small_pass_at_40_pairs():
    pairs = _option_pairs()[:40]
    eng = G.Engine(device=0, encode_threads=2, flags=ON | G.OPT_SMALL_PASS | G.OPT_PATH_STRINGS)
    res = eng.wait(eng.submit(pairs))
    _check_values(res, pairs, assert_matches(res, pairs))
    assert eng.pass_stats().small_passes >= 1
    ref = G.Engine(device=0, encode_threads=2, flags=G.OPT_DEVICE_ENCODE | G.OPT_PATH_STRINGS)
    assert res.path_strings == ref.wait(ref.submit(pairs)).path_strings
    ref.close()
    eng.close()


def test_option_off_and_host_encoded_batches():
    pairs = _option_pairs()
    eng = G.Engine(device=0, encode_threads=2, flags=G.OPT_DEVICE_ENCODE | G.OPT_PATH_STRINGS)
    res = eng.wait(eng.submit(pairs))
    assert res.path_values is None and res.path_strings is not None
    assert _raw_wait(eng, eng.submit(pairs))[0] == G.E_STATE  # the option was off
    vs = eng.path_values_stats()
    assert (vs.batches, vs.paths, vs.bytes, vs.host_paths, vs.kernel_ms, vs.timed_batches) == (0, 0, 0, 0, 0.0, 0)
    eng.close()
    on = G.Engine(device=0, encode_threads=2, flags=ON)
    res_on = on.wait(on.submit(pairs))
    for f in ("pair_flags", "spec_dirty_ids", "status_dirty_ids", "dirty_ids", "path_offsets", "path_hashes",
              "path_kinds"):
        assert np.array_equal(getattr(res, f), getattr(res_on, f)), f
    on.close()
    # a host-encoded batch is out of scope, with the option on too; so is a host-encode store
    eng = G.Engine(device=0, encode_threads=2, flags=G.OPT_PATH_VALUES)
    assert _raw_wait(eng, eng.submit(pairs))[0] == G.E_STATE
    st = eng.object_store(max_slots=8, space_bytes=1 << 20, max_events=16, device_encode=False)
    assert _raw_wait(eng, st.submit([(0, pairs[0][1], pairs[0][0], 0, 0)]))[0] == G.E_STATE
    assert eng.path_values_stats().batches == 0
    st.free()
    eng.close()


def test_no_dirty_pair_has_no_values():
    """No changed path: nothing to scan; n_paths == 0 and offsets == [0] come back (the option is on)."""
    pairs = [(_one_path_pair(i)[0],) * 2 for i in range(5)]
    eng = G.Engine(device=0, encode_threads=2, flags=ON)
    assert _raw_wait(eng, eng.submit(pairs)) == (G.OK, 0, 0)
    res = eng.wait(eng.submit(pairs))
    _check_values(res, pairs, assert_matches(res, pairs))
    assert len(res.dirty_ids) == 0 and res.path_values == []
    vs = eng.path_values_stats()
    assert vs.batches == 2 and vs.paths == 0 and vs.bytes == 0
    eng.close()


# ---------------------------------------------------------------- 7. timing
def test_timing_counts_kernel_time():
    pairs = _option_pairs()
    eng = G.Engine(device=0, encode_threads=2, flags=ON | G.OPT_TIMING)
    res = eng.wait(eng.submit(pairs))
    _check_values(res, pairs, assert_matches(res, pairs))
    vs = eng.path_values_stats()
    assert vs.kernel_ms > 0 and vs.timed_batches == 1 and vs.batches == 1
    assert vs.bytes == sum(len(t) for ot, o, nt, nw in res.path_values for t in (o, nw) if t is not None)
    eng.close()
