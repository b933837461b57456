"""GPUDIFF_OPT_PATH_STRINGS on the GPU: kernels K15 / K16 (kcp_amd/csrc/paths.hip) render every changed path of a
device-encoded batch from the path tables in HBM, the host resolution renders the events K0 defers, and the
strings ride with the result (gpudiff_result_path_strings).  Every comparison is exact byte equality with the
golden fixtures' third column or the oracle's render_path, in result order."""
import copy
import ctypes as C
import functools
import json
import random

import numpy as np
import pytest

from kcp_amd import gpudiff as G
from oracle import gpudiff_oracle as O
from tests import path_strings_cases as PC
from tests.golden import fixtures as F
from tests.golden.kat_cases import cases as kat_cases
from tests.parity import assert_matches, oracle_batch
from tests.workload import _noise, configmap, crd, deployment, mutate

pytestmark = pytest.mark.gpu

ON = G.OPT_DEVICE_ENCODE | G.OPT_PATH_STRINGS


def _want(r):
    """The oracle's (hash, kind, text) list of one pair."""
    return [(h, k | (G.PATH_REGION_STATUS if region else 0), O.render_path(p).encode("utf-8"))
            for (h, region, k, p) in r["paths"]]


def _got(res, k):
    b, e = int(res.path_offsets[k]), int(res.path_offsets[k + 1])
    return list(zip(res.path_hashes[b:e].tolist(), res.path_kinds[b:e].tolist(), res.path_strings[b:e]))


def _check_strings(res, exp):
    """exp: the oracle's per-pair results (what tests.parity.assert_matches returns)."""
    assert res.path_strings is not None and len(res.path_strings) == len(res.path_hashes)
    assert res.paths_unresolved == 0
    dirty = [i for i, r in enumerate(exp) if r["spec_dirty"] or r["status_dirty"]]
    assert len(dirty) == len(res.dirty_ids)
    for k, p in enumerate(dirty):
        assert _got(res, k) == _want(exp[p]), "strings differ for pair %d" % p
        if exp[p]["decode_error"]:
            assert _got(res, k) == []


# ---------------------------------------------------------------- 1. fixtures, pair mode
@pytest.mark.parametrize("name", F.NAMES)
def test_fixtures_pair_mode(name):
    pairs = F.load(name)
    eng = G.Engine(device=0, encode_threads=4, flags=ON)
    res = eng.wait(eng.submit([(a, b) for _n, a, b, _e in pairs]))
    assert res.path_strings is not None and res.paths_unresolved == 0
    dirty = [i for i, (*_, e) in enumerate(pairs) if e["spec_dirty"] or e["status_dirty"]]
    assert res.dirty_ids.tolist() == dirty
    for k, p in enumerate(dirty):
        want = [(h, kd, s.encode("utf-8")) for h, kd, s in pairs[p][3]["paths"]]
        assert _got(res, k) == want, pairs[p][0]
        assert res.rendered_paths_of(k) == [(h, kd, s) for h, kd, s in pairs[p][3]["paths"]]
    deferred = eng.submit_stats().deferred
    if name == "manifests":  # the reference's manifests hold a few floats / keys K0 leaves to the host
        assert deferred <= 0.2 * len(pairs)
    else:  # every string came from K15 / K16
        assert deferred == 0 and res.paths_host == 0
    eng.close()


# ---------------------------------------------------------------- 2. KAT cases, pair mode
def test_kat_cases_pair_mode():
    pairs = [(G.to_json_bytes(a), G.to_json_bytes(b)) for _n, a, b, _se, _st in kat_cases()]
    eng = G.Engine(device=0, encode_threads=4, flags=ON)
    res = eng.wait(eng.submit(pairs))
    exp = assert_matches(res, pairs)
    _check_strings(res, exp)
    assert any(r["decode_error"] for r in exp)  # no strings for those (_check_strings)
    assert eng.submit_stats().deferred > 0      # the designed deferrals went through the host's renderer
    eng.close()


# ---------------------------------------------------------------- 3.-5. the store
def _obj(rnd, i):
    k = rnd.random()
    if k < 0.3:
        return configmap(rnd, i, i % 7)
    if k < 0.45:
        return configmap(rnd, i, i % 7, True)
    if k < 0.8:
        return deployment(rnd, i, i % 7)
    return crd(rnd, i, i % 7, 60)


def _next_version(rnd, o):
    o = _noise(rnd, copy.deepcopy(o))
    if "status" not in o and o.get("kind") not in ("ConfigMap", "Secret"):
        o["status"] = {"readyReplicas": 1, "conditions": [{"type": "Ready", "status": "True"}]}
        return o
    c = rnd.random()
    if c < 0.45:
        return o
    if c < 0.9:
        return mutate(rnd, o)
    if c < 0.95 and "status" in o:
        del o["status"]
        return o
    o.setdefault("spec", {})["extra"] = [1, 2, {"x": None}]
    return o


def _stream(seed, n_slots, n_batches, per_batch):
    """[(batch events [(slot, new_json, old_json)], expected pairs [(old, new)])]: an event's old side is the
    slot's previous version, inside the batch too (tests/test_gpu_store.py's generator)."""
    rnd = random.Random(seed)
    cur = {}
    out = []
    for _b in range(n_batches):
        evs, pairs = [], []
        for _ in range(per_batch):
            s = rnd.randrange(n_slots)
            old = cur.get(s)
            new = _obj(rnd, s) if old is None else _next_version(rnd, old)
            nj = json.dumps(new, separators=(",", ":")).encode()
            oj = json.dumps(old, separators=(",", ":")).encode() if old is not None else None
            evs.append((s, nj, oj))
            pairs.append((oj if oj is not None else b"{}", nj))
            cur[s] = new
        out.append((evs, pairs))
    return out


def _items(evs, drop_old=False):
    return [(s, nj, None if drop_old else oj, i, s % 7) for i, (s, nj, oj) in enumerate(evs)]


@pytest.mark.parametrize("drop_old", [False, True], ids=["old_json", "no_old_json"])
def test_store_replay_with_chains(drop_old):
    eng = G.Engine(device=0, encode_threads=4, flags=G.OPT_PATH_STRINGS)
    st = eng.object_store(max_slots=60, space_bytes=64 << 20, max_events=256, device_encode=True)
    n_paths = 0
    for evs, pairs in _stream(1, 60, 3, 150):
        res = eng.wait(st.submit(_items(evs, drop_old)))
        _check_strings(res, assert_matches(res, pairs))
        n_paths += len(res.path_strings)
    assert n_paths > 100
    ps = eng.path_stats()
    assert ps.batches == 3 and ps.paths == n_paths
    st.free()
    eng.close()


def test_compaction_with_two_submits_in_flight():
    """The lifetime hazard: the strings are rendered at gpudiff_wait, after a later submit's compaction may have
    moved the live blobs and before the batch's own host resolution may compact again.  A wrong answer shows as
    wrong text, not as a fault: both spaces stay allocated."""
    eng = G.Engine(device=0, encode_threads=4, flags=G.OPT_PATH_STRINGS)
    st = eng.object_store(max_slots=40, space_bytes=512 << 10, max_events=128, device_encode=True)
    stream = _stream(2, 40, 12, 60)
    for t in range(0, len(stream), 2):
        t0 = st.submit(_items(stream[t][0]))
        t1 = st.submit(_items(stream[t + 1][0]))
        for ticket, (_evs, pairs) in ((t0, stream[t]), (t1, stream[t + 1])):
            res = eng.wait(ticket)
            _check_strings(res, assert_matches(res, pairs))
    assert st.stats().compactions >= 3, st.stats().compactions
    st.free()
    eng.close()


def test_forced_collisions_16_bits():
    eng = G.Engine(device=0, encode_threads=4, path_hash_bits=16, flags=G.OPT_PATH_STRINGS)
    st = eng.object_store(max_slots=40, space_bytes=64 << 20, max_events=256, device_encode=True)
    n_host = 0
    for evs, pairs in _stream(9, 40, 4, 120):
        res = eng.wait(st.submit(_items(evs)))
        _check_strings(res, assert_matches(res, pairs, hash_bits=16))
        n_host += res.paths_host
    s = st.stats()
    assert s.reseeded > 0 and s.collisions_unresolved == 0 and n_host > 0
    st.free()
    eng.close()


# ---------------------------------------------------------------- 6. edge keys, pair mode
def test_edge_keys_pair_mode():
    eng = G.Engine(device=0, encode_threads=2, flags=ON)
    docs = dict(PC.EDGE_DOCS)
    pairs = []
    for _name, doc in PC.EDGE_DOCS:
        pairs += [(doc, PC.mutate_edge(doc)), (PC.mutate_edge(doc), doc), (b"{}", doc), (doc, b"{}")]
    res = eng.wait(eng.submit(pairs))
    _check_strings(res, assert_matches(res, pairs))
    assert res.paths_host > 0  # the non-ASCII-key documents (TOK_KEY) are the host's
    texts = set(res.path_strings)
    for want in (b"a", b"x.", b"", b"spec..", b"spec.[0]", b"[1].", b"spec.items_[1023]", "spec.é.日".encode()):
        assert want in texts, want
    # ... and the ASCII edge documents alone stay on the device: every string from K15 / K16
    plain = [(docs[n], PC.mutate_edge(docs[n])) for n in ("odd-keys", "long-key", "empty-head", "empty-only",
                                                           "empty-list", "deep-40", "labels")]
    plain += [(docs["list-1024"], b"{}"), (b"{}", docs["list-1024"])]
    d0 = eng.submit_stats().deferred
    res = eng.wait(eng.submit(plain))
    _check_strings(res, assert_matches(res, plain))
    assert res.paths_host == 0 and eng.submit_stats().deferred == d0
    for want in (b"a", b"x.", b"", b"spec..", b"[1].", b"spec.items_[1023]", ("spec." + PC.LONG_KEY + ".x[1]").encode()):
        assert want in set(res.path_strings), want
    eng.close()


def test_non_ascii_keys():
    """K0 leaves every key with a byte >= 0x80 to the host, written raw or escaped (TOK_KEY; tests/test_gpu_tokenize.py
    pins both), so in pair mode both documents' strings are the host renderer's.  Raw UTF-8 key bytes reach K15 / K16
    through the store: the host-resolved version becomes resident with its table, and an ASCII successor that drops
    those paths has them rendered from that table on the device."""
    docs = dict(PC.EDGE_DOCS)
    eng = G.Engine(device=0, encode_threads=2, flags=ON)
    d0 = 0  # (gpudiff_submit_stats_get is E_STATE before the first submit)
    for name in ("utf8-raw", "utf8-escaped"):
        pairs = [(docs[name], PC.mutate_edge(docs[name])), (b"{}", docs[name])]
        res = eng.wait(eng.submit(pairs))
        _check_strings(res, assert_matches(res, pairs))
        assert eng.submit_stats().deferred - d0 == 2 and res.paths_host == len(res.path_strings) > 0
        d0 += 2
        assert "spec.é.日".encode() in set(res.path_strings)
    eng.close()
    eng = G.Engine(device=0, encode_threads=2, flags=G.OPT_PATH_STRINGS)
    st = eng.object_store(max_slots=4, space_bytes=1 << 20, max_events=8, device_encode=True)
    res = eng.wait(st.submit([(0, docs["utf8-raw"], None, 0, 0)]))
    _check_strings(res, assert_matches(res, [(b"{}", docs["utf8-raw"])]))
    assert res.paths_host == len(res.path_strings) > 0
    nxt = b'{"spec":{"plain":1}}'
    res = eng.wait(st.submit([(0, nxt, None, 0, 0)]))
    _check_strings(res, assert_matches(res, [(docs["utf8-raw"], nxt)]))
    assert res.paths_host == 0 and st.stats().deferred == 1
    assert {"spec.é.日".encode(), "spec.café[0]".encode(), b"spec.plain"} <= set(res.path_strings)
    st.free()
    eng.close()


# ---------------------------------------------------------------- 7. path counts at the scan's edges
_EDGE_MAX = 2049


def _one_path_pair(i):
    """A ConfigMap-style pair whose one changed path is data.key-<i> (its status is there and unchanged, so no
    `status` sentinel joins it); the key's and the names' lengths vary, so no two neighbouring offsets repeat."""
    a = {"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": "cm-%d" % i},
         "data": {"key-%d" % i: "a" * (i % 13)}, "status": {"ok": True}}
    b = copy.deepcopy(a)
    b["data"]["key-%d" % i] += "x"
    return G.to_json_bytes(a), G.to_json_bytes(b)


@functools.lru_cache(maxsize=None)
def _edge_pairs():
    """The pairs and the oracle's results, computed once for every case below (a case takes a prefix)."""
    pairs = [_one_path_pair(i) for i in range(_EDGE_MAX)]
    return pairs, oracle_batch(pairs)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, _EDGE_MAX])
def test_path_counts_at_scan_edges(n):
    """n strings with n at the scan tile's edges (scan64: tiles of 1024): one value, a tile less one, a whole tile, a
    tile and one, two tiles and one."""
    pairs, exp = _edge_pairs()
    pairs, exp = pairs[:n], exp[:n]
    eng = G.Engine(device=0, encode_threads=4, flags=ON)
    res = eng.wait(eng.submit(pairs))
    _check_strings(res, assert_matches(res, pairs, exp=exp))
    assert len(res.path_strings) == n and res.paths_host == 0
    assert res.path_strings[n - 1] == b"data.key-%d" % (n - 1)
    eng.close()


def test_no_dirty_pair_has_no_strings():
    """No changed path: nothing to scan, an empty list comes back (not None: the option is on)."""
    pairs = [(_one_path_pair(i)[0],) * 2 for i in range(5)]
    eng = G.Engine(device=0, encode_threads=2, flags=ON)
    res = eng.wait(eng.submit(pairs))
    _check_strings(res, assert_matches(res, pairs))
    assert len(res.dirty_ids) == 0 and len(res.path_strings) == 0
    eng.close()


# ---------------------------------------------------------------- 8. option off
def _raw_wait(eng, ticket):
    r = G.Result()
    assert G.lib().gpudiff_wait(eng.ctx, ticket, C.byref(r)) == G.OK
    ps = G.PathStringsC()
    rc = G.lib().gpudiff_result_path_strings(eng.ctx, C.byref(r), C.byref(ps))
    G.lib().gpudiff_result_release(eng.ctx, C.byref(r))
    return rc


def test_option_off_and_host_encoded_batches():
    pairs = [(a, b) for _n, a, b, _e in F.load("manifests")[:80]]
    results = {}
    for flags in (G.OPT_DEVICE_ENCODE, ON):
        eng = G.Engine(device=0, encode_threads=2, flags=flags)
        res = eng.wait(eng.submit(pairs))
        exp = assert_matches(res, pairs)
        results[flags] = res
        if flags == ON:
            _check_strings(res, exp)
        else:
            assert res.path_strings is None
            assert _raw_wait(eng, eng.submit(pairs)) == G.E_STATE  # the option was off
            with pytest.raises(G.GpuDiffError) as ei:
                eng.path_stats()
            assert ei.value.code == G.E_STATE
        eng.close()
    a, b = results[G.OPT_DEVICE_ENCODE], results[ON]
    for f in ("pair_flags", "spec_dirty_ids", "status_dirty_ids", "dirty_ids", "path_offsets", "path_hashes",
              "path_kinds"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    # a host-encoded batch has no tables to walk, with the option on too; nor has a host-encode store
    eng = G.Engine(device=0, encode_threads=2, flags=G.OPT_PATH_STRINGS)
    assert _raw_wait(eng, eng.submit(pairs)) == G.E_STATE
    st = eng.object_store(max_slots=8, space_bytes=1 << 20, max_events=16, device_encode=False)
    assert _raw_wait(eng, st.submit([(0, pairs[0][1], pairs[0][0], 0, 0)])) == G.E_STATE
    st.free()
    eng.close()
