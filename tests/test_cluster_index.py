"""gpudiff_cluster_index_host (include/gpudiff.h, kcp_amd/csrc/fanout.h) against the model of
tests/cluster_index_model.py -- no GPU needed -- and the host routine as a stand-alone program under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from tests.cluster_index_model import assert_index_equals, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC, STATUS, DECODE, SPEC_NOOP, STATUS_NOOP = 0x1, 0x2, 0x4, 0x8, 0x10


def check(flags, ids, clusters, what=""):
    from kcp_amd import gpudiff as G
    ci = G.cluster_index_host(flags, ids, clusters)
    m = model(flags, ids, clusters)
    assert_index_equals(ci, m, what)
    assert ci.sorted_on_device == 0
    return ci


def test_binding_and_header_agree():
    from kcp_amd import gpudiff as G
    src = open(os.path.join(ROOT, "include", "gpudiff.h")).read()
    body = src[src.index("typedef struct gpudiff_cluster_index {"):src.index("} gpudiff_cluster_index;")]
    fields = [n for n, _ in G.ClusterIndexC._fields_]
    assert fields == ["n_clusters", "cluster_ids", "spec_off", "status_off", "n_spec", "n_status", "spec_ids",
                      "status_ids", "sorted_on_device", "internal"]
    pos = [body.index(f) for f in fields]
    assert pos == sorted(pos)
    assert G.lib().gpudiff_abi_version() == 6  # additive: the ABI number stays


def test_empty_and_clean_and_single():
    z8, z32 = np.zeros(0, np.uint8), np.zeros(0, np.uint32)
    ci = check(z8, z32, z32, "n = 0")
    assert ci.cluster_ids.size == 0 and ci.spec_off.tolist() == [0] and ci.status_off.tolist() == [0]
    ci = check(np.zeros(100, np.uint8), np.arange(100), np.arange(100) % 7, "all clean")
    assert ci.cluster_ids.size == 0 and ci.spec_ids.size == 0 and ci.status_ids.size == 0
    # no-op bits alone are no dirt (they only ever accompany a dirty bit, and play no part)
    check(np.full(5, SPEC_NOOP | STATUS_NOOP, np.uint8), np.arange(5), np.arange(5), "no-op bits only")
    for f in (SPEC, STATUS, SPEC | STATUS, SPEC | STATUS | DECODE, 0):
        for c in (0, 7, 0xFFFFFFFF):
            ci = check([f], [42], [c], "one pair")
            assert ci.cluster_ids.tolist() == ([c] if f else [])
            assert ci.spec_ids.tolist() == ([42] if f & SPEC else [])
            assert ci.status_ids.tolist() == ([42] if f & STATUS else [])


@pytest.mark.parametrize("n,n_clusters", [(1000, 3), (1000, 997), (5000, 64), (4097, 4097)])
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_randomized_against_the_model(n, n_clusters, order):
    rng = np.random.default_rng(n * 31 + n_clusters + len(order))
    pool = np.unique(rng.integers(1, 0xFFFFFFFF, n_clusters - 2, dtype=np.uint64))  # a repeat only shrinks the pool
    pool = np.concatenate([pool, [0, 0xFFFFFFFF]]).astype(np.uint32)
    clusters = pool[rng.integers(0, pool.size, n)]
    if order == "ascending":
        clusters = np.sort(clusters)
    elif order == "descending":
        clusters = np.sort(clusters)[::-1].copy()
    flags = rng.choice(np.array([0, SPEC, STATUS, SPEC | STATUS, SPEC | STATUS | DECODE, SPEC | SPEC_NOOP,
                                 SPEC | STATUS | STATUS_NOOP], np.uint8), size=n)
    ids = rng.permutation(n).astype(np.uint32) + 7
    ci = check(flags, ids, clusters, order)
    assert 0 in pool.tolist() and 0xFFFFFFFF in pool.tolist()
    # ClusterIndex.of: every listed cluster's slices, and a cluster that is not listed
    for c in np.unique(clusters)[:50].tolist() + [0, 0xFFFFFFFF]:
        sel = clusters == c
        s, t = ci.of(c)
        assert s.tolist() == ids[sel & ((flags & SPEC) != 0)].tolist()
        assert t.tolist() == ids[sel & ((flags & STATUS) != 0)].tolist()
    missing = next(c for c in range(1, 10 ** 6) if c not in set(pool.tolist()))
    assert [a.size for a in ci.of(missing)] == [0, 0]


def test_concatenation_property_for_cluster_ordered_inputs():
    """Dirty pairs in non-decreasing cluster order: the index's lists are the result's flat lists, element for
    element (clean pairs may sit anywhere, in any cluster)."""
    rng = np.random.default_rng(5)
    n = 3000
    flags = rng.choice(np.array([0, 0, SPEC, STATUS, SPEC | STATUS, 7], np.uint8), size=n)
    clusters = np.sort(rng.integers(0, 40, n)).astype(np.uint32)
    clean = flags == 0
    clusters[clean] = rng.integers(0, 2 ** 32, int(clean.sum()), dtype=np.uint64).astype(np.uint32)
    ids = rng.permutation(n).astype(np.uint32)
    ci = check(flags, ids, clusters)
    assert ci.spec_ids.tolist() == ids[(flags & SPEC) != 0].tolist()
    assert ci.status_ids.tolist() == ids[(flags & STATUS) != 0].tolist()


def test_clusters_dirty_in_one_kind_only_and_decode_errors():
    # cluster 5: spec only; cluster 6: status only; cluster 2 (later in the batch): a decode error, dirty in both
    flags = np.array([SPEC, 0, STATUS, SPEC, STATUS, SPEC | STATUS | DECODE, 0], np.uint8)
    clusters = np.array([5, 5, 6, 5, 6, 2, 9], np.uint32)
    ids = np.array([10, 11, 12, 13, 14, 15, 16], np.uint32)
    ci = check(flags, ids, clusters)
    assert ci.cluster_ids.tolist() == [2, 5, 6]
    assert ci.spec_ids.tolist() == [15, 10, 13] and ci.spec_off.tolist() == [0, 1, 3, 3]
    assert ci.status_ids.tolist() == [15, 12, 14] and ci.status_off.tolist() == [0, 1, 1, 3]
    assert [a.tolist() for a in ci.of(6)] == [[], [12, 14]]
    assert [a.tolist() for a in ci.of(9)] == [[], []]


def test_arguments():
    from kcp_amd import gpudiff as G
    import ctypes as C
    ci = G.ClusterIndexC()
    assert G.lib().gpudiff_cluster_index_host(None, None, None, 3, C.byref(ci)) == G.E_INVAL
    assert G.lib().gpudiff_cluster_index_host(None, None, None, 0, None) == G.E_INVAL
    assert G.lib().gpudiff_cluster_index_host(None, None, None, 0, C.byref(ci)) == G.OK and ci.n_clusters == 0
    G.lib().gpudiff_cluster_index_release(None, C.byref(ci))
    assert not ci.internal
    G.lib().gpudiff_cluster_index_release(None, C.byref(ci))  # released twice: nothing left to free
    with pytest.raises(ValueError):
        G.cluster_index_host([1, 1], [1], [1, 1])
    # a host-only context has no device index and no statistics
    e = G.Engine(device=G.DEVICE_NONE)
    for call in (lambda: e.cluster_index(1), e.cluster_index_stats):
        with pytest.raises(G.GpuDiffError) as ei:
            call()
        assert ei.value.code == G.E_NODEVICE
    e.close()


# ---------------------------------------------------------------- the host routine under the sanitizers
MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "fanout.h"
using namespace gd;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)

// the definition, restated the slow way: for each listed cluster in ascending order, its rows in batch order
static void reference(const std::vector<uint8_t>& f, const std::vector<uint32_t>& id, const std::vector<uint32_t>& cl,
                      std::vector<uint32_t>& cids, std::vector<uint32_t>& so, std::vector<uint32_t>& to,
                      std::vector<uint32_t>& s, std::vector<uint32_t>& t) {
    std::vector<uint32_t> listed;
    for (size_t i = 0; i < f.size(); i++)
        if (f[i] & 3) listed.push_back(cl[i]);
    std::sort(listed.begin(), listed.end());
    listed.erase(std::unique(listed.begin(), listed.end()), listed.end());
    for (uint32_t c : listed) {
        cids.push_back(c), so.push_back((uint32_t)s.size()), to.push_back((uint32_t)t.size());
        for (size_t i = 0; i < f.size(); i++) {
            if (cl[i] != c) continue;
            if (f[i] & 1) s.push_back(id[i]);
            if (f[i] & 2) t.push_back(id[i]);
        }
    }
    so.push_back((uint32_t)s.size()), to.push_back((uint32_t)t.size());
}

static void run(const std::vector<uint8_t>& f, const std::vector<uint32_t>& id, const std::vector<uint32_t>& cl) {
    std::vector<uint32_t> block;
    uint64_t nc = 99, ns = 99, nt = 99;
    // exact-size heap copies: a read past any input is the sanitizer's to find
    std::vector<uint8_t> f2(f);
    std::vector<uint32_t> id2(id), cl2(cl);
    const FanLayout l = fan_index_host(f2.empty() ? nullptr : f2.data(), id2.empty() ? nullptr : id2.data(),
                                       cl2.empty() ? nullptr : cl2.data(), f2.size(), block, &nc, &ns, &nt);
    std::vector<uint32_t> cids, so, to, s, t;
    reference(f, id, cl, cids, so, to, s, t);
    CHECK(nc == cids.size() && ns == s.size() && nt == t.size());
    CHECK(block.size() == l.words && l.words == 3 * nc + 2 + ns + nt);
    if (fails) return;
    CHECK(std::equal(cids.begin(), cids.end(), block.begin() + l.cluster_ids));
    CHECK(std::equal(so.begin(), so.end(), block.begin() + l.spec_off));
    CHECK(std::equal(to.begin(), to.end(), block.begin() + l.status_off));
    CHECK(std::equal(s.begin(), s.end(), block.begin() + l.spec_ids));
    CHECK(std::equal(t.begin(), t.end(), block.begin() + l.status_ids));
}

int main() {
    run({}, {}, {});                                       // n = 0
    run({0, 0, 0}, {1, 2, 3}, {4, 5, 6});                  // all clean
    run({0x18}, {1}, {4});                                 // no-op bits alone
    for (uint8_t f : {1, 2, 3, 7})
        for (uint32_t c : {0u, 1u, 0xFFFFFFFFu}) run({f}, {9}, {c});  // one pair
    run({1, 2, 3, 7}, {0, 1, 2, 3}, {0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0});  // descending, the extreme ids
    run({1, 0, 2, 1, 2, 7, 0}, {10, 11, 12, 13, 14, 15, 16}, {5, 5, 6, 5, 6, 2, 9});  // one kind only, decode error
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    const uint8_t kinds[] = {0, 1, 2, 3, 7, 0x9, 0x13};
    for (int order = 0; order < 3; order++)
        for (size_t n : {2u, 63u, 64u, 65u, 1000u, 4097u})
            for (uint32_t ncl : {1u, 7u, 5000u}) {
                std::vector<uint8_t> f(n);
                std::vector<uint32_t> id(n), cl(n);
                for (size_t i = 0; i < n; i++) {
                    f[i] = kinds[rnd() % 7], id[i] = (uint32_t)rnd();
                    const uint32_t c = (uint32_t)(rnd() % ncl);
                    cl[i] = c == 0 ? 0u : c == 1 ? 0xFFFFFFFFu : c * 2654435761u;
                }
                if (order == 1) std::sort(cl.begin(), cl.end());
                if (order == 2) std::sort(cl.begin(), cl.end()), std::reverse(cl.begin(), cl.end());
                run(f, id, cl);
            }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
'''

SAN = ["-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _sanitizers_link(d):
    probe = os.path.join(d, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17"] + SAN + [probe, "-o", os.path.join(d, "probe")], capture_output=True)
    return r.returncode == 0


def test_host_routine_under_sanitizers(tmp_path):
    d = str(tmp_path)
    if not _sanitizers_link(d):
        pytest.skip("g++ cannot link -fsanitize=address,undefined here: the fanout.h host program was not run")
    src = os.path.join(d, "main.cpp")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.run(["g++", "-std=c++17"] + SAN + ["-I", os.path.join(ROOT, "kcp_amd", "csrc"), src, "-o",
                                                   os.path.join(d, "t")], check=True)
    r = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert MAIN.count("CHECK(") >= 8  # the program still holds its checks
