"""K2 emits the changed paths of a size-matched dirty region from its compare stream when the mismatching chunks
locate the changed leaves (kcp_amd/csrc/stream_paths.h), and merge-joins the region otherwise.  Every case is
checked three ways: against the oracle, against an engine that defers every join to K4 (which never takes the
stream's path) array for array, and with K2's timeline build installed.  Word 7 of the pass counts says how
many regions the stream emitted."""
import copy

import numpy as np
import pytest
import torch

from kcp_amd import gpudiff as G
from kcp_amd import synth as S
from tests.golden.kat_cases import BASE, J
from tests.parity import assert_matches, oracle_batch
from tests.workload import make_pairs

pytestmark = pytest.mark.gpu

DEFER_ALL = 14 << G.OPT_ARENA_SHIFT  # every join in K4: no pair's paths come from K2


def run(pairs, flags=0, timeline=False, hash_bits=G.PATH_HASH_BITS, make_hb=None):
    """One pass over the pairs (or over the host batch make_hb(engine) encodes): (DiffResult, regions emitted from
    the stream)."""
    e = G.Engine(device=0, encode_threads=4, flags=flags, path_hash_bits=hash_bits)
    prof = None
    if timeline:
        prof = torch.zeros(12 << 16, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        e.k2_profile(prof.data_ptr(), 1 << 16)
    hb = e.encode(pairs) if make_hb is None else make_hb(e)
    inf = hb.info()
    db = e.device_batch(inf.pool_bytes + 4096, max(1, inf.n_pairs))
    db.append(hb)
    res = e.wait(e.diff(db))
    counts = torch.zeros(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the fill runs on torch's stream, the export on the engine's
    db.export(G.EXPORT_COUNTS, counts.data_ptr(), 8)
    e.sync()
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint32)
    assert int(c[2]) == res.dirty_ids.size
    if timeline:
        assert int((prof.view(-1, 12)[:, 4] != 0).sum()) > 0  # the timeline build ran
        e.k2_profile(0, 0)
    db.free()
    hb.free()
    e.close()
    return res, int(c[7])


def same(a: G.DiffResult, b: G.DiffResult):
    for f in ("pair_flags", "spec_dirty_ids", "status_dirty_ids", "dirty_ids", "path_offsets", "path_hashes",
              "path_kinds"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def three_ways(pairs, hash_bits=G.PATH_HASH_BITS):
    """Oracle, all-deferred engine and timeline build; returns (oracle results, default result, its counter)."""
    res, n_stream = run(pairs, hash_bits=hash_bits)
    exp = assert_matches(res, pairs, hash_bits=hash_bits)
    ref, n_ref = run(pairs, flags=DEFER_ALL, hash_bits=hash_bits)
    assert n_ref == 0
    same(res, ref)
    tl, n_tl = run(pairs, timeline=True, hash_bits=hash_bits)
    same(res, tl)
    assert n_tl == n_stream
    return exp, res, n_stream


def base(**spec_extra):
    o = copy.deepcopy(BASE)
    o["spec"].update(spec_extra)
    return o


def edit(o, path, value):
    o = copy.deepcopy(o)
    cur = o
    for k in path[:-1]:
        cur = cur[k]
    cur[path[-1]] = value
    return o


def long_strings(o, path=()):
    """Paths of the string leaves of 10 bytes and more (a tail in the arena)."""
    if isinstance(o, dict):
        for k, v in o.items():
            yield from long_strings(v, path + (k,))
    elif isinstance(o, list):
        for i, v in enumerate(o):
            yield from long_strings(v, path + (i,))
    elif isinstance(o, str) and len(o.encode()) >= 10:
        yield path


def grown_across_padding():
    """A string grown from a 4-byte to a 5-byte tail (4 -> 8 padded: every later tail shifts) beside a filler that
    keeps the region's 16-B arena size equal, so the region is still streamed."""
    for fill in range(9, 26):
        a = base(grow="12345678abcd", zfill="f" * fill, zz="a later long value")
        b = edit(a, ("spec", "grow"), "12345678abcde")
        ia, _ = G.encode_object_host(J(a))
        ib, _ = G.encode_object_host(J(b))
        if ia["spec_ar"] == ib["spec_ar"] and ia["spec_l"] == ib["spec_l"]:
            return a, b
    raise AssertionError("no filler keeps the arena size")


def hand_made():
    """[(A, B, regions the stream is to emit)]; the first 64 pairs fill one item with one change each."""
    out = []
    a0 = base(paused=True, s="abc", nine="123456789", f=2.5,
              vals=["v%d-%s" % (i, "xy" * (6 + 5 * i)) for i in range(5)])
    for i in range(64):
        out.append((a0, edit(a0, ("spec", "replicas"), 100 + i), 1))
    # int -> int at every leaf of an all-int status region (its first and last leaf among them), odd and even L
    for L in (7, 8, 1):
        st = {"n%d" % i: i for i in range(L)}
        a = copy.deepcopy(a0)
        a["status"] = st
        for i in range(L):
            out.append((a, edit(a, ("status", "n%d" % i), 50 + i), 1))
    out.append((a0, edit(a0, ("spec", "replicas"), 3.0), 1))       # int -> float, equal value: the no-op bit
    out.append((a0, edit(a0, ("spec", "replicas"), 3.5), 1))
    out.append((edit(a0, ("spec", "replicas"), 3.0), a0, 1))       # float -> int
    out.append((a0, edit(a0, ("spec", "f"), 2.75), 1))
    out.append((a0, edit(a0, ("spec", "paused"), False), 1))
    out.append((a0, edit(a0, ("spec", "s"), "abcd"), 1))
    out.append((a0, edit(a0, ("spec", "nine"), "1234567890"), 1))  # 9 -> 10 bytes: the same padded tail
    out.append((edit(a0, ("spec", "nine"), "1234567890"), a0, 1))
    for p in long_strings(a0["spec"], ("spec",)):                  # a same-length edit in the tail of every long value
        cur = a0
        for k in p:
            cur = cur[k]
        out.append((a0, edit(a0, p, cur[:-1] + ("#" if cur[-1] != "#" else "!")), 1))
        out.append((a0, edit(a0, p, cur[:8] + ("#" if cur[8] != "#" else "!") + cur[9:]), 1))  # its first tail byte
    ga, gb = grown_across_padding()
    out.append((ga, gb, 0))
    out.append((gb, ga, 0))  # shrunk: every differing arena dword lies in a tail of A, only the lengths tell
    renamed = copy.deepcopy(a0)                                     # a key renamed to one of equal length
    renamed["spec"]["pauseb"] = renamed["spec"].pop("paused")
    out.append((a0, renamed, 0))
    # spec from the stream and status from the join in one pair, and the reverse
    s1 = edit(a0, ("spec", "replicas"), 4)
    t_add = edit(a0, ("status", "extra"), 1)
    out.append((a0, edit(s1, ("status", "extra"), 1), 1))
    out.append((a0, edit(edit(a0, ("spec", "extra"), 1), ("status", "replicas"), 9), 1))
    t_ren = copy.deepcopy(s1)
    t_ren["status"]["replicaz"] = t_ren["status"].pop("replicas")
    out.append((a0, t_ren, 1))
    out.append((a0, edit(s1, ("status", "replicas"), 9), 2))       # both from the stream
    out.append((a0, t_add, 0))
    nos = copy.deepcopy(s1)                                         # the sentinel after a streamed spec region
    del nos["status"]
    out.append((a0, nos, 1))
    # two leaves changed in one region; then more mismatching chunks than the log holds
    out.append((a0, edit(edit(a0, ("spec", "replicas"), 5), ("spec", "s"), "abd"), 1))
    big = base(m={"k%04d" % k: k for k in range(260)})
    big_b = copy.deepcopy(big)
    big_b["spec"]["m"] = {k: v + 1 for k, v in big["spec"]["m"].items()}
    out.append((big, big_b, 0))
    # ... and clean pairs in between
    out += [(a0, a0, 0), (big, big, 0)]
    return out


def test_hand_made_pairs():
    cases = hand_made()
    assert 100 < len(cases) < 400
    pairs = [(J(a), J(b)) for a, b, _ in cases]
    exp, res, n_stream = three_ways(pairs)
    # every case that names its outcome: dirty as meant, and emitted from the stream or not
    for i, ((a, b, want), r) in enumerate(zip(cases, exp)):
        assert (r["spec_dirty"] or r["status_dirty"]) == (J(a) != J(b)), i
    assert n_stream == sum(w for _, _, w in cases)
    # the int -> float pair of equal value carries the no-op bit, from the stream
    i = 64 + 16
    assert cases[i][1]["spec"]["replicas"] == 3.0 and isinstance(cases[i][1]["spec"]["replicas"], float)
    assert res.pair_flags[i] & G.SPEC_NOOP and not res.pair_flags[i + 1] & G.SPEC_NOOP
    # the all-int status regions: the changed leaves include the region's first and last key
    at = 64
    for L in (7, 8, 1):
        hs = [exp[k]["paths"][0][0] for k in range(at, at + L)]
        assert all(len(exp[k]["paths"]) == 1 for k in range(at, at + L)) and len(set(hs)) == L
        at += L
    # each case alone gives the same answer as inside the batch (its item then holds one dirty pair)
    for k in (64 + 16, len(cases) - 4):
        one, n1 = run(pairs[k:k + 1])
        assert_matches(one, pairs[k:k + 1], exp=exp[k:k + 1])
        assert n1 == cases[k][2]


def test_fallback_leaves_the_counter():
    """The string grown across its padding, the renamed key and the 260 changed ints, each in a batch of its own:
    streamed, refused by the rule or the log's cap, joined -- and nothing counted."""
    cases = [c for c in hand_made() if c[2] == 0 and c[0] != c[1]]
    assert len(cases) >= 4
    for a, b, _ in cases:
        pairs = [(J(a), J(b))]
        _, _, n_stream = three_ways(pairs)
        assert n_stream == 0


def test_non_zero_seed():
    """8-bit path hashes force collisions, so pairs are re-seeded: the sentinel and the keys under the pair's seed."""
    pairs, _, _ = make_pairs(200, seed=5, mix=(("cm", 0.5), ("deploy", 0.5)), mutate_frac=0.5)
    pairs += [(J(a), J(b)) for a, b, _ in hand_made()[60:110]]
    _, _, n_stream = three_ways(pairs, hash_bits=8)
    assert n_stream > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000])
def test_mixed_population(n):
    pairs, _, _ = make_pairs(n, seed=70 + n, mutate_frac=0.3)
    _, res, n_stream = three_ways(pairs)
    if n >= 3000:
        assert 0 < n_stream <= 2 * res.dirty_ids.size


def size_matched_dirty_regions(rows, pool):
    """Regions K2 streams (both sides' sizes equal) whose bytes differ: the ones the join used to read again."""
    n = 0
    for r in rows:
        if (int(r["flags_a"]) | int(r["flags_b"])) & G.OBJ_DECODE_ERR:
            continue
        sa = 16 * int(r["spec_l_a"]) + int(r["spec_ar_a"])
        sb = 16 * int(r["spec_l_b"]) + int(r["spec_ar_b"])
        oa, ob = int(r["off_a"]), int(r["off_b"])
        if r["spec_l_a"] == r["spec_l_b"] and r["spec_ar_a"] == r["spec_ar_b"]:
            n += not np.array_equal(pool[oa:oa + sa], pool[ob:ob + sa])
        if (int(r["flags_b"]) & G.OBJ_HAS_STATUS) and r["stat_l_a"] == r["stat_l_b"] and r["stat_ar_a"] == r["stat_ar_b"]:
            st = 16 * int(r["stat_l_a"]) + int(r["stat_ar_a"])
            n += not np.array_equal(pool[oa + sa:oa + sa + st], pool[ob + sb:ob + sb + st])
    return n


def test_config3_most_regions_come_from_the_stream():
    """The first 20,000 pairs of config3: at least half of the size-matched dirty regions are emitted from the
    stream (802 such regions, of which the rule admits 518 -- counted on the host; the bar is 401), none with
    every join deferred, and both engines give the same arrays."""
    pop = S.Population(S.make_cfg("config3", n_pairs=20000, n_clusters=200))
    seen = []

    def make_hb(e):
        hb = pop.chunk(e, 0, pop.n, 8).hb
        if not seen:
            seen.append(size_matched_dirty_regions(hb.rows(), hb.pool_view()))
        return hb
    res, n_stream = run(None, make_hb=make_hb)
    regions = seen[0]
    assert regions == 802
    print("size-matched dirty regions %d, emitted from the stream %d" % (regions, n_stream))
    assert 2 * n_stream >= regions
    assert n_stream <= regions
    ref, n_ref = run(None, flags=DEFER_ALL, make_hb=make_hb)
    assert n_ref == 0
    same(res, ref)
    pop.close()
