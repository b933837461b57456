"""The host encoder states in flags_b whether a pair's two spec keys[] arrays are element for element equal
(GPUDIFF_OBJ_SPEC_KEYS_EQ, include/gpudiff_format.h): it has both sides' leaves sorted by hash when it writes them, so
the fact is exact, and K2 skips the lines of keys on its word.  Here the bit of every encoded row is set against the
two arrays read back from the pool.  No GPU: gpudiff_encode_pairs on a GPUDIFF_DEVICE_NONE context."""
import copy

import numpy as np
import pytest

from kcp_amd import gpudiff as G
from tests.golden.kat_cases import BASE, J, cases
from tests.workload import make_pairs


def keys_of(pool, off, L):
    return np.frombuffer(pool, dtype="<u4", count=L, offset=off + 8 * L) if L else np.zeros(0, "<u4")


def check_rows(hb):
    """Every row of the batch: the bit iff no decode error, equal spec leaf counts and equal keys[] in the pool;
    never in flags_a, never beside a decode error.  Returns the rows' bits."""
    pool = hb.pool()
    out = []
    for r in hb.rows():
        fa, fb = int(r["flags_a"]), int(r["flags_b"])
        bit = bool(fb & G.OBJ_SPEC_KEYS_EQ)
        assert not fa & G.OBJ_SPEC_KEYS_EQ
        if (fa | fb) & G.OBJ_DECODE_ERR:
            assert fa == G.OBJ_DECODE_ERR and fb == G.OBJ_DECODE_ERR
            out.append(False)
            continue
        la, lb = int(r["spec_l_a"]), int(r["spec_l_b"])
        ka, kb = keys_of(pool, int(r["off_a"]), la), keys_of(pool, int(r["off_b"]), lb)
        assert np.all(ka[1:] > ka[:-1]) and np.all(kb[1:] > kb[:-1])  # ascending, unique
        assert bit == (la == lb and np.array_equal(ka, kb)), int(r["pair_id"])
        out.append(bit)
    return out


def encode(pairs, **kw):
    e = G.Engine(device=G.DEVICE_NONE, encode_threads=2, **kw)
    hb = e.encode(pairs)
    bits = check_rows(hb)
    rows = hb.rows().copy()
    info = hb.info()
    reseeded = int(info.n_reseeded)
    hb.free()
    e.close()
    return bits, rows, reseeded


def edit(o, path, value):
    o = copy.deepcopy(o)
    cur = o
    for k in path[:-1]:
        cur = cur[k]
    cur[path[-1]] = value
    return o


def wide(n):
    """A spec of n + a few leaves: keys[] spans whole 128-byte lines from 32 leaves on."""
    o = copy.deepcopy(BASE)
    o["spec"]["m"] = {"k%04d" % k: k for k in range(n)}
    return o


def test_directed_cases():
    w = wide(200)
    renamed = copy.deepcopy(w)
    renamed["spec"]["m"]["k01zz"] = renamed["spec"]["m"].pop("k0100")  # another name of the same length
    empty = {"metadata": {"name": "c"}}  # every other top-level key but status would be a spec leaf
    pairs = [
        (J(w), J(w)),                                                        # 0 identical
        (J(w), J(edit(w, ("spec", "m", "k0100"), 7))),                       # 1 a value edit
        (J(w), J(edit(w, ("spec", "template"), "a long string value, with a tail"))),  # 2 a field added
        (J(w), J(renamed)),                                                  # 3 a key renamed, same length
        (J(w), J(edit(w, ("status", "replicas"), 9))),                       # 4 a status edit: the spec keys stay
        (J(empty), J(empty)),                                                # 5 an empty spec, both sides
        (J(empty), J(edit(empty, ("metadata", "name"), "d"))),               # 6 ... metadata is not compared
        (J(w), J(empty)),                                                    # 7 spec removed
        (J(w), b'{"spec": '),                                                # 8 decode errors, either side
        (b"[1, 2]", J(w)),                                                   # 9
        (J(w), J(edit(w, ("spec", "m", "k0100"), "a string where an int was"))),  # 10 sizes differ (arena), keys equal
    ]
    bits, rows, _ = encode(pairs)
    assert bits == [True, True, False, False, True, True, True, False, False, False, True]
    r = rows[3]  # the rename: sizes equal, so only the bit tells K2 that the keys differ
    assert r["spec_l_a"] == r["spec_l_b"] and r["spec_ar_a"] == r["spec_ar_b"] and r["spec_l_a"] >= 200
    assert rows[5]["spec_l_a"] == 0 and rows[5]["spec_l_b"] == 0
    r = rows[10]
    assert r["spec_l_a"] == r["spec_l_b"] and r["spec_ar_a"] != r["spec_ar_b"]
    # what K2 reads from the descriptors (gpudiff_rows_stream_bytes): the format's bytes less the 64-B row and flag
    # byte, plus the 16-B descriptor, less both sides' key holes where the bit and equal sizes allow them
    holes = 0
    for bit, r in zip(bits, rows):
        L = int(r["spec_l_a"])
        lo, hi = (8 * L + 127) // 128 * 128, 12 * L // 128 * 128
        if bit and r["spec_l_a"] == r["spec_l_b"] and r["spec_ar_a"] == r["spec_ar_b"] and hi > lo:
            holes += 2 * (hi - lo)
    assert holes > 0
    assert G.stream_bytes(rows) == int(G.cluster_bytes(rows, 1)[0]) - (65 - 16) * len(rows) - holes
    plain = rows.copy()
    plain["flags_b"] &= ~np.uint32(G.OBJ_SPEC_KEYS_EQ)
    assert G.stream_bytes(plain) == int(G.cluster_bytes(rows, 1)[0]) - (65 - 16) * len(rows)


def test_kat_cases_and_a_mixed_population():
    pairs = [(a, b) for _, a, b, _, _ in cases()]
    more, _, _ = make_pairs(1500, seed=21, mutate_frac=0.5)
    bits, _, _ = encode(pairs + more)
    assert 0 < sum(bits) < len(bits)  # both outcomes occur


def test_reseeded_pairs():
    """8-bit path hashes force collisions: pairs are re-seeded, and the bit speaks of the keys under the pair's seed."""
    pairs, _, _ = make_pairs(300, seed=7, mix=(("cm", 0.5), ("deploy", 0.5)), mutate_frac=0.5)
    bits, rows, reseeded = encode(pairs, path_hash_bits=8)
    assert reseeded > 0
    seeded = [(int(r["flags_a"]) >> G.OBJ_SEED_SHIFT) & 0xFF != 0 for r in rows]
    assert any(s and b for s, b in zip(seeded, bits)) and any(s and not b for s, b in zip(seeded, bits))
    for r in rows:  # both flag words carry the seed; the bit does not disturb it
        if not int(r["flags_a"]) & G.OBJ_DECODE_ERR:
            assert (int(r["flags_a"]) >> G.OBJ_SEED_SHIFT) == (int(r["flags_b"]) >> G.OBJ_SEED_SHIFT)


@pytest.mark.parametrize("L", [0, 1, 31, 32, 33, 184])
def test_identical_sides_of_every_size(L):
    o = {"apiVersion": "v1", "kind": "X", "metadata": {"name": "n"}, "spec": {"k%04d" % k: k for k in range(L)}}
    bits, rows, _ = encode([(J(o), J(o))])
    assert bits == [True] and rows[0]["spec_l_a"] >= L
