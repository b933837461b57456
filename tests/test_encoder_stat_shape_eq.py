"""The host encoder states in flags_b whether a pair's two status regions have the same shape
(GPUDIFF_OBJ_STAT_SHAPE_EQ, include/gpudiff_format.h): both sides have a status key, stat_l_a == stat_l_b > 0, and the
two status keys[] arrays and the two status metas[] arrays are element for element equal.  A device batch's compare
image then keeps only the status values and string tails of the pair.  Here the bit of every encoded row is held
against the four status arrays read back from the pool.  No GPU: gpudiff_encode_pairs on a GPUDIFF_DEVICE_NONE
context."""
import copy

import numpy as np

from kcp_amd import gpudiff as G
from tests.golden.kat_cases import BASE, J, cases
from tests.workload import make_pairs


def u32s(pool, off, n):
    return np.frombuffer(pool, dtype="<u4", count=n, offset=off) if n else np.zeros(0, "<u4")


def check_rows(hb):
    """Every row of the batch: the bit iff no decode error, both sides with a status key, equal non-zero status leaf
    counts and equal status keys[] and metas[] in the pool; never in flags_a, never beside a decode error; with it the
    status arenas are equal.  Returns the rows' bits."""
    pool = hb.pool()
    out = []
    for r in hb.rows():
        fa, fb = int(r["flags_a"]), int(r["flags_b"])
        bit = bool(fb & G.OBJ_STAT_SHAPE_EQ)
        assert not fa & G.OBJ_STAT_SHAPE_EQ
        if (fa | fb) & G.OBJ_DECODE_ERR:
            assert fa == G.OBJ_DECODE_ERR and fb == G.OBJ_DECODE_ERR
            out.append(False)
            continue
        la, lb = int(r["stat_l_a"]), int(r["stat_l_b"])
        # the status segment follows the spec segment in each blob
        oa = int(r["off_a"]) + 16 * int(r["spec_l_a"]) + int(r["spec_ar_a"])
        ob = int(r["off_b"]) + 16 * int(r["spec_l_b"]) + int(r["spec_ar_b"])
        ka, kb = u32s(pool, oa + 8 * la, la), u32s(pool, ob + 8 * lb, lb)
        ma, mb = u32s(pool, oa + 12 * la, la), u32s(pool, ob + 12 * lb, lb)
        both = bool(fa & fb & G.OBJ_HAS_STATUS)
        want = both and la == lb and la > 0 and np.array_equal(ka, kb) and np.array_equal(ma, mb)
        assert bit == want, int(r["pair_id"])
        if bit:
            assert r["stat_ar_a"] == r["stat_ar_b"]
        out.append(bit)
    return out


def encode(pairs, **kw):
    e = G.Engine(device=G.DEVICE_NONE, encode_threads=2, **kw)
    hb = e.encode(pairs)
    bits = check_rows(hb)
    rows = hb.rows().copy()
    reseeded = int(hb.info().n_reseeded)
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


def with_status():
    o = copy.deepcopy(BASE)
    o["status"] = {"replicas": 3, "ready": True, "phase": "Running",
                   "message": "a long status message, with a tail",
                   "conditions": [{"type": "Available", "status": "True"}, {"type": "Progressing", "status": "True"}]}
    return o


def test_directed_cases():
    w = with_status()
    renamed = copy.deepcopy(w)
    renamed["status"]["stage"] = renamed["status"].pop("phase")  # another name of the same length
    no_status = copy.deepcopy(w)
    del no_status["status"]
    wide = edit(w, ("status", "m"), {"k%04d" % k: k for k in range(64)})
    pairs = [
        (J(w), J(w)),                                                                  # 0 identical
        (J(w), J(edit(w, ("status", "replicas"), 9))),                                 # 1 a status value edit
        (J(w), J(edit(w, ("status", "message"), w["status"]["message"] + "x"))),       # 2 a status string one byte longer
        (J(w), J(edit(w, ("status", "replicas"), 3.5))),                               # 3 int -> float in status
        (J(w), J(renamed)),                                                            # 4 a renamed status key
        (J(w), J(edit(w, ("status", "observedGeneration"), 4))),                       # 5 an added status field
        (J(w), J(no_status)),                                                          # 6 B without status
        (J(edit(w, ("status",), {})), J(edit(w, ("status",), {}))),                    # 7 status: {} on both sides (one leaf)
        (J(w), b'{"status": '),                                                        # 8 decode errors, either side
        (b"[1, 2]", J(w)),                                                             # 9
        (J(w), J(edit(w, ("spec", "replicas"), 9))),                                   # 10 a spec edit: the status shape stays
        (J(no_status), J(no_status)),                                                  # 11 neither side has status
        (J(w), J(edit(w, ("status", "message"), "a long status message, with a tai#"))),  # 12 a tail edit, same length
        (J(no_status), J(w)),                                                          # 13 A without status
        (J(wide), J(edit(wide, ("status", "m", "k0007"), 70))),                        # 14 a wide status, one value edit
    ]
    bits, rows, _ = encode(pairs)
    T, F = True, False
    assert bits == [T, T, F, F, F, F, F, T, F, F, T, F, T, F, T]
    # status: {} is one leaf, the empty object under the status key: the same shape on both sides
    assert rows[7]["stat_l_a"] == 1 and rows[7]["stat_l_b"] == 1 and int(rows[7]["flags_b"]) & G.OBJ_HAS_STATUS
    r = rows[2]  # one byte more: the leaf counts stay, only the meta (and perhaps the arena) moves
    assert r["stat_l_a"] == r["stat_l_b"]
    r = rows[3]  # a type flip: every size stays -- only the bit tells
    assert r["stat_l_a"] == r["stat_l_b"] and r["stat_ar_a"] == r["stat_ar_b"]
    # the bit does not depend on the spec's bits, nor they on it
    assert int(rows[10]["flags_b"]) & G.OBJ_SPEC_KEYS_EQ and int(rows[10]["flags_b"]) & G.OBJ_SPEC_SHAPE_EQ
    assert int(rows[1]["flags_b"]) & G.OBJ_SPEC_SHAPE_EQ
    # what the image saves: with the bit a pair's image bytes never exceed those of the same row without it, and fall
    # below them once the status keys and metas fill a line (8 Lt bytes a side: 64 leaves and more here)
    with_bit = rows[1:2].copy()
    without = with_bit.copy()
    without["flags_b"] &= ~np.uint32(G.OBJ_STAT_SHAPE_EQ)
    assert G.image_read_bytes(with_bit) <= G.image_read_bytes(without) <= G.read_bytes(with_bit)
    with_bit = rows[14:15].copy()
    without = with_bit.copy()
    without["flags_b"] &= ~np.uint32(G.OBJ_STAT_SHAPE_EQ)
    assert G.image_read_bytes(with_bit) + 2 * 8 * 64 - 2 * 128 < G.image_read_bytes(without) < G.read_bytes(with_bit)
    assert G.read_bytes(with_bit) == G.read_bytes(without)  # the pool's stream does not read the bit


def test_kat_cases_and_a_mixed_population():
    pairs = [(a, b) for _, a, b, _, _ in cases()]
    more, _, _ = make_pairs(1500, seed=21, mutate_frac=0.5)
    bits, rows, _ = encode(pairs + more)
    has = [bool(int(r["flags_a"]) & int(r["flags_b"]) & G.OBJ_HAS_STATUS) and r["stat_l_a"] > 0 for r in rows]
    assert 0 < sum(bits) < sum(has) < len(bits)  # both outcomes occur among the pairs with status on both sides
    print("of %d pairs: status on both sides %d, status shape equal %d" % (len(bits), sum(has), sum(bits)))


def test_reseeded_pairs():
    """8-bit path hashes force collisions: pairs are re-seeded, and the bit speaks of the arrays under the pair's
    seed."""
    pairs, _, _ = make_pairs(300, seed=7, mix=(("deploy", 1.0),), mutate_frac=0.5)
    bits, rows, reseeded = encode(pairs, path_hash_bits=8)
    assert reseeded > 0
    seeded = [(int(r["flags_a"]) >> G.OBJ_SEED_SHIFT) & 0xFF != 0 for r in rows]
    assert any(s and b for s, b in zip(seeded, bits))
    for r in rows:  # both flag words carry the seed; the bit does not disturb it
        if not int(r["flags_a"]) & G.OBJ_DECODE_ERR:
            assert (int(r["flags_a"]) >> G.OBJ_SEED_SHIFT) == (int(r["flags_b"]) >> G.OBJ_SEED_SHIFT)
