"""The host encoder states in flags_b whether a pair's two spec metas[] arrays -- every leaf's type tag and byte length
-- are element for element equal beside equal keys[] (GPUDIFF_OBJ_SPEC_SHAPE_EQ, include/gpudiff_format.h): K2 then
skips the lines of keys and metas on its word.  Here the bit of every encoded row is set against the four arrays read
back from the pool.  No GPU: gpudiff_encode_pairs on a GPUDIFF_DEVICE_NONE context."""
import copy

import numpy as np

from kcp_amd import gpudiff as G
from tests.golden.kat_cases import BASE, J, cases
from tests.workload import make_pairs


def u32s(pool, off, n):
    return np.frombuffer(pool, dtype="<u4", count=n, offset=off) if n else np.zeros(0, "<u4")


def check_rows(hb):
    """Every row of the batch: the bit iff no decode error, equal spec leaf counts, equal keys[] and equal metas[] in
    the pool; never without OBJ_SPEC_KEYS_EQ, never in flags_a, never beside a decode error; with it the spec arenas
    are equal.  Returns the rows' (keys bit, shape bit)."""
    pool = hb.pool()
    out = []
    for r in hb.rows():
        fa, fb = int(r["flags_a"]), int(r["flags_b"])
        keys, shape = bool(fb & G.OBJ_SPEC_KEYS_EQ), bool(fb & G.OBJ_SPEC_SHAPE_EQ)
        assert not fa & G.OBJ_SPEC_SHAPE_EQ
        assert keys or not shape
        if (fa | fb) & G.OBJ_DECODE_ERR:
            assert fa == G.OBJ_DECODE_ERR and fb == G.OBJ_DECODE_ERR
            out.append((False, False))
            continue
        la, lb = int(r["spec_l_a"]), int(r["spec_l_b"])
        oa, ob = int(r["off_a"]), int(r["off_b"])
        ka, kb = u32s(pool, oa + 8 * la, la), u32s(pool, ob + 8 * lb, lb)
        ma, mb = u32s(pool, oa + 12 * la, la), u32s(pool, ob + 12 * lb, lb)
        keys_eq = la == lb and np.array_equal(ka, kb)
        assert keys == keys_eq, int(r["pair_id"])
        assert shape == (keys_eq and np.array_equal(ma, mb)), int(r["pair_id"])
        if shape:
            assert r["spec_ar_a"] == r["spec_ar_b"]
        out.append((keys, shape))
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


def wide(n):
    o = copy.deepcopy(BASE)
    o["spec"]["m"] = {"k%04d" % k: k for k in range(n)}
    o["spec"]["flag"] = True
    o["spec"]["text"] = "a long string value, with a tail"
    return o


def shape_hole(L):
    lo, hi = (8 * L + 127) // 128 * 128, 16 * L // 128 * 128
    return (lo, hi) if hi > lo else (0, 0)


def keys_hole(L):
    lo, hi = (8 * L + 127) // 128 * 128, 12 * L // 128 * 128
    return (lo, hi) if hi > lo else (0, 0)


def test_directed_cases():
    w = wide(200)
    renamed = copy.deepcopy(w)
    renamed["spec"]["m"]["k01zz"] = renamed["spec"]["m"].pop("k0100")  # another name of the same length
    empty = {"metadata": {"name": "c"}}
    pairs = [
        (J(w), J(w)),                                                          # 0 identical
        (J(w), J(edit(w, ("spec", "m", "k0100"), 7))),                         # 1 a value edit, int for int
        (J(w), J(edit(w, ("spec", "text"), "a long string value, with a tai#"))),  # 2 ... a long string, same length
        (J(w), J(edit(w, ("spec", "text"), w["spec"]["text"] + "x"))),         # 3 a long string one byte longer
        (J(w), J(edit(w, ("spec", "m", "k0100"), 100.5))),                     # 4 int -> float
        (J(w), J(edit(w, ("spec", "flag"), False))),                           # 5 true -> false: the tag alone
        (J(w), J(renamed)),                                                    # 6 a key renamed, same length
        (J(w), J(edit(w, ("spec", "template"), "new"))),                       # 7 a field added
        (J(empty), J(empty)),                                                  # 8 an empty spec, both sides
        (J(w), b'{"spec": '),                                                  # 9 decode errors, either side
        (b"[1, 2]", J(w)),                                                     # 10
        (J(w), J(edit(w, ("status", "replicas"), 9))),                         # 11 a status edit: the spec's shape stays
    ]
    bits, rows, _ = encode(pairs)
    K, S, N = (True, True), (True, False), (False, False)  # both bits, the keys' alone, neither
    assert bits == [K, K, K, S, S, S, N, N, K, N, N, K]
    r = rows[3]  # one byte more: the padded tail and so every size may stay -- only the bit tells K2
    assert r["spec_l_a"] == r["spec_l_b"]
    r = rows[5]
    assert r["spec_l_a"] == r["spec_l_b"] and r["spec_ar_a"] == r["spec_ar_b"]
    assert rows[8]["spec_l_a"] == 0 and rows[8]["spec_l_b"] == 0
    # the two byte sums: gpudiff_rows_stream_bytes keeps the key holes' meaning, gpudiff_rows_read_bytes honours the bit
    kh = sh = 0
    for (keys, shape), r in zip(bits, rows):
        L = int(r["spec_l_a"])
        if not (r["spec_l_a"] == r["spec_l_b"] and r["spec_ar_a"] == r["spec_ar_b"]):
            continue
        lo, hi = keys_hole(L)
        slo, shi = shape_hole(L)
        kh += 2 * (hi - lo) if keys else 0
        sh += 2 * (shi - slo) if shape else 2 * (hi - lo) if keys else 0
    assert sh > kh > 0
    fmt = int(G.cluster_bytes(rows, 1)[0]) - (65 - 16) * len(rows)
    assert G.stream_bytes(rows) == fmt - kh
    assert G.read_bytes(rows) == fmt - sh
    plain = rows.copy()
    plain["flags_b"] &= ~np.uint32(G.OBJ_SPEC_SHAPE_EQ)
    assert G.read_bytes(plain) == fmt - kh


def test_kat_cases_and_a_mixed_population():
    pairs = [(a, b) for _, a, b, _, _ in cases()]
    more, _, _ = make_pairs(1500, seed=21, mutate_frac=0.5)
    bits, _, _ = encode(pairs + more)
    shape = [s for _, s in bits]
    assert 0 < sum(shape) < len(shape)  # both outcomes occur
    print("of %d pairs: keys equal %d, shape equal %d" % (len(bits), sum(k for k, _ in bits), sum(shape)))


def test_reseeded_pairs():
    """8-bit path hashes force collisions: pairs are re-seeded, and the bit speaks of the arrays under the pair's
    seed."""
    pairs, _, _ = make_pairs(300, seed=7, mix=(("cm", 0.5), ("deploy", 0.5)), mutate_frac=0.5)
    bits, rows, reseeded = encode(pairs, path_hash_bits=8)
    assert reseeded > 0
    seeded = [(int(r["flags_a"]) >> G.OBJ_SEED_SHIFT) & 0xFF != 0 for r in rows]
    assert any(s and b[1] for s, b in zip(seeded, bits)) and any(s and not b[1] for s, b in zip(seeded, bits))
    for r in rows:  # both flag words carry the seed; the bit does not disturb it
        if not int(r["flags_a"]) & G.OBJ_DECODE_ERR:
            assert (int(r["flags_a"]) >> G.OBJ_SEED_SHIFT) == (int(r["flags_b"]) >> G.OBJ_SEED_SHIFT)
