"""K2 leaves the whole 128-byte lines that hold only spec keys and metas out of its stream when the encoder has stated
both arrays equal (GPUDIFF_OBJ_SPEC_SHAPE_EQ, gpudiff_shape_hole in include/gpudiff_format.h).  One batch of about 280
pairs holds every spec size around the rule's edges, in three shapes (spec and status compared, spec only, no status
leaves), clean and with one edit each at the places the hole could hurt: the last value before it, the last meta's
leaf (a long string edited at its head and its tail's end, same length), the arena's first dword right behind it, a
long value's tail, a type flip (the bit is clear: the key hole alone), a rename (neither bit) and a status value.  The
default engine must match the oracle, match the GPUDIFF_OPT_K2_ROWS engine (which never skips) array for array, and
emit from the stream exactly the regions the rule of kcp_amd/csrc/stream_paths.h admits, counted on the host.  A last
case shows that the hole is honoured: a meta of B inside it, changed in the host batch behind the encoder's back, goes
unseen by the default engine and is found by the row path."""
import numpy as np
import pytest

from kcp_amd import gpudiff as G
from tests.golden.kat_cases import J
from tests.parity import assert_matches
from tests.test_gpu_keys_hole import admitted, order_of, run, same

pytestmark = pytest.mark.gpu

SPEC_LS = (15, 16, 17, 24, 25, 31, 32, 33, 47, 48, 49, 184)  # 16: the first hole; 17..23: none; 24: one line again
EDITS = ("clean", "last_val", "last_meta", "first_arena", "long_tail", "type_flip", "rename", "status")
SHAPES = ("both", "spec_only", "no_status")
LONG = "a long string value: its tail lies in the arena"


def shape_hole_of(L):
    lo, hi = (8 * L + 127) // 128 * 128, 16 * L // 128 * 128
    return (lo, hi) if hi > lo else (0, 0)


def keys_hole_of(L):
    lo, hi = (8 * L + 127) // 128 * 128, 12 * L // 128 * 128
    return (lo, hi) if hi > lo else (0, 0)


def make_case(L, kind, shape):
    """(A, B) with L spec leaves a side (top-level keys are spec leaves); 17 status leaves a side (both), 17 and 18
    (spec_only: the status sizes differ, so K2 streams the spec alone) or no status at all."""
    names = order_of(L)  # names[i]: leaf i of the segment
    a = {"metadata": {"name": "n%d" % L}}
    if shape != "no_status":
        a["status"] = {"s%02d" % i: i for i in range(17)}
    for nm in names:
        a[nm] = 7
    b = dict(a)
    if kind == "clean":
        pass
    elif kind == "status":
        if shape == "no_status":
            return None
        b["status"] = dict(a["status"], s05=500)
    elif kind == "last_val":
        b[names[-1]] = 8
    elif kind == "last_meta":
        a[names[-1]] = LONG
        b = dict(a)
        b[names[-1]] = "A" + LONG[1:-1] + "#"
    elif kind == "first_arena":
        a[names[0]] = LONG  # the only long string: its tail is the arena's first bytes
        b = dict(a)
        b[names[0]] = LONG[:8] + "#" + LONG[9:]
    elif kind == "long_tail":
        a[names[L // 2]] = LONG
        b = dict(a)
        b[names[L // 2]] = LONG[:-1] + "#"
    elif kind == "type_flip":
        a[names[0]] = True  # true -> false: the meta's tag alone
        b = dict(a)
        b[names[0]] = False
    elif kind == "rename":
        b = dict(a)
        del b[names[L // 2]]
        b["q" + names[L // 2][1:]] = 7
    if shape == "spec_only":
        b["status"] = dict(b["status"], extra=1)
    return a, b


def all_cases():
    out = []
    for shape in SHAPES:
        for L in SPEC_LS:
            for kind in EDITS:
                c = make_case(L, kind, shape)
                if c is not None:
                    out.append((L, kind, shape, c[0], c[1]))
    return out


def host_counts(hb):
    """(regions the rule admits, pairs with a shape hole, pairs with the key hole alone, bytes the holes leave out) of
    a host batch; the bytes of every hole are equal on both sides."""
    pool, n_adm, n_shape, n_keys, skipped = hb.pool_view(), 0, 0, 0, 0
    for r in hb.rows():
        fa, fb = int(r["flags_a"]), int(r["flags_b"])
        if (fa | fb) & G.OBJ_DECODE_ERR:
            continue
        la, lb, ara, arb = int(r["spec_l_a"]), int(r["spec_l_b"]), int(r["spec_ar_a"]), int(r["spec_ar_b"])
        sa, sb = 16 * la + ara, 16 * lb + arb
        oa, ob = int(r["off_a"]), int(r["off_b"])
        if la == lb and ara == arb:
            n_adm += admitted(pool[oa:oa + sa], pool[ob:ob + sa], la)
            lo = hi = 0
            if fb & G.OBJ_SPEC_KEYS_EQ and fb & G.OBJ_SPEC_SHAPE_EQ:
                lo, hi = shape_hole_of(la)
                n_shape += hi > lo
            elif fb & G.OBJ_SPEC_KEYS_EQ:
                lo, hi = keys_hole_of(la)
                n_keys += hi > lo
            skipped += 2 * (hi - lo)
            assert np.array_equal(pool[oa + lo:oa + hi], pool[ob + lo:ob + hi])
        ta, tb, tra, trb = int(r["stat_l_a"]), int(r["stat_l_b"]), int(r["stat_ar_a"]), int(r["stat_ar_b"])
        if fb & G.OBJ_HAS_STATUS and ta == tb and tra == trb:
            st = 16 * ta + tra
            n_adm += admitted(pool[oa + sa:oa + sa + st], pool[ob + sb:ob + sb + st], ta)
    return n_adm, n_shape, n_keys, skipped


def test_every_size_shape_and_edit():
    cases = all_cases()
    assert 250 <= len(cases) <= 320
    pairs = [(J(a), J(b)) for _, _, _, a, b in cases]

    def prepare(hb):
        rows, pool = hb.rows(), hb.pool_view()
        for (L, kind, shape, _, _), r in zip(cases, rows):  # each case is the size, the shape and the edit it says
            fb = int(r["flags_b"])
            assert int(r["spec_l_a"]) == L and int(r["flags_a"]) >> G.OBJ_SEED_SHIFT == 0
            assert bool(fb & G.OBJ_SPEC_KEYS_EQ) == (kind != "rename")
            assert bool(fb & G.OBJ_SPEC_SHAPE_EQ) == (kind not in ("rename", "type_flip"))
            assert r["spec_l_a"] == r["spec_l_b"] and r["spec_ar_a"] == r["spec_ar_b"]
            stat_sz = r["stat_l_a"] == r["stat_l_b"] and r["stat_ar_a"] == r["stat_ar_b"]
            assert stat_sz == (shape != "spec_only") and (int(r["stat_l_a"]) == 0) == (shape == "no_status")
            oa, ob, seg = int(r["off_a"]), int(r["off_b"]), 16 * L + int(r["spec_ar_a"])
            diff = np.nonzero(pool[oa:oa + seg] != pool[ob:ob + seg])[0]
            lo, hi = shape_hole_of(L)
            if kind == "last_val":
                assert diff.size and 8 * (L - 1) <= diff.min() and diff.max() < 8 * L
            elif kind == "last_meta":  # the head in vals[L - 1], the tail's end in the arena; metas[L - 1] equal
                assert diff.size == 2 and diff.min() == 8 * (L - 1) and diff.max() >= 16 * L
            elif kind == "first_arena":
                assert diff.tolist() == [16 * L]
                if 16 * L % 128 == 0:
                    assert hi == 16 * L  # the hole ends at this byte
            elif kind == "long_tail":
                assert diff.size and diff.min() >= 16 * L
            elif kind == "type_flip":
                assert diff.size and 12 * L <= diff.min() and diff.max() < 12 * L + 4
            elif kind == "rename":
                assert diff.size and 8 * L <= diff.min() and diff.max() < 12 * L
            else:
                assert diff.size == 0
        return host_counts(hb)

    res, n_stream, (n_adm, n_shape, n_keys, skipped) = run(pairs, prepare=prepare)
    exp = assert_matches(res, pairs)
    for (L, kind, shape, a, b), r in zip(cases, exp):
        assert r["spec_dirty"] == (kind not in ("clean", "status"))
        # (statussyncer.go:15-27 is asymmetric: B without a "status" key is status dirty)
        assert r["status_dirty"] == (kind == "status" or shape != "both")
    ref, n_ref, _ = run(pairs, flags=G.OPT_K2_ROWS)
    same(res, ref)
    # the regions emitted from the stream: the ones the rule admits -- every spec edit but the renames (their differing
    # key dwords send the region to the join), and the status edits of the pairs whose status sizes are equal
    print("regions admitted %d, emitted %d (row path %d); %d pairs with a shape hole, %d with the key hole alone, "
          "%d bytes left out" % (n_adm, n_stream, n_ref, n_shape, n_keys, skipped))
    assert n_adm == sum(kind not in ("clean", "rename", "status") or (kind == "status" and shape == "both")
                        for _, kind, shape, _, _ in cases)
    assert n_stream == n_adm and n_ref == n_adm
    assert n_shape == sum(shape_hole_of(L) != (0, 0) and kind not in ("rename", "type_flip") for L, kind, _, _, _ in cases)
    assert n_keys == sum(keys_hole_of(L) != (0, 0) and kind == "type_flip" for L, kind, _, _, _ in cases)
    assert n_shape > 100 and n_keys > 0


def test_the_hole_is_not_read():
    """One of B's metas inside the hole and past the keys, its tag flipped between int64 and float64 in the host batch
    after the encoder stated the arrays equal (an inline 8-byte value either way: lengths and the arena stay): the
    default engine reports the pair clean, the row path spec dirty."""
    L = 184
    a, _ = make_case(L, "clean", "both")
    small, _ = make_case(31, "clean", "both")
    pairs = [(J(small), J(small))] * 3 + [(J(a), J(a))] + [(J(small), J(small))] * 3
    at = 3
    lo, hi = shape_hole_of(L)
    assert (lo, hi) == (1536, 2944)
    i = 20  # meta i lies at byte 12 L + 4 i: inside the hole, behind the key hole's end
    assert keys_hole_of(L)[1] <= 12 * L + 4 * i and 12 * L + 4 * i + 4 <= hi

    def prepare(hb):
        r = hb.rows()[at]
        fb = int(r["flags_b"])
        assert int(r["spec_l_b"]) == L and fb & G.OBJ_SPEC_SHAPE_EQ and fb & G.OBJ_SPEC_KEYS_EQ and r["off_a"] != r["off_b"]
        metas = hb.pool_view()[int(r["off_b"]) + 12 * L:int(r["off_b"]) + 16 * L].view("<u4")
        assert int(metas[i]) == 8 << 3 | 3  # GPUDIFF_TAG_INT, 8 bytes
        metas[i] = 8 << 3 | 4               # GPUDIFF_TAG_FLOAT
        return True

    res, _, _ = run(pairs, prepare=prepare)
    assert not res.pair_flags.any() and res.dirty_ids.size == 0
    ref, _, _ = run(pairs, flags=G.OPT_K2_ROWS, prepare=prepare)
    assert ref.pair_flags[at] & G.SPEC_DIRTY and not ref.pair_flags[at] & G.STATUS_DIRTY
    assert ref.dirty_ids.tolist() == [at]
