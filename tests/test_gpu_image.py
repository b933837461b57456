"""K2 streams a shape-equal pair from the batch's compare image (include/gpudiff_format.h: gpudiff_pair_image_parts):
spec vals[L] padded to 16, the spec arena, then the status region -- vals[Lt] and arena under
GPUDIFF_OBJ_STAT_SHAPE_EQ, the whole segment otherwise -- without the keys and metas the encoder has proved equal.
One batch of about 270 pairs, appended in three uneven chunks so image offsets cross appends, holds every spec size
around the compaction's edges (odd and even L: the chunk the last value shares with the padding), four status forms
(equal shape, sizes equal but a type flipped, sizes unequal, none) and one edit each at the places the compaction
could hurt.  The default engine must match the oracle, match the GPUDIFF_OPT_NO_IMAGE and GPUDIFF_OPT_K2_ROWS engines
array for array, emit from the stream exactly the regions the rule of kcp_amd/csrc/stream_paths.h admits (counted on
the host), give the same through a view, with an image that fills mid-batch and with none.  A last case shows that
the image is honoured: a spec meta of B in a partial line of the pool stream's hole and a status meta of B, each flipped
in the host batch behind the encoder's back, go unseen by the default engine and are found by the row path."""
import numpy as np
import pytest

from kcp_amd import gpudiff as G
from tests.golden.kat_cases import J
from tests.parity import assert_matches
from tests.test_gpu_keys_hole import admitted, counts_of, order_of, same

pytestmark = pytest.mark.gpu

SPEC_LS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 184)
STAT_LTS = (1, 2, 17, 18)
EDITS = ("clean", "last_val", "first_arena", "last_arena", "first_stat_val", "last_stat_val", "stat_tail", "type_flip",
         "rename", "stat_rename")
FORMS = ("eq", "flip", "uneq", "none")
LONG = "a long string value: its tail is 32 byte"  # 40 bytes: a tail of 32, so the arena ends on its last dword
CHUNKS = (97, 5)  # the first two appends' pairs; the third takes the rest
assert len(LONG) == 40


def stat_name(i):
    return "s%04d" % i


def stat_order(n):
    """The names of n status keys in the order of their (seed 0) path hashes: the leaf order of a status segment that
    holds them all.  Read from the encoder: each name alone under "status" is that object's only status leaf."""
    e = G.Engine(device=G.DEVICE_NONE)
    hb = e.encode([(J({"status": {stat_name(i): 1}}), J({"status": {stat_name(i): 1}})) for i in range(n)])
    pool, rows = hb.pool(), hb.rows()
    assert all(int(r["spec_l_a"]) == 0 and int(r["stat_l_a"]) == 1 and int(r["flags_a"]) == G.OBJ_HAS_STATUS for r in rows)
    hs = [int(np.frombuffer(pool, "<u4", 1, int(r["off_a"]) + 8)[0]) for r in rows]
    hb.free()
    e.close()
    assert len(set(hs)) == n
    return [stat_name(i) for i in sorted(range(n), key=lambda i: hs[i])]


STAT_ORDER = {}


def stat_order_of(n):
    if n not in STAT_ORDER:
        STAT_ORDER[n] = stat_order(n)
    return STAT_ORDER[n]


def make_case(L, Lt, kind, form):
    """(A, B) with L spec leaves a side (top-level keys are spec leaves) and Lt status leaves in the given form, or
    None where the edit has no place."""
    names = order_of(L)
    a = {"metadata": {"name": "n%d" % L}}
    for nm in names:
        a[nm] = 7
    snames = stat_order_of(Lt) if form != "none" else []
    if form != "none":
        a["status"] = {nm: 3 for nm in snames}
    if kind in ("first_stat_val", "last_stat_val", "stat_tail", "stat_rename") and form == "none":
        return None
    if kind in ("first_arena", "last_arena"):
        a[names[0]] = LONG  # the only long string: its tail is the whole arena
    if kind == "stat_tail":
        a["status"][snames[Lt // 2]] = LONG
    if kind == "type_flip":
        a[names[0]] = True
    b = {k: (dict(v) if isinstance(v, dict) else v) for k, v in a.items()}
    if kind == "last_val":
        b[names[-1]] = 8
    elif kind == "first_arena":
        b[names[0]] = LONG[:8] + "#" + LONG[9:]
    elif kind == "last_arena":
        b[names[0]] = LONG[:-1] + "#"
    elif kind == "first_stat_val":
        b["status"][snames[0]] = 4
    elif kind == "last_stat_val":
        b["status"][snames[-1]] = 4
    elif kind == "stat_tail":
        b["status"][snames[Lt // 2]] = LONG[:-1] + "#"
    elif kind == "type_flip":
        b[names[0]] = False  # true -> false: the meta's tag alone; the spec is not imaged
    elif kind == "rename":
        del b[names[L // 2]]
        b["q" + names[L // 2][1:]] = 7
    elif kind == "stat_rename":
        del b["status"][snames[Lt // 2]]
        b["status"]["q" + snames[Lt // 2][1:]] = 3
    if form == "flip":  # sizes equal, one status type flipped: the status segment is copied whole
        a["status"]["flag"] = True
        b["status"]["flag"] = False
    elif form == "uneq":
        b["status"]["extra"] = 1
    return a, b


def all_cases():
    out, i = [], 0
    for form in FORMS:
        for L in SPEC_LS:
            for kind in EDITS:
                if form != "eq" and kind in ("last_arena", "type_flip", "rename", "stat_rename") and L not in (3, 32):
                    continue  # the full cross product under the equal-shape form; the others on two sizes
                Lt = STAT_LTS[i % len(STAT_LTS)]
                c = make_case(L, Lt, kind, form)
                if c is not None:
                    out.append((L, Lt, kind, form, c[0], c[1]))
                    i += 1
    return out


def imaged_row(r):
    fa, fb = int(r["flags_a"]), int(r["flags_b"])
    both = G.OBJ_SPEC_KEYS_EQ | G.OBJ_SPEC_SHAPE_EQ
    return (not (fa | fb) & G.OBJ_DECODE_ERR and r["spec_l_a"] == r["spec_l_b"] and r["spec_ar_a"] == r["spec_ar_b"]
            and fb & both == both)


def image_side(r):
    """One side's image bytes of an imaged row, restated."""
    fb = int(r["flags_b"])
    s = 16 * ((int(r["spec_l_a"]) + 1) // 2) + int(r["spec_ar_a"])
    t = 0
    if fb & G.OBJ_HAS_STATUS and r["stat_l_a"] == r["stat_l_b"] and r["stat_ar_a"] == r["stat_ar_b"]:
        lt, tar = int(r["stat_l_a"]), int(r["stat_ar_a"])
        t = 16 * ((lt + 1) // 2) + tar if fb & G.OBJ_STAT_SHAPE_EQ else 16 * lt + tar
    return (s + t + 127) // 128 * 128


def host_counts(hbs):
    """(regions the rule admits, rows that are imaged, their image bytes, rows with GPUDIFF_OBJ_STAT_SHAPE_EQ)."""
    n_adm = n_img = img_bytes = n_stat = 0
    for hb in hbs:
        pool = hb.pool_view()
        for r in hb.rows():
            fa, fb = int(r["flags_a"]), int(r["flags_b"])
            if (fa | fb) & G.OBJ_DECODE_ERR:
                continue
            la, lb, ara, arb = int(r["spec_l_a"]), int(r["spec_l_b"]), int(r["spec_ar_a"]), int(r["spec_ar_b"])
            sa, sb = 16 * la + ara, 16 * lb + arb
            oa, ob = int(r["off_a"]), int(r["off_b"])
            if la == lb and ara == arb:
                n_adm += admitted(pool[oa:oa + sa], pool[ob:ob + sa], la)
            ta, tb, tra, trb = int(r["stat_l_a"]), int(r["stat_l_b"]), int(r["stat_ar_a"]), int(r["stat_ar_b"])
            if fb & G.OBJ_HAS_STATUS and ta == tb and tra == trb:
                st = 16 * ta + tra
                n_adm += admitted(pool[oa + sa:oa + sa + st], pool[ob + sb:ob + sb + st], ta)
            if imaged_row(r):
                n_img += 1
                img_bytes += 2 * image_side(r)
                n_stat += bool(fb & G.OBJ_STAT_SHAPE_EQ)
    return n_adm, n_img, img_bytes, n_stat


def check_cases(cases, hbs):
    """Each encoded row is the size, the status form and the edit its case says, the edits lie where they should;
    returns host_counts."""
    rows = np.concatenate([hb.rows() for hb in hbs])
    assert [int(r["pair_id"]) for r in rows] == list(range(len(cases)))
    for (L, Lt, kind, form, _, _), r in zip(cases, rows):  # each case is the size, the form and the edit it says
        fb = int(r["flags_b"])
        assert int(r["spec_l_a"]) == L and int(r["flags_a"]) >> G.OBJ_SEED_SHIFT == 0
        assert r["spec_l_a"] == r["spec_l_b"] and r["spec_ar_a"] == r["spec_ar_b"]
        assert bool(imaged_row(r)) == (kind not in ("type_flip", "rename"))
        want_lt = 0 if form == "none" else Lt + (form == "flip")
        assert int(r["stat_l_a"]) == want_lt
        stat_sz = r["stat_l_a"] == r["stat_l_b"] and r["stat_ar_a"] == r["stat_ar_b"]
        assert stat_sz == (form != "uneq")
        assert bool(fb & G.OBJ_STAT_SHAPE_EQ) == (form == "eq" and kind != "stat_rename")
    # where the edits lie: the last value of an odd L shares its chunk with the image's padding
    for hb in hbs:
        pool = hb.pool_view()
        for r in hb.rows():
            L, Lt, kind, form = cases[int(r["pair_id"])][:4]
            oa, ob, ar = int(r["off_a"]), int(r["off_b"]), int(r["spec_ar_a"])
            seg = 16 * L + ar
            diff = np.nonzero(pool[oa:oa + seg] != pool[ob:ob + seg])[0]
            if kind == "last_val":
                assert diff.size and 8 * (L - 1) <= diff.min() and diff.max() < 8 * L
            elif kind == "first_arena":
                assert diff.tolist() == [16 * L]
            elif kind == "last_arena":
                assert ar == 32 and diff.tolist() == [16 * L + ar - 1]
            elif kind == "type_flip":
                assert diff.size and 12 * L <= diff.min() and diff.max() < 12 * L + 4
            elif kind == "rename":
                assert diff.size and 8 * L <= diff.min() and diff.max() < 12 * L
            else:
                assert diff.size == 0
            if form in ("eq", "flip") and kind != "stat_rename":
                lt, tar = int(r["stat_l_a"]), int(r["stat_ar_a"])
                st = 16 * lt + tar
                sd = np.nonzero(pool[oa + seg:oa + seg + st] != pool[ob + seg:ob + seg + st])[0]
                if form == "flip":  # the flipped flag's meta aside
                    sd = sd[(sd < 12 * lt) | (sd >= 16 * lt)]
                if kind == "first_stat_val" and form == "eq":
                    assert sd.size and sd.max() < 8
                elif kind == "last_stat_val" and form == "eq":
                    assert sd.size and 8 * (lt - 1) <= sd.min() and sd.max() < 8 * lt
                elif kind == "stat_tail":
                    assert sd.size and sd.min() >= 16 * lt
    return host_counts(hbs)


def run(pairs, flags=0, prepare=None, capacity=None, view=False, chunks=CHUNKS):
    """One pass over the pairs, appended in len(chunks) + 1 host batches (prepare(hbs): before the appends); view: the
    pass runs on a view of the batch, under a second context.  Returns (DiffResult, word 7 of the counts, what prepare
    returned, the batch's image stats)."""
    e = G.Engine(device=0, encode_threads=4, flags=flags)
    cuts = [0] + list(np.cumsum(chunks)) + [len(pairs)]
    hbs = [e.encode(pairs[lo:hi], ids=list(range(lo, hi))) for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]
    seen = prepare(hbs) if prepare else None
    db = e.device_batch(sum(hb.info().pool_bytes for hb in hbs) + 4096, len(pairs))
    if capacity is not None:
        db.set_image_capacity(capacity)
    for hb in hbs:
        db.append(hb)
    st = db.image_stats()
    stats = (int(st.bytes_used), int(st.capacity), int(st.pairs))
    if view:
        e.sync()
        e2 = G.Engine(device=0, encode_threads=1, flags=flags)
        v = db.view(e2)
        res = e2.wait(e2.diff(v))
        c = counts_of(e2, v)
        st = v.image_stats()
        assert (int(st.bytes_used), int(st.capacity), int(st.pairs)) == stats
        v.free()
        e2.close()
    else:
        res = e.wait(e.diff(db))
        c = counts_of(e, db)
    assert int(c[2]) == res.dirty_ids.size
    db.free()
    for hb in hbs:
        hb.free()
    e.close()
    return res, int(c[7]), seen, stats


@pytest.fixture(scope="module")
def batch():
    """The cases, their pairs and the default engine's pass over them: shared by the tests below, never changed."""
    cases = all_cases()
    assert 240 <= len(cases) <= 320
    pairs = [(J(a), J(b)) for _, _, _, _, a, b in cases]


    res, n_stream, counts, stats = run(pairs, prepare=lambda hbs: check_cases(cases, hbs))
    return cases, pairs, res, n_stream, counts, stats


def test_matches_the_oracle_and_the_rule(batch):
    cases, pairs, res, n_stream, (n_adm, n_img, img_bytes, n_stat), stats = batch
    exp = assert_matches(res, pairs)
    for (L, Lt, kind, form, a, b), r in zip(cases, exp):
        assert r["spec_dirty"] == (kind in ("last_val", "first_arena", "last_arena", "type_flip", "rename"))
        stat_edit = kind in ("first_stat_val", "last_stat_val", "stat_tail", "stat_rename")
        # (statussyncer.go:15-27 is asymmetric: B without a "status" key is status dirty)
        assert r["status_dirty"] == (stat_edit or form != "eq")
    print("regions admitted %d, emitted %d; %d pairs imaged (%d with the status shape), %d image bytes" % (
        n_adm, n_stream, n_img, n_stat, img_bytes))
    assert n_stream == n_adm
    # every edit of a size-matched region is admitted but the renames (a differing key dword); a flipped status type
    # is an edit of its region too
    spec_edits, stat_edits = ("last_val", "first_arena", "last_arena", "type_flip"), ("first_stat_val", "last_stat_val", "stat_tail")
    assert n_adm == sum((kind in spec_edits) + (form == "eq" and kind in stat_edits) + (form == "flip" and kind != "stat_rename")
                        for _, _, kind, form, _, _ in cases)
    # the image holds every row it can, offsets running on across the three appends
    assert stats == (img_bytes, stats[1], n_img) and stats[1] >= img_bytes
    assert n_img == sum(kind not in ("type_flip", "rename") for _, _, kind, _, _, _ in cases) and n_stat > 60


@pytest.mark.parametrize("flags", [G.OPT_NO_IMAGE, G.OPT_K2_ROWS], ids=["no_image", "k2_rows"])
def test_same_as_the_pool_stream(batch, flags):
    _, pairs, res, n_stream, _, _ = batch
    ref, n_ref, _, stats = run(pairs, flags=flags)
    same(res, ref)
    assert n_ref == n_stream
    if flags == G.OPT_NO_IMAGE:
        assert stats == (0, 0, 0)


def test_same_through_a_view(batch):
    _, pairs, res, n_stream, _, stats = batch
    ref, n_ref, _, vstats = run(pairs, view=True)
    same(res, ref)
    assert n_ref == n_stream and vstats == stats


def test_image_full_mid_batch(batch):
    """Capacity for about half the image: the pairs past it keep their pool descriptors, the results do not change."""
    _, pairs, res, n_stream, (_, n_img, img_bytes, _), _ = batch
    cap = (img_bytes // 2) // 128 * 128
    ref, n_ref, _, (used, capacity, n) = run(pairs, capacity=cap)
    same(res, ref)
    assert n_ref == n_stream
    assert capacity == cap and 0 < used <= cap and 0 < n < n_img
    assert cap - used < 2 * 4096  # full: what is left holds no further pair of these sizes


def test_capacity_zero_is_no_image(batch):
    _, pairs, res, n_stream, _, _ = batch
    ref, n_ref, _, stats = run(pairs, capacity=0)
    same(res, ref)
    assert n_ref == n_stream and stats == (0, 0, 0)


def test_the_image_is_honoured():
    """A spec meta of B in the partial line behind the pool stream's shape hole (L = 33: the hole is [384, 512), the
    metas end at 528), and a status meta of B, each flipped between int64 and float64 in the host batch after the
    encoder stated the arrays equal: the pool's stream reads both lines, the image holds neither meta.  The default
    engine reports both pairs clean; the row path finds the one spec dirty and the other status dirty."""
    L, Lt = 33, 17
    a, _ = make_case(L, Lt, "clean", "eq")
    small, _ = make_case(3, 2, "clean", "eq")
    pairs = [(J(small), J(small))] * 3 + [(J(a), J(a))] + [(J(small), J(small))] * 2 + [(J(a), J(a))] + [(J(small), J(small))]
    at_spec, at_stat = 3, 6
    i = 30  # meta i lies at byte 12 L + 4 i = 516: past the hole's end at 512, before the arena at 528
    assert (8 * L + 127) // 128 * 128 == 384 and 16 * L // 128 * 128 == 512 and 512 <= 12 * L + 4 * i < 16 * L

    def prepare(hbs):
        hb = hbs[0]
        pool = hb.pool_view()
        for at, region in ((at_spec, "spec"), (at_stat, "status")):
            r = hb.rows()[at]
            fb = int(r["flags_b"])
            assert int(r["spec_l_b"]) == L and int(r["stat_l_b"]) == Lt and r["off_a"] != r["off_b"]
            assert fb & G.OBJ_SPEC_SHAPE_EQ and fb & G.OBJ_SPEC_KEYS_EQ and fb & G.OBJ_STAT_SHAPE_EQ
            if region == "spec":
                metas = pool[int(r["off_b"]) + 12 * L:int(r["off_b"]) + 16 * L].view("<u4")
                k = i
            else:
                seg = int(r["off_b"]) + 16 * L + int(r["spec_ar_b"])
                metas = pool[seg + 12 * Lt:seg + 16 * Lt].view("<u4")
                k = 5
            assert int(metas[k]) == 8 << 3 | 3  # GPUDIFF_TAG_INT, 8 bytes
            metas[k] = 8 << 3 | 4               # GPUDIFF_TAG_FLOAT
        return True

    res, _, _, stats = run(pairs, prepare=prepare, chunks=())
    assert stats[2] == len(pairs)
    assert not res.pair_flags.any() and res.dirty_ids.size == 0
    ref, _, _, _ = run(pairs, flags=G.OPT_K2_ROWS, prepare=prepare, chunks=())
    assert ref.pair_flags[at_spec] & G.SPEC_DIRTY and not ref.pair_flags[at_spec] & G.STATUS_DIRTY
    assert ref.pair_flags[at_stat] & G.STATUS_DIRTY and not ref.pair_flags[at_stat] & G.SPEC_DIRTY
    assert ref.dirty_ids.tolist() == [at_spec, at_stat]
