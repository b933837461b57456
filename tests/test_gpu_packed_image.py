"""The compare image holds an imaged pair's regions packed to their values' true lengths (include/gpudiff_format.h:
gpudiff_meta_packed): a string's length padded to 4, a number's 8 bytes, nothing for null, false, true, {} and [].
One batch of about 300 pairs, appended in three uneven chunks, holds every tag, strings of every length 0..13 and 16,
17, 40, spec leaf counts around the builder's rounds of 64 leaves, status regions of 0, 1, 2 and 17 leaves in four forms
(equal shape, a type flipped -- copied whole --, absent in B, sizes unequal), regions of tag-only leaves alone, and edits
where the packing could hurt: the first and the last leaf, an int, a float, a one-character string, the last byte of
strings of every length, bytes 7, 8 and 9 of a long string (the head/tail boundary), leaves 63, 64 and 65, more changed
chunks than the log holds and more than 64 changed leaves (which overflow the log first: the bound on the leaf set
cannot be reached with a four-chunk log).  The default engine must match the oracle, match the
GPUDIFF_OPT_NO_IMAGE and GPUDIFF_OPT_K2_ROWS engines array for array, emit from the stream exactly the regions the packed
rule of kcp_amd/csrc/stream_paths.h admits (counted on the host; fewer chunks overflow the log than in the pool's
stream, so the count is not the pool stream's), sum on the device the streamed bytes the host sums, leave the image's
accounting what the slots' formula says, and give the same through a view and with an image that fills mid-batch."""
import numpy as np
import pytest

from kcp_amd import gpudiff as G
from tests.golden.kat_cases import J
from tests.parity import assert_matches
from tests.test_gpu_image import image_side, imaged_row, stat_order_of
from tests.test_gpu_keys_hole import admitted, counts_of, meta_arena, order_of, same

pytestmark = pytest.mark.gpu

LONG = "a long string value: its tail is 32 byte"  # 40 bytes
STRS = ["abcdefghijklmnopqrstuvwxyz"[:n] for n in range(14)] + ["p" * 16, "q" * 17, LONG]
TAG_ONLY = [False, True, {}, []]
VALUES = TAG_ONLY + [7, 1.5] + STRS  # leaf i of a case takes VALUES[(i + shift) % len(VALUES)]
# (a top-level null is no spec leaf; under "status" it is one: the status regions hold the eighth tag)
STAT_TAG_ONLY = [None] + TAG_ONLY
STAT_VALUES = [None] + VALUES
SPEC_LS = (1, 2, 3, 16, 17, 33, 64, 65, 130)
STAT = [(lt, form) for lt in (0, 1, 2, 17) for form in ("eq", "flip", "absent", "uneq")]
CHUNKS = (97, 5)
LOG_CAP = 4
assert len(LONG) == 40 and [len(s) for s in STRS] == list(range(14)) + [16, 17, 40]


def edited(v, at=None):
    """Another value of the same type and length: an int, a float, or a string with byte `at` (default: the last)
    changed."""
    if isinstance(v, str):
        at = len(v) - 1 if at is None else at
        return v[:at] + "#" + v[at + 1:]
    return v + 1


def make_case(idx, L, st, spec_edits=(), stat_edits=(), tag_only=False, stat_tag_only=False):
    """(L, A's status leaves, A, B): L spec leaves (top-level keys) and st = (Lt, form) status leaves, values by VALUES
    shifted by the case's index.  spec_edits / stat_edits: (leaf, value or None, byte or None) -- the leaf is given the value (when not None)
    on both sides, then B's is edited at that byte."""
    names = order_of(L)
    a = {"metadata": {"name": "c%d" % idx}}
    for i, nm in enumerate(names):
        a[nm] = TAG_ONLY[(i + idx) % len(TAG_ONLY)] if tag_only else VALUES[(i + idx) % len(VALUES)]
    lt, form = st
    snames = stat_order_of(lt) if lt else []
    a["status"] = {nm: (STAT_TAG_ONLY[(i + idx) % len(STAT_TAG_ONLY)] if stat_tag_only
                        else STAT_VALUES[(i + 3 * idx + 5) % len(STAT_VALUES)]) for i, nm in enumerate(snames)}
    for leaf, v, _ in spec_edits:
        if v is not None:
            a[names[leaf]] = v
    for leaf, v, _ in stat_edits:
        if v is not None:
            a["status"][snames[leaf]] = v
    b = {k: (dict(v) if k == "status" else v) for k, v in a.items()}  # (the values themselves are never changed)
    for leaf, _, at in spec_edits:
        b[names[leaf]] = edited(a[names[leaf]], at)
    for leaf, _, at in stat_edits:
        b["status"][snames[leaf]] = edited(a["status"][snames[leaf]], at)
    if form == "flip":  # sizes equal, one status type flipped: the status segment is copied whole
        a["status"]["flag"] = True
        b["status"]["flag"] = False
    elif form == "absent":
        del b["status"]
    elif form == "uneq":
        b["status"]["extra"] = 1
    elif lt == 0:  # no status leaf in the equal form: no status key on either side ("status": {} is a leaf, tag {})
        del a["status"], b["status"]
    return L, (lt + (form == "flip")) or int(form != "eq"), a, b


def all_cases():
    out = []

    def add(L, st, **kw):
        out.append(make_case(len(out), L, st, **kw))

    def st_at(k):
        return STAT[k % len(STAT)]

    # every size: clean, the first leaf, the last leaf, each under another status form
    for L in SPEC_LS:
        add(L, st_at(len(out)))
        add(L, st_at(len(out)), spec_edits=[(0, 7, None)])
        add(L, st_at(len(out)), spec_edits=[(L - 1, 7, None)])
    # an int, a float, the last byte of a string of every length, bytes 7, 8, 9 of a long string, at a middle leaf
    for L in (2, 3, 16, 17, 33, 64, 65):
        mid = L // 2
        for v in [7, 1.5] + STRS[1:]:
            add(L, st_at(len(out)), spec_edits=[(mid, v, None)])
        for at in (7, 8, 9):
            add(L, st_at(len(out)), spec_edits=[(mid, LONG, at)])
    # the builder's second round of 64 leaves
    for L, leaf in ((130, 63), (130, 64), (130, 65), (65, 63), (65, 64)):
        add(L, st_at(len(out)), spec_edits=[(leaf, 7, None)])
        add(L, st_at(len(out)), spec_edits=[(leaf, LONG, 39)])
    # more changed chunks than the log holds; more than 64 changed leaves; five ints two leaves apart among tag-only
    # leaves -- five chunks of the pool's vals[], 40 packed bytes
    add(130, (17, "eq"), spec_edits=[(i, LONG, 20) for i in (0, 25, 50, 75, 100, 129)])
    # (65 changed ints are 520 packed bytes: they overflow the four-chunk log long before |S| could pass kSpMaxLeaves
    # -- with kSpLogCap = 4 a log names at most 16 leaves, so that refusal cannot be reached from the stream and the
    # case checks the overflow's way to the join with many leaves, not the |S| bound, which tests/test_packed_rule.py's
    # serial rule keeps)
    add(130, (2, "eq"), spec_edits=[(i, 7, None) for i in range(0, 130, 2)][:70])
    add(33, (1, "eq"), tag_only=True, spec_edits=[(i, 7, None) for i in (4, 6, 8, 10, 12)])
    add(33, (17, "eq"), stat_tag_only=True, stat_edits=[(i, 7, None) for i in (4, 6, 8, 10, 12)])
    # regions of tag-only leaves alone: they pack to nothing
    for L in (3, 17):
        for st in ((17, "eq"), (2, "flip"), (0, "eq"), (1, "absent")):
            add(L, st, tag_only=True)
        add(L, (17, "eq"), tag_only=True, stat_edits=[(16, 7, None)])
        add(L, (2, "eq"), stat_tag_only=True)
        add(L, (17, "eq"), stat_tag_only=True, spec_edits=[(L - 1, "z", None)])
    # the status region under the equal-shape form: the same edits
    for lt in (1, 2, 17):
        for k, L in enumerate((1, 16, 65)):
            add(L, (lt, "eq"), stat_edits=[(0, 7, None)])
            add(L, (lt, "eq"), stat_edits=[(lt - 1, 1.5, None)])
            add(L, (lt, "eq"), stat_edits=[(lt // 2, STRS[1 + 4 * k], None)])
            add(L, (lt, "eq"), stat_edits=[(lt // 2, LONG, 7 + k)])
            add(L, (lt, "eq"), stat_edits=[(lt - 1, LONG, 39)], spec_edits=[(L - 1, STRS[9], None)])
    # every status form beside an edited and a clean spec
    for st in STAT:
        add(16, st, spec_edits=[(15, "abcde", None)])
        add(17, st)
    return out


# ---- the packed region and its rule (kcp_amd/csrc/stream_paths.h: sp_packed_rule), restated
def pk(m):
    tag, ln = m & 7, m >> 3
    return (ln + 3) // 4 * 4 if tag == 5 else 8 if tag in (3, 4) else 0


def pack(seg: np.ndarray, metas, L: int):
    """(the packed bytes of the region's segment by the given metas, the leaf that owns each dword; L: the padding)."""
    out, own, t = bytearray(), [], 0
    for i, m in enumerate(metas):
        n = pk(m)
        out += seg[8 * i:8 * i + min(n, 8)].tobytes()
        if n > 8:
            out += seg[16 * L + t:16 * L + t + n - 8].tobytes()
        t += meta_arena(m)
        own += [i] * (n // 4)
    pad = -len(out) % 16
    out += bytes(pad)
    own += [L] * (pad // 4)
    return np.frombuffer(bytes(out), "<u4"), own


def packed_admitted(sa: np.ndarray, sb: np.ndarray, L: int):
    ma = [int(m) for m in sa.view("<u4")[3 * L:4 * L]]
    mb = [int(m) for m in sb.view("<u4")[3 * L:4 * L]]
    pa, own = pack(sa, ma, L)
    pb, _ = pack(sb, ma, L)  # (A's metas for both sides, as the builder does)
    d = np.nonzero(pa != pb)[0]
    if d.size == 0 or np.unique(d // 4).size > LOG_CAP:
        return False
    leaves = {own[w] for w in d.tolist()}
    return L not in leaves and len(leaves) <= 64 and all(meta_arena(ma[i]) == meta_arena(mb[i]) for i in leaves)


def host_counts(hbs):
    """(regions the default engine emits from the stream, the same for the pool's stream, imaged rows, their image
    bytes by the slots' formula, the streamed bytes the library sums on the host)."""
    n_adm = n_pool = n_img = img_bytes = streamed = 0
    for hb in hbs:
        pool = hb.pool_view()
        rows = hb.rows()
        streamed += G.image_streamed_bytes(rows, pool)
        for r in rows:
            fa, fb = int(r["flags_a"]), int(r["flags_b"])
            assert not (fa | fb) & G.OBJ_DECODE_ERR and fa >> G.OBJ_SEED_SHIFT == 0
            la, lb, ara, arb = int(r["spec_l_a"]), int(r["spec_l_b"]), int(r["spec_ar_a"]), int(r["spec_ar_b"])
            sa, sb = 16 * la + ara, 16 * lb + arb
            oa, ob = int(r["off_a"]), int(r["off_b"])
            img = bool(imaged_row(r))
            if la == lb and ara == arb:
                A, B = pool[oa:oa + sa], pool[ob:ob + sa]
                n_pool += admitted(A, B, la)
                n_adm += packed_admitted(A, B, la) if img else admitted(A, B, la)
            ta, tb, tra, trb = int(r["stat_l_a"]), int(r["stat_l_b"]), int(r["stat_ar_a"]), int(r["stat_ar_b"])
            if fb & G.OBJ_HAS_STATUS and ta == tb and tra == trb:
                st = 16 * ta + tra
                A, B = pool[oa + sa:oa + sa + st], pool[ob + sb:ob + sb + st]
                n_pool += admitted(A, B, ta)
                n_adm += packed_admitted(A, B, ta) if img and fb & G.OBJ_STAT_SHAPE_EQ else admitted(A, B, ta)
            if img:
                n_img += 1
                img_bytes += 2 * image_side(r)
    return n_adm, n_pool, n_img, img_bytes, streamed


def run(pairs, flags=0, prepare=None, capacity=None, view=False):
    """One pass over the pairs, appended in three host batches.  Returns (DiffResult, word 7 of the counts, what prepare
    returned, the batch's image stats, the device's streamed-bytes sum)."""
    e = G.Engine(device=0, encode_threads=4, flags=flags)
    cuts = [0] + list(np.cumsum(CHUNKS)) + [len(pairs)]
    hbs = [e.encode(pairs[lo:hi], ids=list(range(lo, hi))) for lo, hi in zip(cuts[:-1], cuts[1:])]
    seen = prepare(hbs) if prepare else None
    db = e.device_batch(sum(hb.info().pool_bytes for hb in hbs) + 4096, len(pairs))
    if capacity is not None:
        db.set_image_capacity(capacity)
    for hb in hbs:
        db.append(hb)
    st = db.image_stats()
    stats = (int(st.bytes_used), int(st.capacity), int(st.pairs))
    streamed = db.image_streamed_bytes()
    if view:
        e.sync()
        e2 = G.Engine(device=0, encode_threads=1, flags=flags)
        v = db.view(e2)
        res = e2.wait(e2.diff(v))
        c = counts_of(e2, v)
        assert v.image_streamed_bytes() == streamed
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
    return res, int(c[7]), seen, stats, streamed


@pytest.fixture(scope="module")
def batch():
    """The pairs and the default engine's pass over them: shared by the tests below, never changed."""
    cases = all_cases()
    assert 250 <= len(cases) <= 330
    pairs = [(J(a), J(b)) for _, _, a, b in cases]

    def prepare(hbs):  # each case has the leaves it says, so the edits lie where they should
        rows = np.concatenate([hb.rows() for hb in hbs])
        assert [(int(r["spec_l_a"]), int(r["stat_l_a"])) for r in rows] == [(L, lt) for L, lt, _, _ in cases]
        return host_counts(hbs)

    res, n_stream, counts, stats, streamed = run(pairs, prepare=prepare)
    return pairs, res, n_stream, counts, stats, streamed


def test_matches_the_oracle_and_the_packed_rule(batch):
    pairs, res, n_stream, (n_adm, n_pool, n_img, img_bytes, host_streamed), stats, streamed = batch
    assert_matches(res, pairs)
    print("regions emitted %d, admitted packed %d, by the pool's stream %d; %d of %d pairs imaged, %d image bytes, "
          "%d streamed" % (n_stream, n_adm, n_pool, n_img, len(pairs), img_bytes, streamed))
    assert n_stream == n_adm
    assert n_adm > n_pool > 100  # (the five ints two leaves apart: five chunks of the pool, three or four packed)
    # the device's sum is the host's, and below what the slots hold
    assert streamed == host_streamed and 0 < streamed < 16 * n_img + img_bytes
    # the image's accounting is the slots', whatever is packed into them
    assert stats == (img_bytes, stats[1], n_img) and stats[1] >= img_bytes and n_img > 250


@pytest.mark.parametrize("flags", [G.OPT_NO_IMAGE, G.OPT_K2_ROWS], ids=["no_image", "k2_rows"])
def test_same_as_the_pool_stream(batch, flags):
    pairs, res, _, (_, n_pool, _, _, _), _, _ = batch
    ref, n_ref, _, stats, streamed = run(pairs, flags=flags)
    same(res, ref)
    assert n_ref == n_pool
    if flags == G.OPT_NO_IMAGE:
        assert stats == (0, 0, 0) and streamed == 0


def test_same_through_a_view(batch):
    pairs, res, n_stream, _, stats, streamed = batch
    ref, n_ref, _, vstats, vstreamed = run(pairs, view=True)
    same(res, ref)
    assert n_ref == n_stream and vstats == stats and vstreamed == streamed


def test_image_full_mid_batch(batch):
    """Capacity for about half the image: the pairs past it keep their pool descriptors, the results do not change."""
    pairs, res, _, (_, _, n_img, img_bytes, _), _, streamed = batch
    cap = (img_bytes // 2) // 128 * 128
    ref, _, _, (used, capacity, n), part = run(pairs, capacity=cap)
    same(res, ref)
    assert capacity == cap and 0 < used <= cap and 0 < n < n_img
    assert 0 < part < streamed
