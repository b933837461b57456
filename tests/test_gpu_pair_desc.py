"""K2 streams from the 16-byte pair descriptors gpudiff_dbatch_append writes beside the rows (include/gpudiff_format.h)
and loads a pair's 64-byte row only for what the descriptor leaves out.  Every batch is diffed by the default engine
and by one opened with GPUDIFF_OPT_K2_ROWS, which makes K2 read the rows as before: the two results are equal array
for array, word 7 of the pass counts (regions emitted from the stream) included, and the default one matches the
oracle."""
import copy

import numpy as np
import pytest
import torch

from kcp_amd import gpudiff as G
from tests.golden.kat_cases import BASE, J
from tests.parity import assert_matches
from tests.workload import make_pairs

pytestmark = pytest.mark.gpu

FIELDS = ("pair_flags", "spec_dirty_ids", "status_dirty_ids", "dirty_ids", "path_offsets", "path_hashes", "path_kinds")


def same(a: G.DiffResult, b: G.DiffResult):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def counts_of(e, db):
    counts = torch.zeros(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the fill runs on torch's stream, the export on the engine's
    db.export(G.EXPORT_COUNTS, counts.data_ptr(), 8)
    e.sync()
    torch.cuda.synchronize()
    return counts.cpu().numpy().view(np.uint32)


def run(pairs, flags=0, hash_bits=G.PATH_HASH_BITS, appends=1, through_view=False):
    """One pass over the pairs, appended in `appends` host batches: (DiffResult, regions emitted from the stream,
    compared bytes a pair).  through_view: the pass runs on a view of the batch, from a second context."""
    e = G.Engine(device=0, encode_threads=4, flags=flags, path_hash_bits=hash_bits)
    cuts = [len(pairs) * k // appends for k in range(appends + 1)]
    hbs = [e.encode(pairs[cuts[k]:cuts[k + 1]], ids=list(range(cuts[k], cuts[k + 1]))) for k in range(appends)]
    db = e.device_batch(sum(hb.info().pool_bytes for hb in hbs) + 4096, len(pairs))
    for hb in hbs:
        db.append(hb)
    per_pair = db.stats().compare_bytes / len(pairs)
    if through_view:
        e.sync()
        e2 = G.Engine(device=0, flags=flags, path_hash_bits=hash_bits)
        v = db.view(e2)
        res = e2.wait(e2.diff(v))
        c = counts_of(e2, v)
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
    return res, int(c[7]), per_pair


def both_ways(pairs, **kw):
    """The descriptor path against the oracle and against the row path; returns (result, compared bytes a pair)."""
    res, n_stream, per_pair = run(pairs, **kw)
    assert_matches(res, pairs, hash_bits=kw.get("hash_bits", G.PATH_HASH_BITS))
    ref, n_ref, _ = run(pairs, flags=G.OPT_K2_ROWS, **kw)
    same(res, ref)
    assert n_ref == n_stream
    return res, per_pair


def edit(o, path, value):
    o = copy.deepcopy(o)
    cur = o
    for k in path[:-1]:
        cur = cur[k]
    cur[path[-1]] = value
    return o


def without(o, key):
    o = copy.deepcopy(o)
    del o[key]
    return o


def dirty_kinds():
    """[(A, B)]: every way a pair is dirty that K2 tells apart, between clean pairs."""
    cm = {"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": "c"}, "data": {"k": "v", "long": "x" * 40}}
    grown = edit(BASE, ("spec", "extra"), {"a": 1, "b": "a string with a tail"})  # spec sizes differ
    out = [
        (J(BASE), J(BASE)),
        (J(BASE), J(grown)),                                                   # spec mismatch, status compared
        (J(BASE), J(edit(grown, ("status", "replicas"), 2))),                  # ... and status dirty in the stream
        (J(BASE), J(edit(BASE, ("status", "extra"), [1, 2, 3]))),              # status size mismatch
        (J(grown), J(edit(BASE, ("status", "extra"), 7))),                     # both sizes mismatch
        (J(cm), J(edit(cm, ("data", "k"), "w"))),                              # B without status: sentinel only
        (J(cm), J(cm)),                                                        # ... with nothing else changed
        (J(BASE), J(without(BASE, "status"))),                                 # the sentinel, A with status leaves
        (J(BASE), J(without(grown, "status"))),                                # ... after a spec join
        (J(without(BASE, "status")), J(BASE)),                                 # A without status, B with
        (J(BASE), J(edit(edit(BASE, ("spec", "replicas"), 4), ("status", "replicas"), 4))),  # both regions, streamed
        (J(BASE), J(edit(BASE, ("status", "replicas"), 3.0))),                 # a no-op status change
        (J(BASE), b'{"spec": '),                                               # decode errors, either side
        (b'[1, 2]', J(BASE)),
        (J(BASE), J(BASE)),
    ]
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_mixed_kinds(n):
    pairs, _, _ = make_pairs(n, seed=90 + n, mutate_frac=0.4)
    both_ways(pairs)


def test_every_dirty_kind():
    pairs = dirty_kinds()
    res, _ = both_ways(pairs)
    assert res.pair_flags[0] == 0 and res.pair_flags[-1] == 0
    assert int(np.count_nonzero(res.pair_flags & G.DECODE_ERROR)) == 2
    # ... and each alone in its item, and 70 of each kind side by side (an item of 64 lanes of one kind)
    for k in range(len(pairs)):
        both_ways(pairs[k:k + 1])
    both_ways([p for p in pairs for _ in range(70)])


def test_non_zero_seed():
    """8-bit path hashes force collisions, so pairs are re-seeded: the seed's value comes from the row."""
    pairs, _, _ = make_pairs(300, seed=7, mix=(("cm", 0.5), ("deploy", 0.5)), mutate_frac=0.5)
    pairs += dirty_kinds()
    e = G.Engine(device=G.DEVICE_NONE, path_hash_bits=8)
    hb = e.encode(pairs)
    assert hb.info().n_reseeded > 0
    hb.free()
    e.close()
    both_ways(pairs, hash_bits=8)


def test_escape_lane():
    """A segment of 8 MiB and more does not fit the descriptor's size fields: that pair's lane reads its row, in the
    default kernel (the batch stays under 16 KiB a pair)."""
    pairs, _, _ = make_pairs(2500, seed=11, mutate_frac=0.3)
    big = edit(BASE, ("spec", "blob"), "z" * (9 << 20))
    at = 1000 + 37
    # one pair streamed through its 9 MiB (18 MiB compared: a second one would lift the batch over 16 KiB a pair), one
    # decided by its sizes
    pairs[at:at] = [(J(big), J(edit(big, ("spec", "blob"), "z" * ((9 << 20) - 1) + "y"))),
                    (J(big), J(edit(BASE, ("spec", "blob"), "z" * (8 << 20))))]
    res, per_pair = both_ways(pairs)
    assert per_pair < 16384
    assert res.pair_flags[at] & G.SPEC_DIRTY and res.pair_flags[at + 1] & G.SPEC_DIRTY


def test_two_appends_and_a_view():
    pairs, _, _ = make_pairs(700, seed=13, mutate_frac=0.4)
    pairs += dirty_kinds()
    both_ways(pairs, appends=2)
    both_ways(pairs, appends=2, through_view=True)


def test_store_mode_keeps_the_rows():
    """The object store builds its rows on the device: the descriptors are stale, K2 reads the rows, and the option
    changes nothing."""
    from tests.test_gpu_store import _stream
    stream = _stream(5, 60, 3, 150)
    got = []
    for flags in (0, G.OPT_K2_ROWS):
        e = G.Engine(device=0, encode_threads=4, flags=flags)
        st = e.object_store(max_slots=60, space_bytes=64 << 20, max_events=256)
        out = []
        for evs, pairs in stream:
            res = e.wait(st.submit([(s, nj, oj, i, s % 7) for i, (s, nj, oj) in enumerate(evs)]))
            if not flags:
                assert_matches(res, pairs, hash_bits=e.path_hash_bits)
            out.append(res)
        got.append(out)
        st.free()
        e.close()
    for a, b in zip(*got):
        same(a, b)
