"""The model of gpudiff_cluster_index (include/gpudiff.h): a stable sort of the dirty positions by cluster, then the
slices.  Pure numpy, written apart from both implementations."""
import numpy as np

SPEC, STATUS = 0x1, 0x2


def model(flags, pair_ids, cluster_ids):
    """-> dict(cluster_ids, spec_off, status_off, spec_ids, status_ids), all u32, for rows in batch order."""
    flags = np.asarray(flags, dtype=np.uint8)
    pair_ids = np.asarray(pair_ids, dtype=np.uint32)
    cluster_ids = np.asarray(cluster_ids, dtype=np.uint32)
    pos = np.flatnonzero(flags & (SPEC | STATUS))
    pos = pos[np.argsort(cluster_ids[pos], kind="stable")]
    listed = np.unique(cluster_ids[pos])
    out = {"cluster_ids": listed.astype(np.uint32)}
    for name, bit in (("spec", SPEC), ("status", STATUS)):
        p = pos[(flags[pos] & bit) != 0]
        out[name + "_ids"] = pair_ids[p].astype(np.uint32)
        # cluster_ids[p] ascends: a listed cluster's slice starts at its first entry (or where it would be), and the
        # closing offset is the list's length
        starts = np.searchsorted(cluster_ids[p], listed, side="left")
        out[name + "_off"] = np.append(starts, p.size).astype(np.uint32)
    return out


def assert_index_equals(ci, m, what=""):
    """ci: kcp_amd.gpudiff.ClusterIndex, m: model(...)"""
    for k in ("cluster_ids", "spec_off", "status_off", "spec_ids", "status_ids"):
        got = getattr(ci, k)
        assert got.dtype == np.uint32 and np.array_equal(got, m[k]), (what, k, got[:16], m[k][:16])
    # the structure the consumer relies on, stated on the index itself
    assert np.all(ci.cluster_ids[1:] > ci.cluster_ids[:-1])
    for off, ids in ((ci.spec_off, ci.spec_ids), (ci.status_off, ci.status_ids)):
        assert off.size == ci.cluster_ids.size + 1 and int(off[0]) == 0 and int(off[-1]) == ids.size
        assert np.all(off[1:] >= off[:-1])
