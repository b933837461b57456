"""gpudiff_cluster_index_get_final (include/gpudiff.h): what holds without a GPU -- the symbols, the argument checks,
a host-only context's refusal and the Python wrappers.  The index itself is tests/test_gpu_cluster_index_final.py."""
import ctypes as C

from kcp_amd import gpudiff as G


def test_symbols_exist():
    lib = G.lib()
    for name in ("gpudiff_cluster_index_get_final", "gpudiff_cluster_index_final_stats_get"):
        assert hasattr(lib, name), name
    assert {"gpudiff_cluster_index_get_final", "gpudiff_cluster_index_final_stats_get"} <= {
        n for n, _, _ in G.SIGNATURES}


def test_null_arguments_are_invalid():
    lib = G.lib()
    e = G.Engine(device=G.DEVICE_NONE)
    try:
        ci = G.ClusterIndexC()
        assert lib.gpudiff_cluster_index_get_final(None, 1, C.byref(ci)) == G.E_INVAL
        assert lib.gpudiff_cluster_index_get_final(e.ctx, 1, None) == G.E_INVAL
        st = G.ClusterIndexFinalStats()
        assert lib.gpudiff_cluster_index_final_stats_get(None, C.byref(st)) == G.E_INVAL
        assert lib.gpudiff_cluster_index_final_stats_get(e.ctx, None) == G.E_INVAL
    finally:
        e.close()


def test_host_only_context_gets_nodevice():
    lib = G.lib()
    e = G.Engine(device=G.DEVICE_NONE)
    try:
        ci = G.ClusterIndexC()
        ci.n_spec = 7  # the call clears its output before it refuses
        assert lib.gpudiff_cluster_index_get_final(e.ctx, 1, C.byref(ci)) == G.E_NODEVICE
        assert ci.n_spec == 0 and not ci.internal
        st = G.ClusterIndexFinalStats()
        assert lib.gpudiff_cluster_index_final_stats_get(e.ctx, C.byref(st)) == G.E_NODEVICE
        for call in (lambda: e.cluster_index_final(1), e.cluster_index_final_stats):
            try:
                call()
            except G.GpuDiffError as err:
                assert err.code == G.E_NODEVICE
            else:
                raise AssertionError("a host-only context served the call")
    finally:
        e.close()


def test_python_wrappers():
    assert callable(G.Engine.cluster_index_final) and callable(G.Engine.cluster_index_final_stats)
    names = [n for n, _ in G.ClusterIndexFinalStats._fields_]
    assert names == ["calls", "patched_calls", "compacted_calls", "sorted_calls", "syncs", "entries_in",
                     "entries_live", "patch_rows", "h2d_bytes", "d2h_bytes", "kernel_ms", "timed_calls"]
    assert set(G.ClusterIndexFinalStats().as_dict()) == set(names)
    # the struct the binding declares is the header's: 11 u64 and one double
    assert C.sizeof(G.ClusterIndexFinalStats) == 12 * 8
