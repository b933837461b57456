"""The path renderer shared by host and device (kcp_amd/csrc/pathstr.h) through its host entry point,
gpudiff_render_path_from_blob: a path hash becomes the oracle's text ("spec.containers[0].image") by a walk of
one blob's path table -- no document is decoded again.  Every comparison is exact byte equality.  No GPU needed;
tests/test_gpu_path_strings.py runs the same walk as kernels K15 / K16."""
import ctypes as C

import pytest

from kcp_amd import gpudiff as G
from oracle import gpudiff_oracle as O
from tests import path_strings_cases as PC
from tests.golden import fixtures as F


def _render(blob, info, seed, h):
    return G.render_path_from_blob(blob, info, seed, h)


def _code(blob, info, seed, h):
    with pytest.raises(G.GpuDiffError) as ei:
        _render(blob, info, seed, h)
    return ei.value.code


@pytest.mark.parametrize("name", F.NAMES)
def test_fixture_paths_render_from_blobs(name):
    """Every (hash, kind, string) of the golden fixtures, from the blob of the side the kind selects."""
    n = 0
    for pname, a, b, e in F.load(name):
        if not e["paths"]:
            continue
        sides = {}
        for h, k, want in e["paths"]:
            if (k & 3) == G.PATH_STATUS_ABSENT:
                continue
            doc = a if (k & 3) == G.PATH_REMOVED else b
            if id(doc) not in sides:
                info, blob = G.encode_object_host(doc, seed=e["seed"])
                assert info["status"] == G.TOK_OK, (pname, info)
                sides[id(doc)] = (info, blob)
            info, blob = sides[id(doc)]
            assert _render(blob, info, e["seed"], h) == want.encode("utf-8"), (pname, want)
            n += 1
    assert n > 0


def test_fixture_entry_count():
    """714 pairs, 2,939 path entries over the five fixtures: the population the renderer is pinned to."""
    pairs = [p for name in F.NAMES for p in F.load(name)]
    assert len(pairs) == 714
    assert sum(len(e["paths"]) for *_, e in pairs) == 2939


@pytest.mark.parametrize("name,doc", PC.EDGE_DOCS, ids=[n for n, _ in PC.EDGE_DOCS])
@pytest.mark.parametrize("seed", [0, 9])
def test_edge_objects(name, doc, seed):
    info, blob = G.encode_object_host(doc, seed=seed)
    assert info["status"] == G.TOK_OK, info
    paths = PC.doc_paths(doc)
    assert len(paths) == info["n_tab"]
    for p in paths:
        assert _render(blob, info, seed, O.path_hash(p, seed) & 0xFFFFFFFF) == PC.rendered(p), p


def test_edge_expectations_cover_the_rules():
    """The cases the issue names are really in the edge set (a changed generator must not drop them)."""
    texts = {PC.rendered(p) for _n, doc in PC.EDGE_DOCS for p in PC.doc_paths(doc)}
    for want in (b"a", b"x.", b"", b"spec.", b"spec..", b"spec.a.b", b"spec.[0]", b"spec.a.b", b"[0]", b"[1].",
                 b"spec.items_[9]", b"spec.items_[10]", b"spec.items_[999]", b"spec.items_[1023]",
                 "spec.é.日".encode(), ("spec." + PC.LONG_KEY + ".x[1]").encode()):
        assert want in texts, want
    deep = [p for p in PC.doc_paths(dict(PC.EDGE_DOCS)["deep-40"])]
    assert max(len(p) for p in deep) >= 41
    assert PC.doc_paths(dict(PC.EDGE_DOCS)["utf8-raw"]) == PC.doc_paths(dict(PC.EDGE_DOCS)["utf8-escaped"])


def test_empty_object_has_no_paths():
    info, blob = G.encode_object_host(PC.EMPTY_DOC)
    assert info["status"] == G.TOK_OK and info["n_tab"] == 0
    assert _code(blob, info, 0, 0x1234) == G.E_NOTFOUND
    assert _code(blob, info, 0, 0) == G.E_NOTFOUND  # the root itself is no entry


def test_reduced_width_nonzero_seed():
    """path_hash_bits=16 under a non-zero seed: the root is the seed, the hashes are cut to 16 bits."""
    doc = dict(PC.EDGE_DOCS)["odd-keys"]
    for seed in range(1, 256):
        info, blob = G.encode_object_host(doc, seed=seed, path_hash_bits=16)
        if info["status"] == G.TOK_OK:
            break
    assert info["status"] == G.TOK_OK
    for p in PC.doc_paths(doc):
        assert _render(blob, info, seed, O.path_hash(p, seed) & 0xFFFF) == PC.rendered(p), p
    with pytest.raises(G.GpuDiffError):  # the unmasked hash is not an entry (1 in 65,536 that it is: not this one)
        _render(blob, info, seed, O.path_hash(PC.doc_paths(doc)[0], seed) | (1 << 40))


# ---------------------------------------------------------------- hand-built tables
def test_largest_index():
    blob, info = PC.make_blob([(10, 3, ("K", b"spec")), (20, 10, ("I", 4294967295)), (30, 20, ("I", 0))])
    assert _render(blob, info, 3, 20) == b"spec[4294967295]"
    assert _render(blob, info, 3, 30) == b"spec[4294967295][0]"


def _chain(n, seed=0, first=1000):
    return [(first + i, (first + i - 1) if i else seed, ("K", b"k")) for i in range(n)]


def test_chain_lengths():
    """255 steps render; 256 is the limit; 257 is unresolved."""
    for n, ok in ((255, True), (256, True), (257, False)):
        blob, info = PC.make_blob(_chain(n))
        if ok:
            assert _render(blob, info, 0, 1000 + n - 1) == b".".join([b"k"] * n)
        else:
            assert _code(blob, info, 0, 1000 + n - 1) == G.E_NOTFOUND
        assert _render(blob, info, 0, 1000) == b"k"


def test_absent_parent_and_cycle_end_unresolved():
    blob, info = PC.make_blob([(10, 0, ("K", b"a")), (20, 99, ("K", b"orphan")), (30, 20, ("I", 1))])
    assert _render(blob, info, 0, 10) == b"a"
    assert _code(blob, info, 0, 20) == G.E_NOTFOUND
    assert _code(blob, info, 0, 30) == G.E_NOTFOUND
    blob, info = PC.make_blob([(10, 20, ("K", b"a")), (20, 10, ("K", b"b")), (30, 30, ("I", 2)), (40, 0, ("K", b"c"))])
    for h in (10, 20, 30):  # a two-node cycle, a self-parent: must end, not loop
        assert _code(blob, info, 0, h) == G.E_NOTFOUND
    assert _render(blob, info, 0, 40) == b"c"


def test_key_outside_the_key_area_is_unresolved():
    blob, info = PC.make_blob([(10, 0, ("RAW", (5 << 32) | 1000)), (20, 0, ("RAW", (0x7FFFFFFF << 32) | 0xFFFFFFF0)),
                               (30, 0, ("K", b"ok"))])
    assert _code(blob, info, 0, 10) == G.E_NOTFOUND
    assert _code(blob, info, 0, 20) == G.E_NOTFOUND
    assert _render(blob, info, 0, 30) == b"ok"


def test_no_table_and_bad_info():
    blob, info = PC.make_blob([(10, 0, ("K", b"a"))])
    none = dict(info, n_tab=G.TAB_NONE)
    assert _code(blob, none, 0, 10) == G.E_STATE
    assert _code(blob, dict(info, n_tab=1000), 0, 10) == G.E_INVAL  # the table would not fit the blob
    assert _code(blob, dict(info, spec_l=1 << 20), 0, 10) == G.E_INVAL


def test_capacity_reports_the_length():
    blob, info = PC.make_blob([(10, 0, ("K", b"spec")), (20, 10, ("K", b"replicas"))])
    ci = G.ObjInfo(**info)
    n = C.c_size_t(77)
    buf = C.create_string_buffer(b"#" * 32, 32)
    f = G.lib().gpudiff_render_path_from_blob
    assert f(blob, C.byref(ci), 0, 20, C.cast(buf, C.c_void_p), 12, C.byref(n)) == G.E_CAPACITY
    assert n.value == 13 and buf.raw == b"#" * 32  # nothing written
    assert f(blob, C.byref(ci), 0, 20, C.cast(buf, C.c_void_p), 13, C.byref(n)) == G.OK
    assert n.value == 13 and buf.raw == b"spec.replicas" + b"#" * 19  # no terminator
    assert f(blob, C.byref(ci), 0, 21, C.cast(buf, C.c_void_p), 32, C.byref(n)) == G.E_NOTFOUND and n.value == 0
