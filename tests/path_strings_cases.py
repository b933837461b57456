"""Shared by tests/test_path_strings_host.py and tests/test_gpu_path_strings.py: the edge objects of the
path renderer (pathstr.h) as raw JSON documents, the oracle's expectations for them, and hand-built path
tables the encoders cannot produce."""
import json
import struct

from kcp_amd import gpudiff as G
from oracle import gpudiff_oracle as O


def _J(o) -> bytes:
    return json.dumps(o, separators=(",", ":"), ensure_ascii=False).encode()


def _deep(n):
    o = {"leaf": [1, {"z": "end"}]}
    for i in range(n):
        o = {"k%d" % i: o} if i % 3 else [o]
    return o


LONG_KEY = "L" * 300

# (name, document bytes): every key shape the empty-prefix rule, the index digits and the walk depend on
EDGE_DOCS = [
    ("odd-keys", _J({"spec": {"": 1, ".": 2, "a.b": 3, "[0]": 4, "a": {"b": 5}}, "status": {"": {"": 0}, ".": [7]}})),
    ("long-key", _J({"spec": {LONG_KEY: {"x": [0, 1]}, "y": 2}})),
    ("utf8-raw", b'{"spec":{"\xc3\xa9":{"\xe6\x97\xa5":1},"caf\xc3\xa9":[2]}}'),
    ("utf8-escaped", b'{"spec":{"\\u00e9":{"\\u65e5":1},"caf\\u00e9":[2]}}'),
    # the three empty-prefix cases: ("", "a") -> "a"; ("x", "") -> "x."; ("",) -> ""
    ("empty-head", _J({"": {"a": 1, "": {"": 2, "b": [3]}}, "x": {"": 4, "y": {"": 5}}})),
    ("empty-only", _J({"": 1})),
    ("empty-list", _J({"": [1, {"": 2}], "spec": [[[0]]]})),
    ("list-1024", _J({"spec": {"items_": list(range(1024))}, "status": {"l": [{"i": i} for i in range(12)]}})),
    ("deep-40", _J({"spec": _deep(40)})),
    ("labels", _J({"metadata": {"labels": {"": "a", "app.kubernetes.io/name": "b"}, "annotations": {"x.y": "z"}},
                   "spec": {"r": 1}})),
]
EMPTY_DOC = b"{}"


def doc_paths(doc: bytes):
    """The oracle's region leaves of a document and all their ancestors (what a path table names)."""
    obj = O.informer_decode(doc)
    leaves = set(O.spec_leaves(obj)) | set(O.status_leaves(obj))
    return sorted({p[:k] for p in leaves for k in range(1, len(p) + 1)}, key=repr)


def rendered(path) -> bytes:
    return O.render_path(path).encode("utf-8")


def mutate_edge(doc: bytes) -> bytes:
    """A second version of an edge document: every leaf changed, one path removed, one added."""
    obj = O.informer_decode(doc)

    def bump(x):
        if type(x) is dict and x:
            return {k: bump(v) for k, v in x.items()}
        if type(x) is list and x:
            return [bump(v) for v in x]
        return "changed" if type(x) is not str else x + "!"
    out = bump(obj)
    meta = out.get("metadata")  # label values stay strings (they are), the rest is free
    if "spec" in out and type(out["spec"]) is dict:
        k = sorted(out["spec"])[0]
        del out["spec"][k]
        out["spec"]["added" + k] = {"": [1, 2]}
    if meta is not None:
        out["metadata"] = meta
    return _J(out)


# ---------------------------------------------------------------- hand-built tables
TAB_INDEX = G.TAB_INDEX


def make_blob(nodes, key_pad: int = 0):
    """A blob with empty segments and the given table: nodes = [(hash, parent hash, ('K', bytes) | ('I', index) |
    ('RAW', cs word))], any order.  Returns (blob bytes, info dict)."""
    nodes = sorted(nodes, key=lambda t: t[0])
    n = len(nodes)
    keys = bytearray()
    cs = []
    for _h, _ph, (kind, c) in nodes:
        if kind == "I":
            cs.append(TAB_INDEX | c)
        elif kind == "RAW":
            cs.append(c)
        else:
            cs.append((len(c) << 32) | len(keys))
            keys += c
    keys += b"\0" * key_pad
    raw = struct.pack("<%dQ" % n, *[h for h, _, _ in nodes]) + struct.pack("<%dQ" % n, *[ph for _, ph, _ in nodes]) \
        + struct.pack("<%dQ" % n, *cs) + bytes(keys)
    raw += b"\0" * (-len(raw) % 128)
    info = dict(status=0, oflags=0, spec_l=0, spec_ar=0, stat_l=0, stat_ar=0, off=0, bytes=len(raw), n_tab=n,
                reserved=0)
    return raw, info
