"""The model GPUDIFF_OPT_PATH_VALUES is pinned to, from the oracle alone: for every changed path of a pair
(oracle.gpudiff_oracle.diff_pair), the type tag and the JSON text of A's and B's leaf.  The leaves are the oracle's
(spec_leaves / status_leaves: path -> (tag, canonical bytes)); the text of (tag, bytes) is the write path's encoder
as oracle/upsert_oracle.py restates it (go_float, _go_string)."""
import struct

from oracle import gpudiff_oracle as O
from oracle import upsert_oracle as U

ABSENT = 0xFF  # GPUDIFF_VALUE_ABSENT
_LITERAL = {O.TAG_NULL: b"null", O.TAG_FALSE: b"false", O.TAG_TRUE: b"true", O.TAG_EOBJ: b"{}", O.TAG_EARR: b"[]"}
REGION_BIT = 0x80


def text_of(tag: int, raw: bytes) -> bytes:
    """The JSON text of one canonical leaf value."""
    if tag in _LITERAL:
        assert raw == b""
        return _LITERAL[tag]
    if tag == O.TAG_INT:
        return str(struct.unpack("<q", raw)[0]).encode()
    if tag == O.TAG_FLOAT:
        return U.go_float(struct.unpack("<d", raw)[0])
    assert tag == O.TAG_STR
    out = bytearray()
    U._go_string(raw.decode("utf-8"), out)
    return bytes(out)


def _region_leaves(doc: bytes):
    obj = O.informer_decode(doc)
    return O.spec_leaves(obj), O.status_leaves(obj)


def region_leaves(doc: bytes):
    """(spec leaves, status leaves) of one document: path -> (tag, canonical bytes)."""
    if O._nesting_bound(doc) > 500:  # the recursive restatement needs a big stack for these, as diff_pair does
        return O._on_big_stack(_region_leaves, doc)
    return _region_leaves(doc)


def _side(leaves, path):
    v = leaves.get(path)
    return (ABSENT, None) if v is None else (v[0], text_of(*v))


def values_of(a_json: bytes, b_json: bytes, r=None, hash_bits: int = O.PATH_HASH_BITS):
    """[(hash, kind | region bit, old_tag, old_text | None, new_tag, new_text | None)] of one pair, in result order.
    r: the pair's diff_pair result, when the caller has it."""
    r = O.diff_pair(a_json, b_json, hash_bits) if r is None else r
    if not r["paths"]:
        return []
    la, lb = region_leaves(a_json), region_leaves(b_json)
    out = []
    for h, region, kind, p in r["paths"]:
        k = kind | (REGION_BIT if region else 0)
        if kind == O.KIND_STATUS_ABSENT:
            out.append((h, k, ABSENT, None, ABSENT, None))
            continue
        old, new = _side(la[1 if region else 0], p), _side(lb[1 if region else 0], p)
        assert (old[0] == ABSENT) == (kind == O.KIND_ADDED), (p, kind)
        assert (new[0] == ABSENT) == (kind == O.KIND_REMOVED), (p, kind)
        out.append((h, k) + old + new)
    return out
