"""The request target: the model the target descriptors are tested against -- TEST INFRASTRUCTURE ONLY.

Controller.process reads ``meta.GetNamespace(), meta.GetName()`` (pkg/syncer/syncer.go:310) before anything else.
Restated from the published algorithm of the apimachinery fork pinned at go.mod:33 (third-party, not vendored: the
same status as oracle/upsert_oracle.py):

* ``GetName()`` / ``GetNamespace()`` = ``NestedString(obj, "metadata", field)``: the value when the root has a
  ``metadata`` member that is a map, that map has the member, and the member is a string; else ``""``.
* The object is decoded with the oracle's Go rules: the last of duplicate keys wins, keys are compared decoded.

The descriptor says where the two values stand in the body the engine renders: the span is found by marshalling
with the write-path model (oracle/upsert_oracle.py) member by member.
"""
from __future__ import annotations

from typing import Optional, Tuple

from oracle import upsert_oracle as U
from oracle.gpudiff_oracle import DecodeError, go_json_decode
from tests.update_body_model import _deep, _key, _transformed

TGT_NAME, TGT_NAME_ESC, TGT_NS, TGT_NS_ESC = 0x1, 0x2, 0x4, 0x8
FIELDS = ("name", "namespace")
NOT_GROUPED = 0xFFFFFFFF


def _nested_string(obj, field: str) -> bytes:
    md = obj.get("metadata")
    v = md.get(field) if isinstance(md, dict) else None
    return v.encode("utf-8") if isinstance(v, str) else b""


def target_strings(doc: bytes) -> Optional[Tuple[bytes, bytes]]:
    """(GetNamespace(), GetName()) of the decoded document as bytes; None on a Go decode error."""
    return _deep(_target_strings, doc)


def _target_strings(doc: bytes):
    try:
        obj = go_json_decode(doc)
    except DecodeError:
        return None
    return _nested_string(obj, "namespace"), _nested_string(obj, "name")


def descriptor(doc: bytes, mode: int):
    """((name_off, ns_off), (name_len, ns_len), flags) of the body the engine renders for doc, in canonical form;
    None on a Go decode error."""
    return _deep(_descriptor, doc, mode)


def _descriptor(doc: bytes, mode: int):
    obj = _transformed(doc, mode)
    if obj is None:
        return None
    off, ln, flags = [0, 0], [0, 0], 0
    md = obj.get("metadata")
    if not isinstance(md, dict):
        return (0, 0), (0, 0), 0
    # the metadata map's '{': the root's members before it, each with its comma, then the key and the colon
    pos = 1
    for k in sorted(obj.keys(), key=_key):
        if k == "metadata":
            break
        pos += len(U.go_marshal(k)) + 1 + len(U.go_marshal(obj[k])) + 1
    pos += len(b'"metadata":') + 1
    for i, k in enumerate(sorted(md.keys(), key=_key)):
        pos += (1 if i else 0) + len(U.go_marshal(k)) + 1
        text = U.go_marshal(md[k])
        if k in FIELDS and isinstance(md[k], str):
            f = FIELDS.index(k)
            off[f], ln[f] = pos + 1, len(text) - 2
            flags |= (TGT_NAME | (TGT_NAME_ESC if b"\\" in text else 0)) << (2 * f)
        pos += len(text)
    return tuple(off), tuple(ln), flags


def namespaces(keys, cluster_ids=None, skip=None):
    """gpudiff_targets_namespaces as a dictionary: keys[w] = the write's rendered namespace bytes, or None for a write
    without a body.  (group_of, first)."""
    groups, group_of, first = {}, [], []
    for w, key in enumerate(keys):
        if key is None or (skip is not None and skip[w]):
            group_of.append(NOT_GROUPED)
            continue
        g = groups.setdefault((int(cluster_ids[w]) if cluster_ids is not None else 0, bytes(key)), len(groups))
        if g == len(first):
            first.append(w)
        group_of.append(g)
    return group_of, first
