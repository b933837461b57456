"""The Update body: the model the resourceVersion splice is tested against -- TEST INFRASTRUCTURE ONLY.

Every steady-state write sets the live object's resourceVersion on the body the engine rendered
(pkg/syncer/statussyncer.go:50-57, specsyncer.go:116-124).  Restated from the published algorithm of the
apimachinery fork pinned at go.mod:33 (third-party, not vendored: the same status as oracle/upsert_oracle.py):

* ``SetResourceVersion("")`` = ``RemoveNestedField(obj, "metadata", "resourceVersion")``: the body is the one the
  transform already gives.
* ``SetResourceVersion(rv)`` = ``SetNestedField(obj, rv, "metadata", "resourceVersion")``: metadata a map: the
  member is set; the metadata key absent: a new map ``{"resourceVersion": rv}`` is created under it; metadata
  present and not a map: SetNestedField returns an error the accessor drops, the object is unchanged.
* The body is ``json.NewEncoder(w).Encode(obj.Object)``: keys sorted by bytes, rv escaped as any Go string
  (HTML-safe; a byte utf8.DecodeRune rejects becomes the six characters of the escape of U+FFFD).

``rv`` is a Go string, i.e. bytes: it need not be valid UTF-8.
"""
from __future__ import annotations

from typing import Optional, Tuple

from oracle import upsert_oracle as U
from oracle.gpudiff_oracle import DecodeError, _nesting_bound, _on_big_stack, go_json_decode

RV_NONE, RV_INSERT, RV_LEAD, RV_TRAIL, RV_WRAP = 0x0, 0x1, 0x2, 0x4, 0x8

_HEX = b"0123456789abcdef"


def _rune_len(s: bytes, i: int) -> int:
    """utf8.DecodeRune at s[i] (a byte >= 0x80): the sequence's length, 0 for RuneError of width 1."""
    c = s[i]
    lo, hi = 0x80, 0xBF
    if 0xC2 <= c <= 0xDF:
        need = 1
    elif 0xE0 <= c <= 0xEF:
        need = 2
        lo = 0xA0 if c == 0xE0 else lo
        hi = 0x9F if c == 0xED else hi
    elif 0xF0 <= c <= 0xF4:
        need = 3
        lo = 0x90 if c == 0xF0 else lo
        hi = 0x8F if c == 0xF4 else hi
    else:
        return 0
    if i + need >= len(s) or not lo <= s[i + 1] <= hi:
        return 0
    if any(not 0x80 <= s[i + k] <= 0xBF for k in range(2, need + 1)):
        return 0
    return need + 1


def go_string_bytes(s: bytes) -> bytes:
    """encodeState.string(s, escapeHTML=true) of Go 1.16 over a Go string (bytes)."""
    out = bytearray(b'"')
    i = 0
    while i < len(s):
        c = s[i]
        if c < 0x80:
            if c in (0x22, 0x5C):
                out += b"\\" + bytes([c])
            elif c == 0x0A:
                out += b"\\n"
            elif c == 0x0D:
                out += b"\\r"
            elif c == 0x09:
                out += b"\\t"
            elif c < 0x20 or c in (0x3C, 0x3E, 0x26):
                out += b"\\u00" + bytes([_HEX[c >> 4], _HEX[c & 15]])
            else:
                out.append(c)
            i += 1
            continue
        n = _rune_len(s, i)
        if n == 0:
            out += b"\\ufffd"
            i += 1
        elif s[i:i + 3] in (b"\xe2\x80\xa8", b"\xe2\x80\xa9"):
            out += b"\\u202" + (b"8" if s[i + 2] == 0xA8 else b"9")
            i += 3
        else:
            out += s[i:i + n]
            i += n
    out.append(0x22)
    return bytes(out)


def _key(k: str) -> bytes:
    return k.encode("utf-8")


def _marshal_map(d: dict, raw: dict) -> bytes:
    """go_marshal of a map whose members named in `raw` are already text."""
    out = bytearray(b"{")
    for i, k in enumerate(sorted(d.keys(), key=_key)):
        if i:
            out.append(0x2C)
        out += U.go_marshal(k) + b":"
        out += raw[k] if k in raw else U.go_marshal(d[k])
    out.append(0x7D)
    return bytes(out)


def _transformed(doc: bytes, mode: int) -> Optional[dict]:
    try:
        return U.transform(go_json_decode(doc), mode)
    except DecodeError:
        return None


def _deep(fn, doc, *args):
    """fn(doc, *args), on a big stack when the document nests as deep as Go's 10000-level limit allows."""
    if _nesting_bound(doc) > 1000:
        return _on_big_stack(fn, doc, *args)
    return fn(doc, *args)


def update_body(doc: bytes, mode: int, rv: bytes) -> Optional[bytes]:
    """decode -> transform -> SetResourceVersion(rv) -> marshal + newline; None on a Go decode error."""
    return _deep(_update_body, doc, mode, rv)


def _update_body(doc: bytes, mode: int, rv: bytes) -> Optional[bytes]:
    obj = _transformed(doc, mode)
    if obj is None:
        return None
    md = obj.get("metadata")
    if not rv or ("metadata" in obj and not isinstance(md, dict)):
        return U.go_marshal(obj) + b"\n"
    md = dict(md) if isinstance(md, dict) else {}
    md["resourceVersion"] = None
    obj = dict(obj)
    obj["metadata"] = None
    return _marshal_map(obj, {"metadata": _marshal_map(md, {"resourceVersion": go_string_bytes(rv)})}) + b"\n"


def splice_point(doc: bytes, mode: int) -> Optional[Tuple[int, int]]:
    """The canonical (off, form) of the body the engine renders for doc, from the decoded tree: a visible member
    precedes in the container -> LEAD, off just past its value; none precedes and one follows -> TRAIL, off just
    past the container's '{'; neither -> no comma, off just past '{'.  None on a Go decode error."""
    return _deep(_splice_point, doc, mode)


def _splice_point(doc: bytes, mode: int) -> Optional[Tuple[int, int]]:
    obj = _transformed(doc, mode)
    if obj is None:
        return None
    if "metadata" in obj and not isinstance(obj["metadata"], dict):
        return 0, RV_NONE
    wrap = "metadata" not in obj
    cont, name, start = (obj, "metadata", 0) if wrap else (obj["metadata"], "resourceVersion", None)
    if start is None:
        # the metadata map's '{': the root's members before it, each with its comma, then the key and the colon
        start = 1
        for k in sorted(obj.keys(), key=_key):
            if k == "metadata":
                break
            start += len(U.go_marshal(k)) + 1 + len(U.go_marshal(obj[k])) + 1
        start += len(b'"metadata":')
    form = RV_INSERT | (RV_WRAP if wrap else 0)
    keys = sorted(cont.keys(), key=_key)
    before = [k for k in keys if _key(k) < _key(name)]
    if not before:
        return start + 1, form | (RV_TRAIL if keys else 0)
    # '{', then the preceding members joined by commas
    off = start + 1 + sum(len(U.go_marshal(k)) + 1 + len(U.go_marshal(cont[k])) for k in before) + len(before) - 1
    return off, form | RV_LEAD


def splice(body: bytes, off: int, form: int, rv: bytes) -> bytes:
    """The Update body from a rendered body and its descriptor."""
    if form == RV_NONE or not rv:
        return body
    member = b'"resourceVersion":' + go_string_bytes(rv)
    if form & RV_WRAP:
        member = b'"metadata":{' + member + b"}"
    text = (b"," if form & RV_LEAD else b"") + member + (b"," if form & RV_TRAIL else b"")
    return body[:off] + text + body[off:]
