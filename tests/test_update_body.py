"""The Update body on the host (no GPU): the resourceVersion splice descriptor the Go-exact marshaller records
with each body, gpudiff_splice_resource_version, and gpudiff_update_body_host (the direct marshal), against
known answers stating the Go output and against the model (tests/update_body_model.py) over the write path's
corpus."""
import pytest

from kcp_amd import gpudiff as G
from tests import update_body_model as M
from tests import upsert_cases as UC

I, L, T, W = G.RV_INSERT, G.RV_LEAD, G.RV_TRAIL, G.RV_WRAP
OWN_REF = b'"ownerReferences":[{"name":"own"}]'
KEPT_REF = b'"ownerReferences":[{"apiVersion":"","kind":"","name":"own","uid":""}]'

# (doc, mode, rv, the body the engine renders, the Update body Go sends, off, form)
KNOWN = [
    (b'{"metadata":{"name":"a","uid":"u","resourceVersion":"1"},"kind":"K"}', UC.SPEC, b"42",
     b'{"kind":"K","metadata":{"name":"a"}}\n',
     b'{"kind":"K","metadata":{"name":"a","resourceVersion":"42"}}\n', 34, I | L),
    (b'{"metadata":{"uid":"u"}}', UC.SPEC, b"42",
     b'{"metadata":{}}\n', b'{"metadata":{"resourceVersion":"42"}}\n', 13, I),
    (b'{"b":1,"a":2}', UC.SPEC, b"42",
     b'{"a":2,"b":1}\n', b'{"a":2,"b":1,"metadata":{"resourceVersion":"42"}}\n', 12, I | L | W),
    (b'{}', UC.STATUS, b"42", b'{}\n', b'{"metadata":{"resourceVersion":"42"}}\n', 1, I | W),
    (b'{"spec":{}}', UC.SPEC, b"42",
     b'{"spec":{}}\n', b'{"metadata":{"resourceVersion":"42"},"spec":{}}\n', 1, I | T | W),
    (b'{"spec":{},"kind":"K"}', UC.SPEC, b"42",
     b'{"kind":"K","spec":{}}\n', b'{"kind":"K","metadata":{"resourceVersion":"42"},"spec":{}}\n', 11, I | L | W),
    # metadata present and not a map: SetNestedField fails, the accessor drops the error
    (b'{"metadata":null,"x":1}', UC.SPEC, b"42", b'{"metadata":null,"x":1}\n', b'{"metadata":null,"x":1}\n', 0, 0),
    (b'{"metadata":"s"}', UC.STATUS, b"42", b'{"metadata":"s"}\n', b'{"metadata":"s"}\n', 0, 0),
    (b'{"metadata":[1]}', UC.SPEC, b"42", b'{"metadata":[1]}\n', b'{"metadata":[1]}\n', 0, 0),
    # between name and selfLink
    (b'{"metadata":{"selfLink":"s","resourceVersion":"1","name":"n"}}', UC.STATUS, b"42",
     b'{"metadata":{"name":"n","selfLink":"s"}}\n',
     b'{"metadata":{"name":"n","resourceVersion":"42","selfLink":"s"}}\n', 23, I | L),
    # nothing visible precedes (uid is hidden), zz follows
    (b'{"metadata":{"resourceVersion":"1","uid":"u","zz":1}}', UC.SPEC, b"42",
     b'{"metadata":{"zz":1}}\n', b'{"metadata":{"resourceVersion":"42","zz":1}}\n', 13, I | T),
    # spec mode removes the owner reference the owned-by label names: it is no preceding member
    (b'{"metadata":{' + UC.OWN + b',' + OWN_REF + b',"resourceVersion":"1"}}', UC.SPEC, b"42",
     b'{"metadata":{' + UC.OWN + b'}}\n',
     b'{"metadata":{' + UC.OWN + b',"resourceVersion":"42"}}\n', len(b'{"metadata":{' + UC.OWN), I | L),
    # ... status mode keeps it as it is
    (b'{"metadata":{' + UC.OWN + b',' + OWN_REF + b',"resourceVersion":"1"}}', UC.STATUS, b"42",
     b'{"metadata":{' + UC.OWN + b',' + OWN_REF + b'}}\n',
     b'{"metadata":{' + UC.OWN + b',' + OWN_REF + b',"resourceVersion":"42"}}\n',
     len(b'{"metadata":{' + UC.OWN + b',' + OWN_REF), I | L),
    # ... and without the label the reference stays, normalized: the member goes behind the normalized text
    (b'{"metadata":{' + OWN_REF + b',"resourceVersion":"1"}}', UC.SPEC, b"42",
     b'{"metadata":{' + KEPT_REF + b'}}\n',
     b'{"metadata":{' + KEPT_REF + b',"resourceVersion":"42"}}\n', len(b'{"metadata":{' + KEPT_REF), I | L),
    # metadata emptied by the spec transform, not by the status one
    (b'{"metadata":{"ownerReferences":[],"resourceVersion":"1"}}', UC.SPEC, b"42",
     b'{"metadata":{}}\n', b'{"metadata":{"resourceVersion":"42"}}\n', 13, I),
    (b'{"metadata":{"ownerReferences":[],"resourceVersion":"1"}}', UC.STATUS, b"42",
     b'{"metadata":{"ownerReferences":[]}}\n',
     b'{"metadata":{"ownerReferences":[],"resourceVersion":"42"}}\n', 33, I | L),
    # a nested metadata.resourceVersion is no business of SetResourceVersion: the root gets the wrap
    (b'{"spec":{"metadata":{"resourceVersion":"9"}}}', UC.SPEC, b"42",
     b'{"spec":{"metadata":{"resourceVersion":"9"}}}\n',
     b'{"metadata":{"resourceVersion":"42"},"spec":{"metadata":{"resourceVersion":"9"}}}\n', 1, I | T | W),
    # keys that share the literal's first eight bytes
    (b'{"metadata":{"resources":1,"resourceV":2,"resourceVersion2":3,"resourceVersio":4,"resourceversion":5}}',
     UC.STATUS, b"42",
     b'{"metadata":{"resourceV":2,"resourceVersio":4,"resourceVersion2":3,"resources":1,"resourceversion":5}}\n',
     b'{"metadata":{"resourceV":2,"resourceVersio":4,"resourceVersion":"42","resourceVersion2":3,"resources":1,'
     b'"resourceversion":5}}\n', len(b'{"metadata":{"resourceV":2,"resourceVersio":4'), I | L),
    # rv is escaped as Go escapes any string: HTML-safe, invalid UTF-8 as the escape of U+FFFD
    (b'{"metadata":{"name":"a"}}', UC.SPEC, b'a<b&"\\',
     b'{"metadata":{"name":"a"}}\n',
     b'{"metadata":{"name":"a","resourceVersion":"a\\u003cb\\u0026\\"\\\\"}}\n', 23, I | L),
    (b'{"metadata":{"name":"a"}}', UC.SPEC, b"\xff",
     b'{"metadata":{"name":"a"}}\n', b'{"metadata":{"name":"a","resourceVersion":"\\ufffd"}}\n', 23, I | L),
    (b'{"metadata":{"name":"a"}}', UC.SPEC, b"\xe2\x80\xa8\xed\xa0\x80\xc3\xa9\xe2\x80",
     b'{"metadata":{"name":"a"}}\n',
     b'{"metadata":{"name":"a","resourceVersion":"\\u2028\\ufffd\\ufffd\\ufffd\xc3\xa9\\ufffd\\ufffd"}}\n', 23, I | L),
    # rv == "": RemoveNestedField, which the body has already seen
    (b'{"metadata":{"name":"a","resourceVersion":"1"}}', UC.STATUS, b"",
     b'{"metadata":{"name":"a"}}\n', b'{"metadata":{"name":"a"}}\n', 23, I | L),
]


@pytest.mark.parametrize("k", range(len(KNOWN)))
def test_known_answers(k):
    doc, mode, rv, body, update, off, form = KNOWN[k]
    assert M.update_body(doc, mode, rv) == update
    assert M.splice_point(doc, mode) == (off, form)
    assert M.splice(body, off, form, rv) == update
    assert G.upsert_body_host_rv(doc, mode) == (body, off, form)
    assert G.upsert_body_host(doc, mode) == body
    assert G.update_body_host(doc, mode, rv) == update
    assert G.splice_resource_version(body, off, form, rv) == update


RVS = (b"1", b"987654321", b'x<"y')


def _corpus():
    return [k[1] for k in UC.KAT] + UC.fixture_docs() + UC.boundary_docs() + UC.synthetic_docs()


@pytest.mark.parametrize("mode", [UC.SPEC, UC.STATUS])
def test_corpus(mode):
    """splice(body_host, off, form, rv) == update_body_host == the model, the host descriptor equals the model's,
    and decode errors stay decode errors."""
    n_err = 0
    for d in _corpus():
        host = G.upsert_body_host_rv(d, mode)
        want_pt = M.splice_point(d, mode)
        if want_pt is None:
            n_err += 1
            assert host is None, d[:200]
            for rv in RVS:
                assert G.update_body_host(d, mode, rv) is None and M.update_body(d, mode, rv) is None
            continue
        body, off, form = host
        assert (off, form) == want_pt, d[:200]
        for rv in RVS:
            want = M.update_body(d, mode, rv)
            assert G.update_body_host(d, mode, rv) == want, (rv, d[:200])
            assert G.splice_resource_version(body, off, form, rv) == want, (rv, d[:200])
    assert n_err > 0


def test_splice_argument_checks():
    """GPUDIFF_E_INVAL for an off outside the body or an unknown form bit; GPUDIFF_E_CAPACITY with the length set
    when the result does not fit; rv_len == 0 or GPUDIFF_RV_NONE copy the body."""
    import ctypes as C
    L_ = G.lib()
    body = b'{"metadata":{}}\n'
    n = C.c_size_t()
    out = C.create_string_buffer(256)

    def call(off, form, rv=b"42", cap=256):
        return L_.gpudiff_splice_resource_version(body, len(body), off, form, rv, len(rv),
                                                  C.cast(out, C.c_void_p), cap, C.byref(n))
    assert call(13, I) == G.OK and out.raw[:n.value] == b'{"metadata":{"resourceVersion":"42"}}\n'
    for off, form in ((len(body), I), (len(body) + 1, I), (0, I), (0xFFFFFFFF, I | L), (13, 0x10), (13, I | 0x80),
                      (13, L), (13, W | T), (len(body) + 1, G.RV_NONE)):
        assert call(off, form) == G.E_INVAL, (off, form)
    assert call(13, I, cap=10) == G.E_CAPACITY and n.value == len(body) + len(b'"resourceVersion":"42"')
    assert call(13, I, rv=b"") == G.OK and out.raw[:n.value] == body
    assert call(0, G.RV_NONE) == G.OK and out.raw[:n.value] == body
    assert L_.gpudiff_splice_resource_version(body, len(body), 13, I, b"42", 2, None, 0, C.byref(n)) == G.E_CAPACITY
    assert L_.gpudiff_splice_resource_version(body, len(body), 13, I, b"42", 2, None, 0, None) == G.E_INVAL


def test_update_body_host_argument_checks():
    import ctypes as C
    L_ = G.lib()
    n = C.c_size_t()
    assert L_.gpudiff_update_body_host(b"{}", 2, 2, b"1", 1, None, 0, C.byref(n)) == G.E_INVAL  # no such mode
    assert L_.gpudiff_update_body_host(b"{}", 2, 0, b"1", 1, None, 0, C.byref(n)) == G.E_CAPACITY
    assert n.value == len(b'{"metadata":{"resourceVersion":"1"}}\n')
    assert L_.gpudiff_update_body_host(b"[", 1, 0, b"1", 1, None, 0, C.byref(n)) == G.E_DECODE and n.value == 0
