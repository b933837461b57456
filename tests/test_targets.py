"""The request target on the host (no GPU): the descriptor the Go-exact marshaller records with each body
(gpudiff_upsert_body_host_targets), gpudiff_target_decode, gpudiff_target_host (the direct decode) and
gpudiff_targets_namespaces, against known answers stating the Go output and against the model
(tests/targets_model.py) over the write path's corpus."""
import ctypes as C

import numpy as np
import pytest

from kcp_amd import gpudiff as G
from tests import targets_model as M
from tests import upsert_cases as UC

N, NE, S, SE = G.TGT_NAME, G.TGT_NAME_ESC, G.TGT_NS, G.TGT_NS_ESC

# (doc, mode, the body the engine renders, the body up to the name's span (None: absent), the name's span,
#  the body up to the namespace's span, the namespace's span, flags, GetNamespace(), GetName())
KNOWN = [
    (b'{"metadata":{"name":"a","uid":"u","resourceVersion":"1"},"kind":"K"}', UC.SPEC,
     b'{"kind":"K","metadata":{"name":"a"}}\n', b'{"kind":"K","metadata":{"name":"', b"a", None, b"", N, b"", b"a"),
    (b'{"metadata":{"namespace":"ns1","name":"n1"}}', UC.STATUS,
     b'{"metadata":{"name":"n1","namespace":"ns1"}}\n', b'{"metadata":{"name":"', b"n1",
     b'{"metadata":{"name":"n1","namespace":"', b"ns1", N | S, b"ns1", b"n1"),
    # uid and resourceVersion leave the body: the spans move with it
    (b'{"metadata":{"uid":"u","namespace":"ns","a":1,"resourceVersion":"9","name":"n"}}', UC.SPEC,
     b'{"metadata":{"a":1,"name":"n","namespace":"ns"}}\n', b'{"metadata":{"a":1,"name":"', b"n",
     b'{"metadata":{"a":1,"name":"n","namespace":"', b"ns", N | S, b"ns", b"n"),
    # present and empty: the flag is set, the offset stands behind the opening quote
    (b'{"metadata":{"name":"","namespace":""}}', UC.SPEC,
     b'{"metadata":{"name":"","namespace":""}}\n', b'{"metadata":{"name":"', b"",
     b'{"metadata":{"name":"","namespace":"', b"", N | S, b"", b""),
    # what Go's encoder escapes: _ESC, and the span decodes to the value
    (b'{"metadata":{"name":"a<b","namespace":"x\\"y\\\\z\xe2\x80\xa8"}}', UC.STATUS,
     b'{"metadata":{"name":"a\\u003cb","namespace":"x\\"y\\\\z\\u2028"}}\n', b'{"metadata":{"name":"', b"a\\u003cb",
     b'{"metadata":{"name":"a\\u003cb","namespace":"', b'x\\"y\\\\z\\u2028', N | NE | S | SE,
     b'x"y\\z\xe2\x80\xa8', b"a<b"),
    (b'{"metadata":{"name":"\\n\\r\\t\\b\\f\\u0001&>"}}', UC.SPEC,
     b'{"metadata":{"name":"\\n\\r\\t\\u0008\\u000c\\u0001\\u0026\\u003e"}}\n', b'{"metadata":{"name":"',
     b"\\n\\r\\t\\u0008\\u000c\\u0001\\u0026\\u003e", None, b"", N | NE, b"", b"\n\r\t\x08\x0c\x01&>"),
    # an input escape that renders clean, a non-ASCII value that renders as its bytes: no _ESC
    (b'{"metadata":{"name":"\\u0061b","namespace":"caf\xc3\xa9"}}', UC.SPEC,
     b'{"metadata":{"name":"ab","namespace":"caf\xc3\xa9"}}\n', b'{"metadata":{"name":"', b"ab",
     b'{"metadata":{"name":"ab","namespace":"', b"caf\xc3\xa9", N | S, b"caf\xc3\xa9", b"ab"),
    # invalid UTF-8 is repaired by the decode (U+FFFD), which the encoder writes as its bytes
    (b'{"metadata":{"name":"a\xffb"}}', UC.SPEC,
     b'{"metadata":{"name":"a\xef\xbf\xbdb"}}\n', b'{"metadata":{"name":"', b"a\xef\xbf\xbdb", None, b"", N, b"",
     b"a\xef\xbf\xbdb"),
    # metadata that is no object: NestedString finds nothing
    (b'{"metadata":null,"x":1}', UC.SPEC, b'{"metadata":null,"x":1}\n', None, b"", None, b"", 0, b"", b""),
    (b'{"metadata":"name"}', UC.STATUS, b'{"metadata":"name"}\n', None, b"", None, b"", 0, b"", b""),
    (b'{"metadata":[{"name":"a"}]}', UC.SPEC, b'{"metadata":[{"name":"a"}]}\n', None, b"", None, b"", 0, b"", b""),
    (b'{"metadata":{}}', UC.SPEC, b'{"metadata":{}}\n', None, b"", None, b"", 0, b"", b""),
    (b'{"kind":"K"}', UC.SPEC, b'{"kind":"K"}\n', None, b"", None, b"", 0, b"", b""),
    # values that are no strings
    (b'{"metadata":{"name":5,"namespace":null}}', UC.SPEC, b'{"metadata":{"name":5,"namespace":null}}\n',
     None, b"", None, b"", 0, b"", b""),
    (b'{"metadata":{"name":{"name":"a"},"namespace":["ns"]}}', UC.STATUS,
     b'{"metadata":{"name":{"name":"a"},"namespace":["ns"]}}\n', None, b"", None, b"", 0, b"", b""),
    # keys are compared byte for byte, without case folding
    (b'{"metadata":{"Name":"x","NAMESPACE":"y","names":"z","namespac":"w","clusterName":"c"}}', UC.SPEC,
     b'{"metadata":{"NAMESPACE":"y","Name":"x","clusterName":"c","names":"z","namespac":"w"}}\n',
     None, b"", None, b"", 0, b"", b""),
    # the last of duplicate keys wins: a later string, a later non-string, a later metadata
    (b'{"metadata":{"name":"a","name":"b"}}', UC.SPEC, b'{"metadata":{"name":"b"}}\n',
     b'{"metadata":{"name":"', b"b", None, b"", N, b"", b"b"),
    (b'{"metadata":{"name":"a","name":5}}', UC.SPEC, b'{"metadata":{"name":5}}\n', None, b"", None, b"", 0, b"", b""),
    (b'{"metadata":{"name":"a"},"metadata":{"namespace":"q"}}', UC.STATUS, b'{"metadata":{"namespace":"q"}}\n',
     None, b"", b'{"metadata":{"namespace":"', b"q", S, b"q", b""),
    # a key that needs unescaping to spell the field's name counts
    (b'{"metadata":{"n\\u0061me":"x","namesp\\u0061ce":"y"}}', UC.SPEC,
     b'{"metadata":{"name":"x","namespace":"y"}}\n', b'{"metadata":{"name":"', b"x",
     b'{"metadata":{"name":"x","namespace":"', b"y", N | S, b"y", b"x"),
    # decoys: a root-level name, spec.metadata.name, an owner reference's name (normalised in spec mode)
    (b'{"name":"r","spec":{"metadata":{"name":"s","namespace":"t"}},"metadata":{"ownerReferences":[{"name":"o"}]}}',
     UC.SPEC,
     b'{"metadata":{"ownerReferences":[{"apiVersion":"","kind":"","name":"o","uid":""}]},"name":"r",'
     b'"spec":{"metadata":{"name":"s","namespace":"t"}}}\n', None, b"", None, b"", 0, b"", b""),
    # ... and removed with the owned-by label, beside a real name
    (b'{"metadata":{' + UC.OWN + b',"ownerReferences":[{"name":"own"}],"name":"real"}}', UC.SPEC,
     b'{"metadata":{' + UC.OWN + b',"name":"real"}}\n', b'{"metadata":{' + UC.OWN + b',"name":"', b"real",
     None, b"", N, b"", b"real"),
]


def _want(k):
    doc, mode, body, npre, nspan, spre, sspan, flags, ns, name = KNOWN[k]
    off = (len(npre) if npre is not None else 0, len(spre) if spre is not None else 0)
    return off, (len(nspan), len(sspan)), flags


@pytest.mark.parametrize("k", range(len(KNOWN)))
def test_known_answers(k):
    doc, mode, body, npre, nspan, spre, sspan, flags, ns, name = KNOWN[k]
    off, ln, fl = _want(k)
    for pre, span in ((npre, nspan), (spre, sspan)):  # the table states the body consistently
        assert pre is None or body[len(pre):len(pre) + len(span) + 1] == span + b'"'
    assert M.descriptor(doc, mode) == (off, ln, fl)
    assert M.target_strings(doc) == (ns, name)
    assert G.upsert_body_host(doc, mode) == body
    assert G.upsert_body_host_targets(doc, mode) == (body, off, ln, fl)
    assert G.target_decode(body, off[0], ln[0]) == name
    assert G.target_decode(body, off[1], ln[1]) == ns
    assert G.target_host(doc) == (ns, name)


def _corpus():
    return [k[1] for k in UC.KAT] + UC.fixture_docs() + UC.boundary_docs() + UC.synthetic_docs()


@pytest.mark.parametrize("mode", [UC.SPEC, UC.STATUS])
def test_corpus(mode):
    """The host descriptor equals the model's, target_decode of each span equals gpudiff_target_host equals the
    model's string, and decode errors stay decode errors."""
    n_err = n_name = n_ns = 0
    for d in _corpus():
        host = G.upsert_body_host_targets(d, mode)
        want = M.descriptor(d, mode)
        strings = M.target_strings(d)
        if want is None:
            n_err += 1
            assert host is None and strings is None and G.target_host(d) is None, d[:200]
            continue
        body, off, ln, fl = host
        assert (off, ln, fl) == want, d[:200]
        assert body == G.upsert_body_host(d, mode)
        got = (G.target_decode(body, off[1], ln[1]), G.target_decode(body, off[0], ln[0]))
        assert got == G.target_host(d) == strings, d[:200]
        n_name += bool(fl & N)
        n_ns += bool(fl & S)
    assert n_err > 0 and n_name > 100 and n_ns > 100


def test_target_decode_errors():
    """GPUDIFF_E_INVAL for a span outside the body or a malformed escape; GPUDIFF_E_CAPACITY with the length set when
    the result does not fit."""
    L_ = G.lib()
    n = C.c_size_t()
    out = C.create_string_buffer(64)

    def call(body, off, ln, cap=64, buf=out):
        return L_.gpudiff_target_decode(body, len(body), off, ln, C.cast(buf, C.c_void_p) if buf else None, cap,
                                        C.byref(n))
    every = b'\\"\\\\\\n\\r\\t\\b\\f\\u00e9\\u2028\\ud83d\\ude00\\ud800x'
    assert call(every, 0, len(every)) == G.OK
    assert out.raw[:n.value] == b'"\\\n\r\t\x08\x0c\xc3\xa9\xe2\x80\xa8\xf0\x9f\x98\x80\xef\xbf\xbdx'
    body = b'{"a":"xy"}\n'
    assert call(body, 6, 2) == G.OK and out.raw[:n.value] == b"xy"
    assert call(body, len(body), 0) == G.OK and n.value == 0
    for off, ln in ((len(body) + 1, 0), (len(body), 1), (6, len(body)), (0xFFFFFFFF, 2), (2, 0xFFFFFFFF)):
        assert call(body, off, ln) == G.E_INVAL, (off, ln)
    for bad in (b"\\", b"ab\\", b"\\x", b"\\/", b"\\u12", b"\\u12G4", b"\\u", b"a\\u00e"):
        assert call(bad, 0, len(bad)) == G.E_INVAL, bad
    assert call(b"ab\\ncd", 0, 6, cap=3) == G.E_CAPACITY and n.value == 5
    assert call(b"ab", 0, 2, cap=0, buf=None) == G.E_CAPACITY and n.value == 2
    assert call(b"", 0, 0, cap=0, buf=None) == G.OK and n.value == 0
    assert L_.gpudiff_target_decode(b"ab", 2, 0, 2, C.cast(out, C.c_void_p), 64, None) == G.E_INVAL


def test_target_host_argument_checks():
    L_ = G.lib()
    nn, sn = C.c_size_t(), C.c_size_t()
    name, ns = C.create_string_buffer(8), C.create_string_buffer(8)
    doc = b'{"metadata":{"name":"abcdef","namespace":"ns"}}'

    def call(d, name_cap, ns_cap):
        return L_.gpudiff_target_host(d, len(d), C.cast(name, C.c_void_p), name_cap, C.byref(nn),
                                      C.cast(ns, C.c_void_p), ns_cap, C.byref(sn))
    assert call(doc, 8, 8) == G.OK and (name.raw[:nn.value], ns.raw[:sn.value]) == (b"abcdef", b"ns")
    assert call(doc, 5, 8) == G.E_CAPACITY and (nn.value, sn.value) == (6, 2)
    assert call(doc, 8, 1) == G.E_CAPACITY and (nn.value, sn.value) == (6, 2)
    assert call(b"[", 8, 8) == G.E_DECODE and (nn.value, sn.value) == (0, 0)
    assert L_.gpudiff_target_host(doc, len(doc), None, 0, None, None, 0, C.byref(sn)) == G.E_INVAL
    assert G.target_host(b'{"metadata":{"name":"' + b"n" * 1000 + b'"}}') == (b"", b"n" * 1000)


def _plan_of(docs, mode=UC.SPEC):
    """Bodies and their targets as a plan would carry them, from the host path; a document that does not decode is a
    write without a body."""
    bodies, off, ln, fl = [], [], [], []
    for d in docs:
        host = G.upsert_body_host_targets(d, mode) if d is not None else (b"", (0, 0), (0, 0), 0)
        body, o, l, f = host if host is not None else (None, (0, 0), (0, 0), 0)
        bodies.append(body)
        off.append(o)
        ln.append(l)
        fl.append(f)
    tgt = G.Targets(np.array(off, dtype=np.uint32).reshape(-1, 2), np.array(ln, dtype=np.uint32).reshape(-1, 2),
                    np.array(fl, dtype=np.uint8), 0, len(docs))
    return bodies, tgt


def _doc(ns, name=b"n"):
    members = [b'"name":"' + name + b'"'] + ([b'"namespace":"' + ns + b'"'] if ns is not None else [])
    return b'{"metadata":{' + b",".join(members) + b'},"kind":"K"}'


def test_targets_namespaces():
    """gpudiff_targets_namespaces against a dictionary: NULL cluster IDs, a skip mask, absent and "" namespaces in
    one group, equal namespaces in different clusters in two groups, writes without a body not grouped."""
    nss = [b"a", b"b", None, b"", b"a", b"a<b", b"a\\u003cb", b"b", b"c", None, b"a"]
    docs = [_doc(ns, b"n%d" % i) for i, ns in enumerate(nss)]
    docs[4:4] = [None, b"["]  # a no-op write (no body) and an undecodable document
    bodies, tgt = _plan_of(docs)
    n = len(docs)
    keys = [None if not b else b[int(tgt.off[w, 1]):int(tgt.off[w, 1]) + int(tgt.len[w, 1])]
            for w, b in enumerate(bodies)]
    assert keys[4] is None and keys[5] is None and keys[2] == keys[3] == b""
    clusters = np.array([w % 5 for w in range(n)], dtype=np.uint32)
    skip = np.array([w in (0, 7) for w in range(n)], dtype=np.uint8)
    for cl, sk in ((None, None), (clusters, None), (None, skip), (clusters, skip)):
        group_of, first = G.targets_namespaces(bodies, tgt, cl, sk)
        want_g, want_f = M.namespaces(keys, cl, sk)
        assert group_of.tolist() == want_g and first.tolist() == want_f, (cl, sk)
    group_of, first = G.targets_namespaces(bodies, tgt)
    assert group_of[4] == group_of[5] == M.NOT_GROUPED
    assert group_of[2] == group_of[3] and first[group_of[2]] == 2           # absent and "": one group
    assert group_of[0] == group_of[6] == group_of[n - 1] == 0               # "a" again
    assert len({int(group_of[7]), int(group_of[8]), 0}) == 2                # a<b, however the document spelt it
    assert len(first) == 5                                                  # a, b, "", a<b, c
    group_of, first = G.targets_namespaces(bodies, tgt, clusters)
    assert group_of[0] != group_of[n - 1] and clusters[0] != clusters[n - 1]  # equal namespaces, two clusters
    # nothing to group
    group_of, first = G.targets_namespaces([], G.Targets(np.zeros((0, 2), np.uint32), np.zeros((0, 2), np.uint32),
                                                         np.zeros(0, np.uint8), 0, 0))
    assert len(group_of) == 0 and len(first) == 0
    group_of, first = G.targets_namespaces(bodies, tgt, None, np.ones(n, dtype=np.uint8))
    assert set(group_of.tolist()) == {M.NOT_GROUPED} and len(first) == 0


def test_targets_namespaces_argument_checks():
    L_ = G.lib()
    bodies, tgt = _plan_of([_doc(b"a"), _doc(b"b")])
    raw = b"".join(bodies)
    offs = np.array([0, len(bodies[0]), len(raw)], dtype=np.uint64)
    st = np.zeros(2, dtype=np.int32)
    off = np.ascontiguousarray(tgt.off).reshape(-1)
    ln = np.ascontiguousarray(tgt.len).reshape(-1)
    b = G.Bodies(n=2, offsets=offs.ctypes.data, bytes=C.cast(C.c_char_p(raw), C.c_void_p), status=st.ctypes.data)
    group_of, first, ng = np.zeros(2, np.uint32), np.zeros(2, np.uint32), C.c_size_t()

    def call(t, bp=C.byref(b)):
        return L_.gpudiff_targets_namespaces(bp, C.byref(t), None, None, group_of.ctypes.data, first.ctypes.data,
                                             C.byref(ng))
    good = G.TargetsC(n=2, off=off.ctypes.data, len=ln.ctypes.data, flags=tgt.flags.ctypes.data)
    assert call(good) == G.OK and ng.value == 2 and group_of.tolist() == [0, 1] and first.tolist() == [0, 1]
    assert call(G.TargetsC(n=1, off=off.ctypes.data, len=ln.ctypes.data)) == G.E_INVAL  # not these bodies' targets
    assert call(good, None) == G.E_INVAL
    far = ln.copy()
    far[3] = len(bodies[1])  # a span that leaves its body
    assert call(G.TargetsC(n=2, off=off.ctypes.data, len=far.ctypes.data)) == G.E_INVAL
