"""The request target on the GPU: kernel K10 reports, with each body it renders, where metadata.name's and
metadata.namespace's values stand in it (M2 finds the two members, M8c reads their place; gpudiff_bodies_targets).
The device's descriptor must equal the one the host marshaller records for the same document, the decoded spans must
equal gpudiff_target_host (the direct decode, pinned to the model by tests/test_targets.py), and n_device must count
every body K10 rendered -- i.e. the kernel, not the host, decided them.  Through gpudiff_upsert_bodies and both write
plans."""
import json

import numpy as np
import pytest

from kcp_amd import gpudiff as G
from tests import store_plan_cases as C
from tests import targets_model as M
from tests import upsert_cases as UC
from tests.test_gpu_store import _stream
from tests.test_gpu_write_plan import _escaped_key_pairs, _noop_pairs

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("mode", [UC.SPEC, UC.STATUS])
N, NE, S, SE = G.TGT_NAME, G.TGT_NAME_ESC, G.TGT_NS, G.TGT_NS_ESC
ZERO = ((0, 0), (0, 0), 0)


def _desc(tgt, i):
    return ((int(tgt.off[i, 0]), int(tgt.off[i, 1])), (int(tgt.len[i, 0]), int(tgt.len[i, 1])), int(tgt.flags[i]))


def _check_one(doc, mode, body, desc, tgt, bodies, i):
    """One rendered body and its descriptor against the host's for the same document."""
    host = G.upsert_body_host_targets(doc, mode)
    assert host is not None and (body,) + desc == host, (doc[:200], desc, host[1:])
    assert tgt.of(bodies, i) == G.target_host(doc), doc[:200]


def _check_bodies(eng, docs, mode, all_device=True):
    res = eng.upsert_bodies(docs, mode)
    tgt = res.targets()
    assert tgt.off.shape == tgt.len.shape == (len(docs), 2) and len(tgt.flags) == len(docs)
    n_dev = n_host = 0
    for i, d in enumerate(docs):
        if res.bodies[i] is None:  # a Go decode error: no body, an all-zero descriptor
            assert _desc(tgt, i) == ZERO and G.upsert_body_host(d, mode) is None and G.target_host(d) is None
            continue
        _check_one(d, mode, res.bodies[i], _desc(tgt, i), tgt, res.bodies, i)
        if res.source[i] == G.BODY_DEVICE:
            n_dev += 1
        else:
            n_host += 1
    assert (tgt.n_device, tgt.n_host) == (n_dev, n_host)
    assert n_dev == int((res.source == G.BODY_DEVICE).sum())
    if all_device:
        assert n_host == 0 and n_dev == len(docs), [(i, int(k), docs[i][:80]) for i, k in enumerate(res.k10_status) if k]
    return res


def _obj(members):
    return b"{" + b",".join(b'"%s":%s' % (k, v) for k, v in members) + b"}"


def _fill(n, base):
    """n distinct keys around `base`'s place in key order: half sort before it, half behind."""
    return [(b"%s%03d" % (base[:1] if k % 2 else b"z", k), b"%d" % k) for k in range(n)]


def _jstr(raw: bytes) -> bytes:
    """raw (valid UTF-8) as a JSON string that escapes only what it must."""
    return b'"' + raw.replace(b"\\", b"\\\\").replace(b'"', b'\\"') + b'"'


NEAR = [b"nam", b"name2", b"names", b"Name", b"namespac", b"namespace2", b"namespaces", b"Namespace", b"clusterName"]
NOT_STRINGS = [b"7", b"null", b"true", b"{}", b"[]", b'{"name":"in"}', b'["name","namespace"]']
U2028 = b"\xe2\x80\xa8"


def shape_docs():
    docs = []
    name, ns = (b"name", b'"the-name"'), (b"namespace", b'"the-ns"')
    # metadata with 1 .. 130 members (two and three 64-member windows); each of name and namespace absent or present;
    # first, middle or last by key order; the input order reversed
    for n in (1, 2, 63, 64, 65, 130):
        for fields in ([], [name], [ns], [name, ns]):
            k = n - len(fields)
            if k < 0:
                continue
            for keys in ([(b"a%03d" % i, b"%d" % i) for i in range(k)],            # all before: last
                         [(b"z%03d" % i, b'"v%d"' % i) for i in range(k)],         # all behind: first
                         _fill(k, b"name")):                                       # middle
                members = keys + fields
                members.reverse()  # input order is not key order
                docs.append(_obj([(b"kind", b'"K"'), (b"metadata", _obj(members)), (b"spec", b'{"x":[1,{"y":2}]}')]))
    # siblings that share the field names' first bytes, with and without the fields themselves
    for k in range(len(NEAR)):
        near = [(x, b'"d%d"' % i) for i, x in enumerate(NEAR[k:] + NEAR[:k])]
        for fields in ([], [name], [ns], [ns, name]):
            docs.append(_obj([(b"metadata", _obj(near + fields))]))
            docs.append(_obj([(b"metadata", _obj(fields + near[:2]))]))
    # values that are no strings
    for v in NOT_STRINGS:
        docs.append(_obj([(b"metadata", _obj([(b"name", v), ns]))]))
        docs.append(_obj([(b"metadata", _obj([name, (b"namespace", v)]))]))
        docs.append(_obj([(b"metadata", _obj([(b"namespace", v), (b"name", v), (b"zz", b"1")]))]))
    # string values: empty; values around the 16-byte long-string threshold that need escaping ('<', '"', '\\', U+2028,
    # 15 .. 19 decoded bytes); a non-ASCII value that renders clean; an input escape that renders clean
    docs.append(_obj([(b"metadata", _obj([(b"name", b'""'), (b"namespace", b'""')]))]))
    docs.append(_obj([(b"metadata", _obj([(b"name", b'""')])), (b"a", b"1")]))
    docs.append(_obj([(b"metadata", _obj([(b"namespace", b'""'), (b"name", b'"x"')]))]))
    for pad in range(8, 13):
        esc = _jstr(b"abcdefghijkl"[:pad] + b'<"\\' + U2028 + b"z")
        plain = _jstr(b"abcdefghijklmnopqrs"[:pad + 7])
        docs.append(_obj([(b"metadata", _obj([(b"name", esc), (b"namespace", plain)]))]))
        docs.append(_obj([(b"metadata", _obj([(b"name", plain), (b"namespace", esc)]))]))
        docs.append(_obj([(b"metadata", _obj([(b"namespace", esc), (b"name", esc), (b"uid", b'"u"')]))]))
    for one in (b"<", b"\\\\", b'\\"', U2028, b"\\n", b"\\u0001"):
        docs.append(_obj([(b"metadata", _obj([(b"name", b'"' + one + b'"'), (b"namespace", b'"q' + one + b'"')]))]))
    docs.append(_obj([(b"metadata", _obj([(b"name", b'"caf\xc3\xa9-\xe6\x97\xa5\xe6\x9c\xac"'), (b"namespace", b'"\xf0\x9f\x98\x80"')]))]))
    docs.append(_obj([(b"metadata", _obj([(b"name", b'"\\u0061b"'), (b"namespace", b'"n\\u0073"')]))]))
    # metadata absent, null, a string, a list, {}
    docs += [b"{}", b'{"kind":"K","spec":{}}', b'{"metadata":null,"x":1}', b'{"metadata":"name"}',
             b'{"a":0,"metadata":[{"name":"a","namespace":"b"}]}', b'{"metadata":{}}', b'{"a":1,"metadata":{},"z":2}',
             b'{"metadata":7}', b'{"metadata":true,"name":"x"}']
    # decoys that must not count: a root-level name, spec.metadata.name, an owner reference's name -- removed with the
    # owned-by label (spec mode), normalised without it
    docs += [b'{"name":"root","namespace":"rootns","metadata":{"zz":1}}',
             b'{"name":"root","metadata":{"name":"real"},"namespace":"rootns"}',
             b'{"spec":{"metadata":{"name":"s","namespace":"t"}},"metadata":{"labels":{"name":"l","namespace":"m"}}}',
             b'{"spec":{"metadata":{"name":"s"}},"metadata":{"namespace":"real-ns"}}',
             b'{"metadata":{' + UC.OWN + b',"ownerReferences":[{"name":"own","namespace":"x"}]}}',
             b'{"metadata":{' + UC.OWN + b',"ownerReferences":[{"name":"own"}],"name":"real","namespace":"ns"}}',
             b'{"metadata":{"ownerReferences":[{"name":"o1","kind":"K"},{"name":"o2"}]}}',
             b'{"metadata":{"ownerReferences":[{"name":"o1","kind":"K"}],"namespace":"ns","name":"real<"}}']
    return docs


@MODES
def test_shapes_decided_on_the_device(mode):
    eng = G.Engine(device=0)
    res = _check_bodies(eng, shape_docs(), mode)
    tgt = res.targets()
    seen = {int(f) for f in tgt.flags}
    assert {0, N, S, N | S, N | NE | S, N | S | SE, N | NE | S | SE} <= seen, sorted(seen)
    assert all((f & NE) == 0 or (f & N) for f in seen) and all((f & SE) == 0 or (f & S) for f in seen)
    assert any(f & N and tgt.len[i, 0] == 0 and tgt.off[i, 0] > 0 for i, f in enumerate(tgt.flags))  # present, empty
    assert any(f & S and tgt.len[i, 1] == 0 and tgt.off[i, 1] > 0 for i, f in enumerate(tgt.flags))
    eng.close()


DEFER = [
    # a duplicate key (Go: the last wins) of the fields and of metadata itself: TOK_HASH
    (b'{"metadata":{"name":"a","name":"b","namespace":"x"}}', G.TOK_HASH),
    (b'{"metadata":{"namespace":"x","name":"a","namespace":7}}', G.TOK_HASH),
    (b'{"metadata":{"name":"a"},"metadata":{"namespace":"q"}}', G.TOK_HASH),
    (b'{"metadata":null,"metadata":{"name":"zz"}}', G.TOK_HASH),
    # a key that needs unescaping to spell the field's name: TOK_KEY
    (b'{"metadata":{"n\\u0061me":"a","zz":1}}', G.TOK_KEY),
    (b'{"metadata":{"namesp\\u0061ce":"ns","name":"a<"}}', G.TOK_KEY),
    (b'{"met\\u0061data":{"name":"a"},"kind":"K"}', G.TOK_KEY),
]


@MODES
def test_deferred_documents_carry_the_hosts_descriptor(mode):
    eng = G.Engine(device=0)
    docs = [d for d, _ in DEFER] + [b"[", b'{"metadata":{"name":"a"}}']
    res = _check_bodies(eng, docs, mode, all_device=False)
    tgt = res.targets()
    assert [int(k) for k in res.k10_status[:len(DEFER)]] == [k for _, k in DEFER]
    assert (tgt.n_device, tgt.n_host) == (1, len(DEFER)) and res.bodies[len(DEFER)] is None
    assert tgt.of(res.bodies, 0) == (b"x", b"b") and tgt.of(res.bodies, 2) == (b"q", b"")  # the last one wins
    eng.close()


@MODES
def test_corpus(mode):
    """The write path's corpus: what K10 renders carries K10's descriptor, the rest the host's."""
    eng = G.Engine(device=0)
    res = _check_bodies(eng, [k[1] for k in UC.KAT] + UC.fixture_docs(), mode, all_device=False)
    assert res.targets().n_device >= 0.9 * len(res.bodies) - len(UC.KAT)
    _check_bodies(eng, UC.boundary_docs() + UC.synthetic_docs(floats=False), mode)
    eng.close()


def _check_plan(plan, doc_of, cluster_of=None):
    """Every listed write of a plan: no-ops are all zero, the others carry the host's descriptor for the rendered
    document; namespaces() equals the model's grouping."""
    tgt = plan.targets()
    n = len(plan.bodies)
    assert tgt.off.shape == tgt.len.shape == (n, 2) and len(tgt.flags) == n
    n_dev = n_host = 0
    keys = []
    for w in range(n):
        kind = int(plan.kind[w])
        if plan.noop[w]:
            assert plan.bodies[w] == b"" and _desc(tgt, w) == ZERO
            keys.append(None)
            continue
        _check_one(doc_of(w), kind, plan.bodies[w], _desc(tgt, w), tgt, plan.bodies, w)
        _body, off, ln, _fl = G.upsert_body_host_targets(doc_of(w), kind)
        keys.append(_body[off[1]:off[1] + ln[1]])
        if plan.source[w] == G.BODY_DEVICE:
            n_dev += 1
        else:
            n_host += 1
    assert (tgt.n_device, tgt.n_host) == (n_dev, n_host)
    clusters = None if cluster_of is None else np.array([cluster_of(w) for w in range(n)], dtype=np.uint32)
    for kind in (None, G.UPSERT_SPEC, G.UPSERT_STATUS):
        skip = None if kind is None else [int(k) != kind for k in plan.kind]
        group_of, first = plan.namespaces(kind=kind, cluster_ids=clusters)
        want_g, want_f = M.namespaces(keys, clusters, skip)
        assert group_of.tolist() == want_g and first.tolist() == want_f, kind
    return n_dev, n_host


@pytest.mark.parametrize("mode", [G.PLAN_INFORMER, G.PLAN_UPSTREAM_DOWNSTREAM])
def test_write_plan(mode):
    """gpudiff_write_plan_get_ex over a 64-pair device-encoded batch: no-op writes, real edits, and new objects K10
    leaves to the host (an escaped key).  PLAN_TARGETS is accepted and changes nothing."""
    eng = G.Engine(device=0, device_encode=True)
    pairs = _noop_pairs(40, 5) + _escaped_key_pairs(24, 6)
    assert len(pairs) == 64
    t = eng.submit(pairs)
    eng.wait(t)
    plan = eng.write_plan(t, mode)

    def doc_of(w):
        side = 0 if (plan.kind[w] == G.UPSERT_SPEC and mode & G.PLAN_UPSTREAM_DOWNSTREAM) else 1
        return pairs[int(plan.pair_index[w])][side]
    n_dev, n_host = _check_plan(plan, doc_of)
    assert n_dev >= 20 and plan.noop.any()
    assert n_host > 0 or mode & G.PLAN_UPSTREAM_DOWNSTREAM  # (A, B): the spec write renders A, which has no such key
    assert plan.targets().flags.any()
    again = eng.write_plan(t, mode | G.PLAN_TARGETS)
    assert again.bodies == plan.bodies and _all(again.targets()) == _all(plan.targets())
    eng.close()


def _all(tgt):
    return tgt.off.tolist(), tgt.len.tolist(), tgt.flags.tolist(), tgt.n_device, tgt.n_host


def test_store_write_plan():
    """gpudiff_store_write_plan_get with PLAN_TARGETS: a 3-batch replay over 32 slots, then the hand-made chains with
    their no-op writes; 16 B more per write come back, and no more.  The chains again with a last version K10 defers:
    that write carries the host's descriptor (its JSON comes back too, so the byte bound does not apply there)."""
    eng = G.Engine(device=0, encode_threads=2)
    st = eng.object_store(max_slots=32, space_bytes=16 << 20, max_events=128, device_encode=True)
    seen = 0
    for evs, _pairs in _stream(23, 32, 3, 90):
        t = st.submit([(s, nj, oj, i, s % 7) for i, (s, nj, oj) in enumerate(evs)])
        eng.wait(t)
        plan = st.write_plan(t, G.PLAN_TARGETS)
        assert len(set(plan.pair_index.tolist())) < len(evs)  # coalesced
        n_dev, n_host = _check_plan(plan, lambda w: evs[int(plan.pair_index[w])][1],
                                    lambda w: evs[int(plan.pair_index[w])][0] % 7)
        assert n_host == 0
        s = st.plan_stats()
        assert s.writes == len(plan.bodies) and s.d2h_bytes <= s.body_bytes + 38 * s.writes + 96
        seen += n_dev
    assert seen > 60
    st.free()
    dup = json.dumps(json.loads(C.V0), separators=(",", ":")).encode()[:-1] + b',"kind":"Deployment"}'
    for defer in (False, True):
        st = eng.object_store(max_slots=32, space_bytes=16 << 20, max_events=128, device_encode=True)
        events, want = C.chain_batch()
        if defer:
            events.append((len(C.chains()), C.spec_edit(dup), C.V0))  # a duplicate key: K10 leaves it to the host
        t = st.submit([(s, nj, oj, i, s % 7) for i, (s, nj, oj) in enumerate(events)])
        eng.wait(t)
        plan = st.write_plan(t, G.PLAN_TARGETS)
        n_dev, n_host = _check_plan(plan, lambda w: events[int(plan.pair_index[w])][1],
                                    lambda w: events[int(plan.pair_index[w])][0] % 7)
        assert plan.noop.sum() == sum(1 for w in want if w[2]) and n_dev > 0 and n_host == (1 if defer else 0)
        s = st.plan_stats()
        if not defer:
            assert s.d2h_bytes <= s.body_bytes + 38 * s.writes + 96
        st.free()
    eng.close()


def test_store_write_plan_without_targets():
    """The same store ticket without PLAN_TARGETS: the bodies carry no targets (GPUDIFF_E_STATE), the copy back keeps
    the 22-byte bound, and bodies, kinds and splice points are those of the plan with targets."""
    eng = G.Engine(device=0, encode_threads=2)
    st = eng.object_store(max_slots=32, space_bytes=16 << 20, max_events=128, device_encode=True)
    evs, _pairs = next(iter(_stream(23, 32, 3, 90)))
    t = st.submit([(s, nj, oj, i, s % 7) for i, (s, nj, oj) in enumerate(evs)])
    eng.wait(t)
    plain = st.write_plan(t)
    s = st.plan_stats()
    assert s.writes == len(plain.bodies) > 0 and s.d2h_bytes <= s.body_bytes + 22 * s.writes + 96
    d2h_plain = s.d2h_bytes
    for call in (plain.targets, plain.namespaces):
        with pytest.raises(G.GpuDiffError) as ei:
            call()
        assert ei.value.code == G.E_STATE
    with_t = st.write_plan(t, G.PLAN_TARGETS | G.PLAN_SPEC | G.PLAN_STATUS)
    assert st.plan_stats().d2h_bytes == d2h_plain + 16 * s.writes
    assert with_t.bodies == plain.bodies and with_t.kind.tolist() == plain.kind.tolist()
    assert with_t.pair_index.tolist() == plain.pair_index.tolist() and with_t.noop.tolist() == plain.noop.tolist()
    assert [a.tolist() for a in with_t.rv_splice()] == [a.tolist() for a in plain.rv_splice()]
    assert with_t.targets().flags.any()
    st.free()
    eng.close()
