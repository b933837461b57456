"""The resourceVersion splice descriptor on the GPU: kernel K10's phase M8b reports, with each body it renders,
where `"resourceVersion":"<rv>"` goes (gpudiff_bodies_rv_splice).  The device's descriptor must equal the one the
host marshaller records for the same document, the spliced body must equal gpudiff_update_body_host (the direct
marshal, pinned to the model by tests/test_update_body.py), and n_device must count every body K10 rendered --
i.e. the kernel, not the host, decided them.  Through gpudiff_upsert_bodies and both write plans."""
import json

import pytest

from kcp_amd import gpudiff as G
from tests import store_plan_cases as C
from tests import upsert_cases as UC
from tests.test_gpu_store import _stream
from tests.test_gpu_write_plan import _escaped_key_pairs, _noop_pairs

pytestmark = pytest.mark.gpu

RVS = (b"42", b'x<"y\xff')
MODES = pytest.mark.parametrize("mode", [UC.SPEC, UC.STATUS])


def _check_one(doc, mode, body, off, form):
    """One rendered body and its descriptor against the host's for the same document."""
    host = G.upsert_body_host_rv(doc, mode)
    assert host is not None and (body, off, form) == host, (doc[:200], (off, form), host[1:])
    for rv in RVS:
        assert G.splice_resource_version(body, off, form, rv) == G.update_body_host(doc, mode, rv), (rv, doc[:200])


def _check_bodies(eng, docs, mode, all_device=True):
    res = eng.upsert_bodies(docs, mode)
    off, form = res.rv_splice()
    assert len(off) == len(form) == len(docs)
    n_dev = n_host = 0
    for i, d in enumerate(docs):
        if res.bodies[i] is None:  # a Go decode error: no body, no splice
            assert (int(off[i]), int(form[i])) == (0, G.RV_NONE) and G.upsert_body_host(d, mode) is None
            continue
        _check_one(d, mode, res.bodies[i], int(off[i]), int(form[i]))
        if res.source[i] == G.BODY_DEVICE:
            n_dev += 1
        else:
            n_host += 1
    assert (res.rv.n_device, res.rv.n_host) == (n_dev, n_host)
    assert n_dev == int((res.source == G.BODY_DEVICE).sum())
    if all_device:
        assert n_host == 0 and n_dev == len(docs), [int(k) for k in res.k10_status if k]
    return res


def _obj(members):
    return b"{" + b",".join(b'"%s":%s' % (k, v) for k, v in members) + b"}"


def _fill(n, base):
    """n distinct keys around `base`'s place in key order: half sort before it, half behind."""
    return [(b"%s%03d" % (base[:1] if k % 2 else b"z", k), b"%d" % k) for k in range(n)]


def shape_docs():
    docs = []
    rv, uid = (b"resourceVersion", b'"77"'), (b"uid", b'"u"')
    # metadata with 1 .. 130 members (two and three 64-member windows), resourceVersion present or absent, and
    # first, middle or last by key order
    for n in (1, 2, 63, 64, 65, 130):
        for present in (False, True):
            k = n - 1 if present else n
            for keys in ([(b"a%03d" % i, b"%d" % i) for i in range(k)],            # all before: last
                         [(b"z%03d" % i, b'"v%d"' % i) for i in range(k)],         # all behind: first
                         _fill(k, b"resourceVersion")):                            # middle
                members = keys + ([rv] if present else [])
                members.reverse()  # input order is not key order
                docs.append(_obj([(b"kind", b'"K"'), (b"metadata", _obj(members)), (b"spec", b'{"x":[1,{"y":2}]}')]))
    # siblings that share the literal's first bytes: the 8-byte prefix ties, the bytes decide
    near = [b"resourceVersio", b"resourceVersion2", b"resourceV", b"resources", b"resourceversion", b"selfLink", b"uid"]
    for k in range(len(near)):
        for present in (False, True):
            members = [(x, b'"%d"' % i) for i, x in enumerate(near[k:] + near[:k])] + ([rv] if present else [])
            docs.append(_obj([(b"metadata", _obj(members))]))
            docs.append(_obj([(b"metadata", _obj(members[:1] + ([rv] if present else [])))]))
    # the root with 65 and 130 keys around an absent metadata, and with near-misses of "metadata"
    for n in (65, 130):
        docs.append(_obj(list(reversed(_fill(n, b"metadata")))))
        docs.append(_obj([(b"a%03d" % i, b"1") for i in range(n)]))
        docs.append(_obj([(b"n%03d" % i, b"[]") for i in range(n)]))
    docs.append(_obj([(b"metadat", b"1"), (b"metadata2", b"2"), (b"metadatA", b"3"), (b"Metadata", b"{}")]))
    docs.append(_obj([(b"metadata2", b'{"resourceVersion":"1"}')]))
    docs += [b"{}", b'{"spec":{}}', b'{"spec":{},"kind":"K"}', b'{"spec":{"metadata":{"resourceVersion":"9"}}}']
    # metadata {}; emptied (uid / resourceVersion only); emptied by the spec transform but not by the status one
    docs += [b'{"metadata":{}}', b'{"a":1,"metadata":{},"z":2}', _obj([(b"metadata", _obj([uid]))]),
             _obj([(b"metadata", _obj([rv, uid])), (b"x", b"1")]),
             b'{"metadata":{"ownerReferences":[],"resourceVersion":"1"}}',
             b'{"metadata":{"ownerReferences":[{"name":""}],"uid":"u"}}',
             b'{"metadata":{' + UC.OWN + b',"ownerReferences":[{"name":"own"}],"resourceVersion":"1"}}',
             b'{"metadata":{"ownerReferences":[{"name":"own"},{"name":"b","kind":"K","controller":true}]}}']
    # metadata present and not an object
    docs += [b'{"metadata":null,"x":1}', b'{"metadata":"s"}', b'{"a":0,"metadata":[{"resourceVersion":"1"}]}',
             b'{"metadata":7,"spec":{}}', b'{"metadata":[]}', b'{"metadata":true}']
    return docs


@MODES
def test_shapes_decided_on_the_device(mode):
    eng = G.Engine(device=0)
    res = _check_bodies(eng, shape_docs(), mode)
    forms = {int(f) for f in res.rv.form}
    I, L, T, W = G.RV_INSERT, G.RV_LEAD, G.RV_TRAIL, G.RV_WRAP
    assert forms == {G.RV_NONE, I, I | L, I | T, I | W, I | L | W, I | T | W}
    eng.close()


DEFER = [
    # a duplicate key (Go: last wins) in metadata, at the root, and of metadata itself: TOK_HASH
    (b'{"metadata":{"name":"a","name":"b","resourceVersion":"1"}}', G.TOK_HASH),
    (b'{"x":1,"x":2}', G.TOK_HASH),
    (b'{"metadata":{"name":"a"},"metadata":null}', G.TOK_HASH),
    (b'{"metadata":null,"metadata":{"zz":1}}', G.TOK_HASH),
    # a key that needs unescaping: TOK_KEY
    (b'{"metadata":{"n\\u0061me":"a","zz":1}}', G.TOK_KEY),
    (b'{"met\\u0061data":{"name":"a"},"kind":"K"}', G.TOK_KEY),
    (b'{"metadata":{"resourceV\\u0065rsion":"5","name":"a"}}', G.TOK_KEY),
]


@MODES
def test_deferred_documents_carry_the_hosts_descriptor(mode):
    eng = G.Engine(device=0)
    docs = [d for d, _ in DEFER] + [b"[", b'{"metadata":{"name":"a"}}']
    res = _check_bodies(eng, docs, mode, all_device=False)
    assert [int(k) for k in res.k10_status[:len(DEFER)]] == [k for _, k in DEFER]
    assert (res.rv.n_device, res.rv.n_host) == (1, len(DEFER)) and res.bodies[len(DEFER)] is None
    eng.close()


@MODES
def test_corpus(mode):
    """The write path's corpus: what K10 renders carries K10's descriptor, the rest the host's."""
    eng = G.Engine(device=0)
    res = _check_bodies(eng, [k[1] for k in UC.KAT] + UC.fixture_docs(), mode, all_device=False)
    assert res.rv.n_device >= 0.9 * len(res.bodies) - len(UC.KAT)
    _check_bodies(eng, UC.boundary_docs() + UC.synthetic_docs(floats=False), mode)
    eng.close()


def _check_plan(plan, doc_of):
    """Every listed write of a plan: no-ops carry no splice, the others the host's for the rendered document."""
    off, form = plan.rv_splice()
    n = len(plan.bodies)
    assert len(off) == len(form) == n
    n_dev = n_host = 0
    for w in range(n):
        kind = int(plan.kind[w])
        if plan.noop[w]:
            assert plan.bodies[w] == b"" and (int(off[w]), int(form[w])) == (0, G.RV_NONE)
            continue
        _check_one(doc_of(w), kind, plan.bodies[w], int(off[w]), int(form[w]))
        if plan.source[w] == G.BODY_DEVICE:
            n_dev += 1
        else:
            n_host += 1
    assert (plan.rv.n_device, plan.rv.n_host) == (n_dev, n_host)
    return n_dev, n_host


@pytest.mark.parametrize("mode", [G.PLAN_INFORMER, G.PLAN_UPSTREAM_DOWNSTREAM])
def test_write_plan(mode):
    """gpudiff_write_plan_get_ex over a 64-pair device-encoded batch: no-op writes, real edits, and new objects K10
    leaves to the host (an escaped key)."""
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
    eng.close()


def test_store_write_plan():
    """gpudiff_store_write_plan_get: a 3-batch replay over 32 slots (several events of a slot coalesce into one
    write of its last version), then the hand-made chains with their no-op writes and a last version K10 defers."""
    eng = G.Engine(device=0, encode_threads=2)
    st = eng.object_store(max_slots=32, space_bytes=16 << 20, max_events=128, device_encode=True)
    seen = 0
    for evs, _pairs in _stream(23, 32, 3, 90):
        t = st.submit([(s, nj, oj, i, s % 7) for i, (s, nj, oj) in enumerate(evs)])
        eng.wait(t)
        plan = st.write_plan(t)
        assert len(set(plan.pair_index.tolist())) < len(evs)  # coalesced
        n_dev, n_host = _check_plan(plan, lambda w: evs[int(plan.pair_index[w])][1])
        assert n_host == 0
        seen += n_dev
    assert seen > 60
    st.free()
    st = eng.object_store(max_slots=32, space_bytes=16 << 20, max_events=128, device_encode=True)
    events, want = C.chain_batch()
    dup = json.dumps(json.loads(C.V0), separators=(",", ":")).encode()[:-1] + b',"kind":"Deployment"}'
    events.append((len(C.chains()), C.spec_edit(dup), C.V0))  # a duplicate key: K10 leaves it to the host
    t = st.submit([(s, nj, oj, i, s % 7) for i, (s, nj, oj) in enumerate(events)])
    eng.wait(t)
    plan = st.write_plan(t)
    n_dev, n_host = _check_plan(plan, lambda w: events[int(plan.pair_index[w])][1])
    assert plan.noop.sum() == sum(1 for w in want if w[2]) and n_dev > 0 and n_host >= 1
    st.free()
    eng.close()
