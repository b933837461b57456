"""Hand-made watch-replay chains for the store's write plan (tests/store_plan_model.py): versions of the KAT
Deployment whose diffs are known -- clean (metadata churn), a spec or status no-op (int <-> integral float: dirty
under DeepEqual, identical on the wire), real edits, a status dropped and restored."""
import json

from tests.golden.kat_cases import BASE, J

V0 = J(BASE)
assert b'"replicas":3,"selector"' in V0 and b'"readyReplicas":3' in V0 and b'"revisionHistoryLimit":10' in V0


def churn(doc: bytes, k: int) -> bytes:
    """The same object after metadata churn the syncer ignores: clean against `doc`."""
    # on the bytes: a JSON round trip would respell the 3.0 / 3e0 of the retyped versions
    out = doc.replace(b'"resourceVersion":"1001"', b'"resourceVersion":"%d"' % (5000 + k))
    out = out.replace(b'"uid":"6f1d2c3e-0000-4000-8000-000000000001"', b'"uid":"99999999-0000-4000-8000-%012d"' % k)
    assert out != doc and len(out) == len(doc)
    return out


def spec_retype(doc: bytes) -> bytes:      # spec no-op against the int spelling
    return doc.replace(b'"replicas":3,"selector"', b'"replicas":3.0,"selector"')


def status_retype(doc: bytes) -> bytes:    # status no-op against the int spelling
    return doc.replace(b'"readyReplicas":3', b'"readyReplicas":3e0')


def spec_edit(doc: bytes, to: int = 11) -> bytes:
    return doc.replace(b'"revisionHistoryLimit":10', b'"revisionHistoryLimit":%d' % to)


def no_status(doc: bytes) -> bytes:
    o = json.loads(doc)
    del o["status"]
    return J(o)


def chains():
    """[(name, [new versions of one slot, in order; the first event carries old_json = V0],
         expected writes [(index of the chain's event, kind, noop)])]: kind 0 spec, 1 status."""
    return [
        ("noop then clean", [spec_retype(V0), churn(spec_retype(V0), 1)], [(1, 0, True)]),
        ("noop then real", [spec_retype(V0), spec_edit(spec_retype(V0))], [(1, 0, False)]),
        ("real then noop", [spec_edit(V0), spec_retype(spec_edit(V0))], [(1, 0, False)]),
        ("noop, clean, noop back", [spec_retype(V0), churn(spec_retype(V0), 2), churn(V0, 3)], [(2, 0, True)]),
        ("status noop then clean", [status_retype(V0), churn(status_retype(V0), 4)], [(1, 1, True)]),
        ("status dropped then restored", [no_status(V0), churn(V0, 5)], [(1, 1, False)]),
        ("spec noop and status real", [status_retype(spec_retype(V0)), no_status(spec_retype(V0))],
         [(1, 0, True), (1, 1, False)]),
        ("clean only", [churn(V0, 6), churn(V0, 7)], []),
        ("single real", [spec_edit(V0)], [(0, 0, False)]),
    ]


def chain_batch():
    """All chains interleaved in one batch, one slot each: (events [(slot, new, old)], expected writes
    [(pair_index, kind, noop)] in plan order)."""
    cs = chains()
    events, want = [], []
    pos = {}  # (chain, k) -> event index
    depth = max(len(v) for _n, v, _w in cs)
    for k in range(depth):
        for s, (_n, versions, _w) in enumerate(cs):
            if k < len(versions):
                pos[(s, k)] = len(events)
                events.append((s, versions[k], V0 if k == 0 else None))
    for s, (_n, _v, writes) in enumerate(cs):
        want += [(pos[(s, k)], kind, noop) for k, kind, noop in writes]
    want.sort(key=lambda w: (w[1], w[0]))
    return events, want
