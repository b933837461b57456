"""tests/store_plan_model.py, the Python restatement of the store's write plan, against what is
already pinned: on batches where every slot has one event it is oracle/upsert_oracle.write_plan of the (old, new)
pairs, and on hand-made chains (tests/store_plan_cases.py) it gives the writes worked out by hand."""
import pytest

from oracle import upsert_oracle as U
from tests import store_plan_cases as C
from tests.golden.kat_cases import cases
from tests.store_plan_model import PLAN_SPEC, PLAN_STATUS, StoreModel, fold
from tests.workload import make_pairs


@pytest.mark.parametrize("mode", [0, PLAN_SPEC, PLAN_STATUS, PLAN_SPEC | PLAN_STATUS])
def test_one_event_per_slot_is_the_pair_plan(mode):
    pairs = [(a, b) for _, a, b, _, _ in cases() if len(a) < 4096 and len(b) < 4096]  # without the deep-nesting KATs
    pairs += make_pairs(60, seed=5, mutate_frac=0.4)[0]
    events = [(i, b, a) for i, (a, b) in enumerate(pairs)]
    got = StoreModel().plan(events, mode)
    assert got == U.write_plan(pairs, mode)
    assert any(w[2] for w in got) and any(not w[2] for w in got) and any(w[3] is None for w in got)


def test_resident_version_is_the_old_side():
    """The second batch diffs against what the first made resident, whatever old_json says."""
    m = StoreModel()
    assert m.plan([(0, C.V0, None)]) == [(0, 0, False, U.upsert_body(C.V0, 0)), (0, 1, False, U.upsert_body(C.V0, 1))]
    assert m.plan([(0, C.churn(C.V0, 1), C.spec_edit(C.V0))]) == []
    # an undecodable version empties the slot: the next event is a first sighting again ({} without old_json)
    assert m.plan([(0, b'{"spec": ', None)]) == [(0, 0, False, None), (0, 1, False, None)]
    assert [w[:3] for w in m.plan([(0, C.V0, None)])] == [(0, 0, False), (0, 1, False)]
    m.forget(0)
    assert [w[:3] for w in m.plan([(0, C.V0, C.V0)])] == []


@pytest.mark.parametrize("name,versions,writes", C.chains(), ids=[c[0].replace(" ", "_") for c in C.chains()])
def test_hand_made_chain(name, versions, writes):
    events = [(3, v, C.V0 if k == 0 else None) for k, v in enumerate(versions)]
    got = StoreModel().plan(events)
    assert [w[:3] for w in got] == sorted(writes, key=lambda w: (w[1], w[0]))
    for i, kind, noop, body in got:
        assert body == (b"" if noop else U.upsert_body(versions[i], kind))
        assert i == len(versions) - 1  # always the chain's last version


def test_interleaved_chains_and_kind_selection():
    events, want = C.chain_batch()
    assert [w[:3] for w in StoreModel().plan(events)] == want
    assert [w[:3] for w in StoreModel().plan(events, PLAN_SPEC)] == [w for w in want if w[1] == 0]
    assert [w[:3] for w in StoreModel().plan(events, PLAN_STATUS)] == [w for w in want if w[1] == 1]


def test_fold_rule():
    D = lambda sd, sn, td, tn: dict(spec_dirty=sd, spec_noop=sn, status_dirty=td, status_noop=tn)
    assert fold([D(False, False, False, False)]) == {0: (False, False), 1: (False, False)}
    assert fold([D(True, True, False, False), D(False, False, False, False)]) == {0: (True, True), 1: (False, False)}
    assert fold([D(True, True, True, False), D(True, False, True, True)]) == {0: (True, False), 1: (True, False)}
    assert fold([D(True, True, True, True)] * 3) == {0: (True, True), 1: (True, True)}
