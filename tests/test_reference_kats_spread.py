"""Known-answer tests ported from the reference's scheduler/spread_test.go
(TestSpreadIterator_SingleAttribute, lines 15-171, is in test_reference_kats.py).

The reference drives a SpreadIterator alone; at the Stack boundary bin-pack is
scores[0] and job anti-affinity follows it on nodes that hold a planned alloc of
the job, so each case compares the allocation-spread component (the last score,
appended only when non-zero, spread.go:163-167) with the reference's number.
Every engine case also equals the oracle bit for bit, and a whole-list Select
must pick the node the per-node results name.
"""
import pytest

from nomad_amd import synth
from nomad_amd.structs import Allocation, Spread, SpreadTarget
from tests.kat import STACKS_SWEEP, both, kind_of, mk, select_all, select_on


def dc_nodes(dcs, racks=None):
    nodes = []
    for i, dc in enumerate(dcs):
        n = synth.mock_node("n%02d" % i)
        n.datacenter = dc
        if racks:
            n.meta["rack"] = racks[i]
        n.compute_class()
        nodes.append(n)
    return nodes


def spread_job(count, spreads):
    job = synth.mock_job("spreadjob", count=count)
    job.task_groups[0].network = None
    job.task_groups[0].spreads = spreads
    return job


def spread_part(r, collisions):
    """The allocation-spread score of a record: the last of scores when the
    record carries one more than bin-pack and (with collisions) anti-affinity."""
    base = 1 + (1 if collisions else 0)
    assert len(r.scores) in (base, base + 1), r.scores
    return r.scores[-1] if len(r.scores) == base + 1 else 0.0


@pytest.mark.parametrize("name", STACKS_SWEEP)
def test_spread_multiple_attributes(name, monkeypatch):
    """spread_test.go:173-272 TestSpreadIterator_MultipleAttributes: two spreads
    (datacenter 60/40 weight 100, meta.rack 40/60 weight 50) combine to 0.500,
    0.667, 0.556, 0.556 (asserted through %.3f)."""
    def scenario(kind):
        nodes = dc_nodes(["dc1", "dc2", "dc1", "dc1"], ["r1", "r1", "r2", "r2"])
        job = spread_job(10, [
            Spread("${node.datacenter}", 100, [SpreadTarget("dc1", 60), SpreadTarget("dc2", 40)]),
            Spread("${meta.rack}", 50, [SpreadTarget("r1", 40), SpreadTarget("r2", 60)])])
        allocs = [Allocation(node_id=nodes[0].id, job_id=job.id, task_group="web"),
                  Allocation(node_id=nodes[2].id, job_id=job.id, task_group="web")]
        st = mk(kind.generic(), nodes, allocs, job)
        per = [select_on(st, n) for n in nodes]
        want = ["0.500", "0.667", "0.556", "0.556"]
        for i, (r, w) in enumerate(zip(per, want)):
            assert r.row == i
            assert "%.3f" % spread_part(r, i in (0, 2)) == w, (i, r.scores)
        top = select_all(st, nodes, per, full_scan=True)
        assert top.row == 1           # dc2 / r1 and no alloc of the job: the reference's highest
        return per + [top]
    both(kind_of(name, monkeypatch), scenario)


EVEN_DCS = ["dc1", "dc2", "dc1", "dc2", "dc1", "dc2", "dc2", "dc1", "dc1", "dc1"]


@pytest.mark.parametrize("name", STACKS_SWEEP)
def test_spread_even_spread(name, monkeypatch):
    """spread_test.go:274-459 TestSpreadIterator_EvenSpread, all four stages: 0 / 0
    with nothing placed; -1 / +1 after one planned alloc on two dc1 nodes; +0.5 /
    -0.5 (%3.3f) once dc2 holds three; -1 / -1 / +1 when dc1 draws level and a dc3
    node joins. The dc3 node is in the snapshot from the start and enters the
    visit list in the last stage only."""
    def scenario(kind):
        nodes = dc_nodes(EVEN_DCS + ["dc3"])
        visit = nodes[:10]
        job = spread_job(10, [Spread("${node.datacenter}", 100, [])])
        st = mk(kind.generic(), nodes, [], job)
        planned = [0] * len(nodes)
        trace = []

        def stage(visit, want, fmt):
            per = [select_on(st, n) for n in visit]
            for n, r in zip(visit, per):
                i = nodes.index(n)
                assert r.row == i
                got = spread_part(r, planned[i])
                if fmt is None:
                    assert got == want[n.datacenter], (i, r.scores)
                else:
                    assert fmt % got == fmt % want[n.datacenter], (i, r.scores)
            top = select_all(st, visit, per, full_scan=True)
            best = max(want.values())
            if best > 0:
                assert want[nodes[top.row].datacenter] == best
            trace.extend(per + [top])

        def plan(i, k=1):
            for _ in range(k):
                st.Commit(0, i)
                planned[i] += 1

        stage(visit, {"dc1": 0.0, "dc2": 0.0}, "%.3f")
        plan(0); plan(2)
        stage(visit, {"dc1": -1.0, "dc2": 1.0}, None)          # require.Equal on the float
        plan(1, 2); plan(3)
        stage(visit, {"dc1": 0.5, "dc2": -0.5}, "%3.3f")
        plan(4)
        stage(nodes, {"dc1": -1.0, "dc2": -1.0, "dc3": 1.0}, "%.3f")
        return trace
    both(kind_of(name, monkeypatch), scenario)


@pytest.mark.parametrize("name", STACKS_SWEEP)
def test_spread_max_penalty(name, monkeypatch):
    """spread_test.go:462-547 TestSpreadIterator_MaxPenalty: every node is in dc3
    while the targets name dc1 / dc2, and then the spread attribute exists on no
    node: -1.0 exactly, both times."""
    def scenario(kind):
        nodes = dc_nodes(["dc3"] * 5)
        trace = []
        for spread in (Spread("${node.datacenter}", 100, [SpreadTarget("dc1", 80), SpreadTarget("dc2", 20)]),
                       Spread("${meta.foo}", 100, [SpreadTarget("bar", 80), SpreadTarget("baz", 20)])):
            st = mk(kind.generic(), nodes, [], spread_job(5, [spread]))
            per = [select_on(st, n) for n in nodes]
            for i, r in enumerate(per):
                assert r.row == i and len(r.scores) == 2 and r.scores[-1] == -1.0, (i, r.scores)
            top = select_all(st, nodes, per, full_scan=True)
            # every final score is negative and equal: the LimitIterator sets the first
            # three aside (select.go:35-74), so the fourth is the first returned
            assert top.row == 3
            trace.extend(per + [top])
        return trace
    both(kind_of(name, monkeypatch), scenario)


@pytest.mark.parametrize("name", STACKS_SWEEP)
def test_even_spread_score_boost_is_finite(name, monkeypatch):
    """spread_test.go:549-570 Test_evenSpreadScoreBoost: a property value whose
    allocs were all cleared counts 0; with the minimum at 0 the boost is 1.0, not
    +Inf. Existing allocs of the job sit in dc2 and dc3, one placement lands in
    dc1, and the plan stops both existing allocs: dc2 and dc3 score exactly 1.0."""
    def scenario(kind):
        nodes = dc_nodes(["dc1", "dc2", "dc3"])
        job = spread_job(3, [Spread("${node.datacenter}", 100, [])])
        allocs = [Allocation(node_id=nodes[1].id, job_id=job.id, task_group="web"),
                  Allocation(node_id=nodes[2].id, job_id=job.id, task_group="web")]
        st = mk(kind.generic(), nodes, allocs, job)
        st.Commit(0, 0)
        st.StopAllocs([0, 1])
        per = [select_on(st, n) for n in nodes]
        for i in (1, 2):
            assert per[i].row == i and len(per[i].scores) == 2
            assert per[i].scores[-1] == 1.0, per[i].scores
        assert spread_part(per[0], 1) == -1.0     # dc1 holds the only alloc left: the maximum
        top = select_all(st, nodes, per, full_scan=True)
        assert top.row == 1
        return per + [top]
    both(kind_of(name, monkeypatch), scenario)
