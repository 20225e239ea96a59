"""Known-answer tests ported from the reference's scheduler/rank_test.go
(NoExistingAlloc 34-137, ReservedCores 950-1065, JobAntiAffinity 1628-1695,
ScoreNormalization 1744-1807 and NodeAffinity 1809-1882 are in
test_reference_kats.py; the device cases in test_devices.py).

The reference runs a BinPackIterator alone over hand-made nodes. Here the same
nodes and asks go through the whole Stack; bin-pack is scores[0], and where a
case plans allocs of the job itself (the only allocs Commit can plan) the job
anti-affinity score follows it, so those cases compare scores[0] and the others
final_score, which then is bin-pack alone. Every engine case also equals the
oracle bit for bit, and a whole-list Select must pick the node the per-node
results name.
"""
import pytest

from nomad_amd import synth
from nomad_amd.stack import SelectOptions
from nomad_amd.structs import Allocation, Job, NetworkResource, Task, TaskGroup
from tests.kat import STACKS, STACKS_SWEEP, both, kind_of, mk, select_all, select_on


def plain_node(nid, cpu, mem, rcpu=0, rmem=0, reserved_ports=(22,)):
    n = synth.mock_node(nid)
    n.cpu_shares, n.memory_mb, n.reserved_cpu, n.reserved_memory_mb = cpu, mem, rcpu, rmem
    n.disk_mb, n.reserved_disk_mb = 0, 0
    n.reserved_host_ports = list(reserved_ports)
    n.compute_class()
    return n


def plain_job(cpu, mem, count=1, task_net=None, group_net=None, job_id="kat"):
    return Job(id=job_id, task_groups=[TaskGroup(
        name="web", count=count, ephemeral_disk_mb=0, network=group_net,
        tasks=[Task(name="web", driver="exec", cpu=cpu, memory_mb=mem, network=task_net)])])


@pytest.mark.parametrize("name", STACKS_SWEEP)
def test_binpack_mixed_reserve(name, monkeypatch):
    """rank_test.go:139-251 TestBinPackIterator_NoExistingAlloc_MixedReserve: three
    nodes are feasible and rank no-reserved > reserved > reserved2 (reservations
    count against the node); the 900 / 900 node is exhausted."""
    def scenario(kind):
        nodes = [plain_node("a-no-reserved", 1100, 1100), plain_node("b-reserved", 2000, 2000, 800, 800),
                 plain_node("c-reserved2", 2000, 2000, 500, 500), plain_node("d-overloaded", 900, 900)]
        st = mk(kind.generic(), nodes, [], plain_job(1000, 1000))
        per = [select_on(st, n) for n in nodes]
        assert [r.row for r in per] == [0, 1, 2, -1]
        assert per[3].nodes_exhausted == 1
        assert all(len(r.scores) == 1 for r in per[:3])
        assert per[0].final_score > per[1].final_score > per[2].final_score
        top = select_all(st, nodes, per)
        assert top.row == 0
        return per + [top]
    both(kind_of(name, monkeypatch), scenario)


def net_node(nid, cpu, mem):
    return plain_node(nid, cpu, mem, 1024, 1024, reserved_ports=range(1000, 2001))


@pytest.mark.parametrize("name", STACKS_SWEEP)
def test_binpack_network_success(name, monkeypatch):
    """rank_test.go:254-378 TestBinPackIterator_Network_Success: a task network of
    300 MBits and a group network of 500 on 1000-MBit nodes: both nodes take the
    group, the perfect fit scores exactly 1.0 and the 50% fit lands in [0.50, 0.60].
    (The offered MBits the reference also reads are not part of a RankedNode here.)"""
    def scenario(kind):
        nodes = [net_node("n0", 2048, 2048), net_node("n1", 4096, 4096)]
        job = plain_job(1024, 1024, task_net=NetworkResource(device="eth0", mbits=300),
                        group_net=NetworkResource(device="eth0", mbits=500))
        st = mk(kind.generic(), nodes, [], job)
        per = [select_on(st, n) for n in nodes]
        assert [r.row for r in per] == [0, 1]
        assert per[0].scores == [1.0] and per[0].final_score == 1.0
        assert len(per[1].scores) == 1 and 0.50 <= per[1].final_score <= 0.60
        top = select_all(st, nodes, per)
        assert top.row == 0
        return per + [top]
    both(kind_of(name, monkeypatch), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_binpack_network_bandwidth(name):
    """rank_test.go:380-493 TestBinPackIterator_Network_Failure is skipped by the
    reference itself (t.Skip(): bandwidth tracking is deprecated) and its
    expectation is not asserted. Pinned instead is what BinPackIterator does
    (rank.go:248-323) on a 1000-MBit node: task networks are counted against the
    bandwidth, a group network's MBits never are (the group offer is not added
    to the index's used bandwidth, and Overcommitted returns false)."""
    def scenario(kind):
        node = [net_node("n0", 4096, 4096)]
        trace = []

        def run(held, task_mbits, group_mbits):
            allocs = [Allocation(node_id="n0", job_id="other", task_group="web", cpu_shares=2048,
                                 memory_mb=2048, net_mbits=held)]
            job = plain_job(1024, 1024,
                            task_net=NetworkResource(device="eth0", mbits=task_mbits) if task_mbits else None,
                            group_net=NetworkResource(device="eth0", mbits=group_mbits))
            st = mk(kind.generic(), node, allocs, job, metrics=True)
            r = select_on(st, node[0])
            trace.append(r)
            return r, st.LastMetrics()["DimensionExhausted"]

        r, _ = run(700, 300, 250)          # 700 + 300 fills the link; the group's 250 is not counted
        assert r.row == 0
        r, dims = run(700, 301, 250)
        assert r.row == -1 and r.nodes_exhausted == 1
        assert dims == {"network: bandwidth exceeded": 1}
        r, _ = run(1000, 0, 250)           # a full link still takes a group network
        assert r.row == 0
        return trace
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS_SWEEP)
def test_binpack_planned_alloc(name, monkeypatch):
    """rank_test.go:849-949 TestBinPackIterator_PlannedAlloc: planned allocs fill
    the first node and half the second; only the second is left and its bin-pack
    score is exactly 1.0. The planned allocs are the job's own placements here
    (two on the first node, one on the second)."""
    def scenario(kind):
        nodes = [plain_node("n0", 2048, 2048), plain_node("n1", 2048, 2048)]
        st = mk(kind.generic(), nodes, [], plain_job(1024, 1024, count=4))
        for row in (0, 0, 1):
            st.Commit(0, row)
        per = [select_on(st, n) for n in nodes]
        assert per[0].row == -1 and per[0].nodes_exhausted == 1
        assert per[1].row == 1 and per[1].scores[0] == 1.0
        assert per[1].scores[1:] == [-0.5]          # one collision, desired count 4 (rank.go:476-489)
        top = select_all(st, nodes, per)
        assert top.row == 1
        return per + [top]
    both(kind_of(name, monkeypatch), scenario)


def _existing():
    return [Allocation(node_id="n0", job_id="j1", task_group="web", cpu_shares=2048, memory_mb=2048),
            Allocation(node_id="n1", job_id="j2", task_group="web", cpu_shares=1024, memory_mb=1024)]


@pytest.mark.parametrize("name", STACKS_SWEEP)
def test_binpack_existing_alloc(name, monkeypatch):
    """rank_test.go:1067-1180 TestBinPackIterator_ExistingAlloc: other jobs' allocs
    fill the first node and half the second: one option, final score exactly 1.0."""
    def scenario(kind):
        nodes = [plain_node("n0", 2048, 2048), plain_node("n1", 2048, 2048)]
        st = mk(kind.generic(), nodes, _existing(), plain_job(1024, 1024))
        per = [select_on(st, n) for n in nodes]
        assert per[0].row == -1 and per[0].nodes_exhausted == 1
        assert per[1].row == 1 and per[1].scores == [1.0] and per[1].final_score == 1.0
        top = select_all(st, nodes, per)
        assert top.row == 1
        return per + [top]
    both(kind_of(name, monkeypatch), scenario)


@pytest.mark.parametrize("name", STACKS_SWEEP)
def test_binpack_existing_alloc_planned_evict(name, monkeypatch):
    """rank_test.go:1182-1303 TestBinPackIterator_ExistingAlloc_PlannedEvict: the
    plan evicts the alloc that fills the first node: both nodes are options, the
    first in [0.50, 0.95], the second exactly 1."""
    def scenario(kind):
        nodes = [plain_node("n0", 2048, 2048), plain_node("n1", 2048, 2048)]
        st = mk(kind.generic(), nodes, _existing(), plain_job(1024, 1024))
        st.StopAllocs([0])
        per = [select_on(st, n) for n in nodes]
        assert [r.row for r in per] == [0, 1]
        assert len(per[0].scores) == 1 and 0.50 <= per[0].final_score <= 0.95
        assert per[1].scores == [1.0] and per[1].final_score == 1
        top = select_all(st, nodes, per)
        assert top.row == 1
        return per + [top]
    both(kind_of(name, monkeypatch), scenario)


@pytest.mark.parametrize("name", STACKS_SWEEP)
def test_node_anti_affinity_penalty_nodes(name, monkeypatch):
    """rank_test.go:1708-1742 TestNodeAntiAffinity_PenaltyNodes: the penalty node
    scores -1.0 from the rescheduling-penalty scorer, the other node gets no
    score from it (0.0 in the reference, where nothing else scores)."""
    def scenario(kind):
        nodes = [synth.mock_node("n0"), synth.mock_node("n1")]
        job = synth.mock_job("foo", count=1)
        st = mk(kind.generic(), nodes, [], job)
        opts = SelectOptions(penalty_node_ids=["n0"])
        per = [select_on(st, n, options=opts) for n in nodes]
        assert [r.row for r in per] == [0, 1]
        assert len(per[0].scores) == 2 and per[0].scores[1] == -1.0
        assert len(per[1].scores) == 1
        assert per[1].final_score == per[1].scores[0] == per[0].scores[0]
        assert per[0].final_score == (per[0].scores[0] + -1.0) / 2
        top = select_all(st, nodes, per, options=opts)
        assert top.row == 1
        return per + [top]
    both(kind_of(name, monkeypatch), scenario)
