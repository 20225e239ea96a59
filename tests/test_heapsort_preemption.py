"""heapSort_func through the real Preemptor: one node whose single priority
group is a killer input of Go 1.16's sort.Slice (tests/test_go_sort.py), so
that PreemptForNetwork's per-group sort (scheduler/preemption.go:270-410;
evict.inc's go_sort_keyed over the group) runs past quickSort_func's depth
limit and falls back to heapSort_func.

Every alloc of the group holds `base - rank_i` MBits of the node's one network
device, rank_i the killer's key, and the ask needs ten times `base`: the
group's sort key |needed - mbits| / needed rises with the rank, the sort sees
the ranks in alloc order, and the bandwidth need takes a strict prefix of the
sorted group. With the ranks halved the group holds equal keys and the
preempted set depends on the order heapSort_func leaves them in. The oracle's
heapSort counter must rise during the Select, or the case proves nothing.
"""
import numpy as np
import pytest

from nomad_amd import synth
from nomad_amd.stack import SelectOptions
from nomad_amd.structs import Allocation, Job, NetworkResource, Task, TaskGroup
from oracle import oracle
from oracle.oracle import OracleGenericStack


def _engine(**kw):
    from nomad_amd.stack import GenericStack
    return GenericStack(**kw)


# (allocs on the node, ranks halved): n > 32, so the engine evaluates the node
# at the wide eviction width (uint16_t indices)
CASES = [(41, False), (100, True), (250, False), (250, True)]


def killer_node(n, halved):
    ranks = oracle.sort_killer(n)
    if halved:
        ranks = np.floor(ranks / 2.0)
    base = n + 60
    mbits = [base - int(r) for r in ranks]
    nd = synth.mock_node("node-0")
    nd.cpu_shares, nd.memory_mb, nd.disk_mb = 64000, 131072, 400 * 1024
    nd.reserved_host_ports = []
    nd.networks = [NetworkResource(mode="host", device="eth0", cidr="192.168.0.100/32", mbits=sum(mbits))]
    nd.compute_class()
    allocs = [Allocation(node_id=nd.id, job_id="low-%d" % (i % 5), task_group="web", cpu_shares=20, memory_mb=32,
                         disk_mb=0, priority=30, net_mbits=m) for i, m in enumerate(mbits)]
    needed = 10 * base
    job = Job(id="preemptor", priority=100, task_groups=[TaskGroup(name="web", count=1, ephemeral_disk_mb=0, tasks=[
        Task(name="web", driver="exec", cpu=500, memory_mb=256, network=NetworkResource(mbits=needed))])])
    return nd, allocs, job, np.array(mbits), needed


def select_preempt(stack_cls, nd, allocs, job):
    st = stack_cls()
    st.SetState([nd], allocs)
    st.SetJob(job)
    st.SetNodes([nd])
    assert st.SelectRaw(0).row == -1   # the bandwidth is all in use: no fit without eviction
    return st.SelectRaw(0, SelectOptions(preempt=True))


def oracle_select(n, halved):
    nd, allocs, job, mbits, needed = killer_node(n, halved)
    oracle.sort_heap_reset()
    r = select_preempt(OracleGenericStack, nd, allocs, job)
    return r, oracle.sort_heap_stats(), (nd, allocs, job, mbits, needed)


@pytest.mark.parametrize("n,halved", CASES)
def test_oracle_preemptor_reaches_heapsort(n, halved):
    r, (calls, elems, ties), (_, _, _, mbits, needed) = oracle_select(n, halved)
    assert calls >= 1 and elems > 12, (calls, elems)
    assert (ties > 0) == halved
    assert r.row == 0
    got = sorted(r.preempted)
    assert 1 < len(got) < n // 2   # a strict prefix of the sorted group
    assert mbits[got].sum() >= needed
    if not halved:
        # distinct keys: the set is the largest allocs, less those the closing
        # superset filter (largest distance first) finds it can do without
        order = np.argsort(-mbits, kind="stable")
        k = int(np.searchsorted(np.cumsum(mbits[order]), needed)) + 1
        prefix = order[:k]
        kept, avail = [], 0
        for i in prefix[::-1]:
            kept.append(int(i))
            avail += int(mbits[i])
            if avail >= needed:
                break
        assert got == sorted(kept)


@pytest.mark.gpu
@pytest.mark.parametrize("n,halved", CASES)
def test_engine_equals_oracle_through_heapsort(n, halved):
    ro, (calls, _, _), (nd, allocs, job, _, _) = oracle_select(n, halved)
    assert calls >= 1
    re = select_preempt(_engine, nd, allocs, job)
    assert re.row == ro.row == 0
    assert sorted(re.preempted) == sorted(ro.preempted)
    assert re.final_score == ro.final_score and re.scores == ro.scores
    assert (re.nodes_evaluated, re.nodes_filtered, re.nodes_exhausted) == \
        (ro.nodes_evaluated, ro.nodes_filtered, ro.nodes_exhausted)
