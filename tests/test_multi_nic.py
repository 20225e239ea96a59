"""Nodes with several host network devices (multi-NIC), and allocs holding
bandwidth on a device other than their node's first.

NetworkIndex keeps bandwidth per device (AvailBandwidth / UsedBandwidth,
nomad/structs/network.go:36-43, 108-114, 196-217); AssignNetwork walks the
node's AvailNetworks in order and takes the first address whose device has
the bandwidth and whose ports are free (yieldIP, network.go:294-315,
407-482); PreemptForNetwork groups its candidates by device
(scheduler/preemption.go:270-455). The engine answers these nodes from the
host's first fit (engine.cpp build_md, TgTables::md); candidates on two
devices make the reference's answer depend on Go map order, which both sides
refuse. The reference pins one case (preemption_test.go:408,
tests/test_preemption.py); the rest is engine vs oracle on random clusters
(parity unpinned beyond the oracle's restatement).
"""
import numpy as np
import pytest

from nomad_amd import synth
from nomad_amd.stack import SelectOptions
from nomad_amd.structs import Allocation, Job, NetworkResource, SchedulerConfig, Task, TaskGroup
from oracle.oracle import OracleGenericStack, OracleSystemStack
from tests.helpers import assert_same_placements, run_place


def _engine(**kw):
    from nomad_amd.stack import GenericStack
    return GenericStack(**kw)


def nic_job(mbits, ports=(), count=1, priority=50, cpu=100, dyn=0, job_id="nic"):
    net = NetworkResource(mode="host", mbits=mbits, dynamic_ports=dyn, reserved_ports=list(ports),
                          port_labels=["p%d" % p for p in ports])
    return Job(id=job_id, priority=priority, task_groups=[TaskGroup(
        name="web", count=count, ephemeral_disk_mb=100,
        tasks=[Task(name="web", driver="exec", cpu=cpu, memory_mb=64, network=net)])])


def group_task_job(gports=(), gdyn=0, mbits=0, tdyn=0, tports=(), count=1, priority=50, cpu=100,
                   job_id="nic-group"):
    """A group network (static ports `gports`, `gdyn` dynamic ones) beside a
    task network (`mbits`, `tdyn` dynamic ports, static ports `tports`)."""
    gnet = NetworkResource(mode="host", dynamic_ports=gdyn, reserved_ports=list(gports),
                           port_labels=["g%d" % p for p in gports])
    tnet = NetworkResource(mode="host", mbits=mbits, dynamic_ports=tdyn, reserved_ports=list(tports),
                           port_labels=["p%d" % p for p in tports])
    return Job(id=job_id, priority=priority, task_groups=[TaskGroup(
        name="web", count=count, ephemeral_disk_mb=100, network=gnet,
        tasks=[Task(name="web", driver="exec", cpu=cpu, memory_mb=64, network=tnet)])])


def nic_cluster(n, seed, two_nic=0.5, absent=0.05, busy=0.0, mixed=True):
    """Nodes with eth0 and, on `two_nic` of them, eth1 (each CIDR one
    address); allocs on either device, a few on a device the node lacks;
    `busy` of the nodes hold extra low-priority allocs (eviction candidates),
    on either device (`mixed`) or on eth0 only, the others then high-priority."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = sorted(synth.uuids(n, seed))
    nodes, allocs = [], []
    for k, nid in enumerate(ids):
        ip0 = "10.%d.%d.%d" % (k >> 16, (k >> 8) & 255, k & 255)
        ip1 = "10.%d.%d.%d" % (128 + (k >> 16), (k >> 8) & 255, k & 255)
        nd = synth.mock_node(nid)
        nd.name = "node-%05d" % k
        nd.reserved_host_ports = [9000] if rng.random() < 0.2 else []
        nets = [NetworkResource(mode="host", device="eth0", cidr=ip0 + "/32", ip=ip0,
                                mbits=int(rng.choice([600, 1000])))]
        two = rng.random() < two_nic
        if two:
            nets.append(NetworkResource(mode="host", device="eth1", cidr=ip1 + "/32", ip=ip1,
                                        mbits=int(rng.choice([400, 1000]))))
        nd.networks = nets
        nd.compute_class()
        nodes.append(nd)
        full = rng.random() < busy
        for q in range(int(rng.integers(0, 4)) + (2 if full else 0)):
            on1 = two and rng.random() < 0.5
            dev, ip = ("eth1", ip1) if on1 else ("eth0", ip0)
            if rng.random() < absent:
                dev, ip = "eth9", "172.16.0.9"
            port = int(rng.choice([8080, 443, 5000]))
            prio = int(rng.choice([20, 30, 95] if full else [50, 95]))
            if not mixed:
                prio = int(rng.choice([20, 30])) if (full and dev == "eth0") else 95
            allocs.append(Allocation(node_id=nid, job_id="svc-%d" % (k % 7 + q), task_group="web",
                                     cpu_shares=1200 if full else 200, memory_mb=128, disk_mb=50,
                                     priority=prio, net_mbits=int(rng.choice([100, 300, 600])),
                                     net_device=dev, ports=[(ip, port)] if rng.random() < 0.5 else []))
    return nodes, allocs


@pytest.mark.gpu
@pytest.mark.parametrize("mbits,ports", [(550, ()), (450, ()), (200, (8080,)), (100, (443, 5000))])
def test_multi_nic_count_loop(mbits, ports):
    """pe_place's count loop: every placement equal to the oracle's, the
    nodes' devices filling one after the other."""
    nodes, allocs = nic_cluster(1200, seed=mbits + len(ports))
    job = nic_job(mbits, ports, count=2500)
    perm = synth.shuffle(len(nodes), 4)
    _, _, ro = run_place(OracleGenericStack, nodes, allocs, job, perm)
    _, _, re = run_place(_engine, nodes, allocs, job, perm)
    assert_same_placements(re, ro)
    assert 0 < sum(1 for x in re if x.row >= 0) < 2500


@pytest.mark.gpu
@pytest.mark.parametrize("ports", [(), (8080,)])
def test_multi_nic_select_commit_metrics(ports):
    """The caller's Select / Commit loop with AllocMetric on: the maps'
    network reasons ("bandwidth exceeded", the port collision of the last
    device tried) equal the oracle's, with plan stops in between."""
    nodes, allocs = nic_cluster(300, seed=11)
    job = nic_job(350, ports, count=400)
    perm = synth.shuffle(len(nodes), 6)
    sts = []
    for cls in (OracleGenericStack, _engine):
        st = cls()
        st.SetState(nodes, allocs)
        st.SetJob(job)
        st.SetNodes(perm)
        st.EnableMetrics(True)
        st.StopAllocs(list(range(0, len(allocs), 9)))
        sts.append(st)
    placed = 0
    for _ in range(400):
        ro, re = (st.SelectRaw(0) for st in sts)
        assert_same_placements([re], [ro])
        assert sts[1].LastMetrics() == sts[0].LastMetrics()
        if ro.row < 0:
            break
        placed += 1
        for st in sts:
            st.Commit(0, ro.row)
    assert placed > 50


def _select_or_refuse(st, opts=None):
    try:
        return st.SelectRaw(0, opts), None
    except Exception as e:   # PE_EUNSUPPORTED / oracle Unsupported
        return None, str(e)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,mixed", [(3, False), (4, False), (5, True)])
def test_multi_nic_preempt_retry(seed, mixed):
    """selectNextOption's loop (generic_sched.go:773-792) on a busy multi-NIC
    cluster: a nil Select retried with Preempt=true; the preempted sets equal
    the oracle's, and a Preempt Select whose candidates sit on two devices is
    refused on both sides (then the caller's chain would answer: the test
    stops there)."""
    nodes, allocs = nic_cluster(200, seed=seed, busy=0.8, absent=0.0, mixed=mixed)
    job = nic_job(700, (), count=150, priority=70, cpu=1500)
    cfg = SchedulerConfig(preempt_service=True)
    perm = synth.shuffle(len(nodes), 2)
    sts = []
    for cls in (OracleGenericStack, _engine):
        st = cls(config=cfg)
        st.SetState(nodes, allocs)
        st.SetJob(job)
        st.SetNodes(perm)
        sts.append(st)
    evicting = refused = 0
    for _ in range(150):
        ro, re = (st.SelectRaw(0) for st in sts)
        assert_same_placements([re], [ro])
        if ro.row < 0:
            (ro, eo), (re, ee) = (_select_or_refuse(st, SelectOptions(preempt=True)) for st in sts)
            assert (eo is None) == (ee is None), (eo, ee)
            if eo is not None:
                refused += 1
                break
            assert_same_placements([re], [ro])
            assert sorted(re.preempted) == sorted(ro.preempted)
            if ro.row < 0:
                break
            evicting += bool(ro.preempted)
        for st in sts:
            st.Commit(0, ro.row, ro.preempted)
    assert (refused > 0) if mixed else (evicting > 0 and refused == 0)


@pytest.mark.gpu
def test_multi_nic_system_stack():
    """SystemScheduler batch (pe_system_place) on a multi-NIC cluster."""
    from nomad_amd.stack import SystemStack
    nodes, allocs = nic_cluster(3000, seed=21)
    job = nic_job(500, (8080,), job_id="sys-nic")
    job.type = 2
    out = []
    for cls in (OracleSystemStack, SystemStack):
        st = cls()
        st.SetState(nodes, allocs)
        st.SetJob(job)
        st.SetNodes(list(range(len(nodes))))
        out.append(st.SystemPlace(0))
    (so, to, po), (se, te, pe) = out
    assert po == pe and (to == te).all()
    m = to == 0
    assert (so[m] == se[m]).all()
    assert 0 < po < len(nodes)


def test_multi_nic_oracle_first_fit():
    """The oracle's AssignNetwork takes eth1 once eth0 is out of bandwidth,
    and the placement's bandwidth stays on eth1 for the next Select."""
    nd = synth.mock_node("n0")
    nd.networks = [NetworkResource(mode="host", device="eth0", cidr="10.0.0.1/32", mbits=1000),
                   NetworkResource(mode="host", device="eth1", cidr="10.1.0.1/32", mbits=1000)]
    nd.compute_class()
    job = nic_job(400, (), count=6)
    st, _, res = run_place(OracleGenericStack, [nd], [], job, [0], count=6)
    # 2 x 400 on eth0, 2 x 400 on eth1, then neither has 400 left
    rows = [r.row for r in res]
    assert rows[:4] == [0, 0, 0, 0] and rows[4] == -1


# ---- group networks beside the task network -----------------------------------
#
# A group network with ports makes the placed alloc's AllocatedSharedResources
# non-empty; AddAllocs (network.go:144-193) then counts those ports and skips
# the alloc's task networks, so a placement's task bandwidth is never added to
# the index the next Select reads. The group's static ports are checked by
# AssignPorts on the group network's address (the engine's static gate), the
# task network by AssignNetwork per device (build_md's first fit).

def _two_node_pair():
    """n0 with eth0 and eth1 at 1000 MBits, n1 the plain mock node (eth0)."""
    n0 = synth.mock_node("n0")
    n0.networks = [NetworkResource(mode="host", device="eth0", cidr="10.0.0.1/32", mbits=1000),
                   NetworkResource(mode="host", device="eth1", cidr="10.1.0.1/32", mbits=1000)]
    n0.compute_class()
    return [n0, synth.mock_node("n1")]


def test_multi_nic_oracle_group_static_port_and_task_bandwidth():
    """Group static port 8080, task network 300 MBits, count 8, on n0 (two
    devices) and n1: rows [0, 1, nil].

    AssignPorts (network.go:317-363) puts 8080 on the first address of the
    "default" host network and refuses it once UsedPorts of that address has
    it. The first placement on a node passes (nothing holds 8080; 300 <= 1000
    on eth0). AddAllocs of that placement sets 8080 on the address (the shared
    ports) and skips its task network, so no bandwidth is consumed, but the
    second AssignPorts on the node collides on 8080. One placement per node,
    whatever its devices: the third Select finds both nodes exhausted."""
    job = group_task_job((8080,), 0, 300, count=8)
    _, _, res = run_place(OracleGenericStack, _two_node_pair(), [], job, [0, 1], count=8)
    assert [r.row for r in res] == [0, 1, -1]


def test_multi_nic_oracle_group_dynamic_port_consumes_no_bandwidth():
    """Group network with one dynamic port, task network 300 MBits and one
    dynamic port, count 8, on n0 and n1: all 8 placed, rows 0, 1, 0, 1, ...

    Every placed alloc has shared ports, so AddAllocs (network.go:144-193)
    counts its group port and skips its task networks: neither the 300 MBits
    nor the task's dynamic port reach the index. Were the bandwidth counted,
    n1 (one device at 1000 MBits) would be exhausted after 3 placements and
    the loop could not alternate to the end; as it is AssignNetwork sees 0
    MBits used on eth0 every time, the group's dynamic ports (at most 8 of
    12001) are far from the range's end, and cpu (100 of 3900 each) does not
    bind. Both nodes are candidates of every Select; the job anti-affinity
    (one more alloc of the job on the node just taken) alternates them."""
    job = group_task_job((), 1, 300, 1, count=8)
    _, _, res = run_place(OracleGenericStack, _two_node_pair(), [], job, [0, 1], count=8)
    assert [r.row for r in res] == [0, 1, 0, 1, 0, 1, 0, 1]


def _two_group_job(count=3):
    """Group a: a task network of 10 MBits and 2 dynamic ports; group b: a
    group network with 2 dynamic ports and no task network."""
    a = TaskGroup(name="a", count=count, ephemeral_disk_mb=10, tasks=[Task(
        name="a", driver="exec", cpu=50, memory_mb=32,
        network=NetworkResource(mode="host", mbits=10, dynamic_ports=2))])
    b = TaskGroup(name="b", count=count, ephemeral_disk_mb=10,
                  network=NetworkResource(mode="host", dynamic_ports=2),
                  tasks=[Task(name="b", driver="exec", cpu=50, memory_mb=32)])
    return Job(id="two-groups", task_groups=[a, b])


STACKS = [pytest.param(OracleGenericStack, id="oracle"),
          pytest.param(_engine, id="engine", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("stack_cls", STACKS)
def test_multi_nic_other_groups_dynamic_ports_fill_the_range(stack_cls):
    """One two-device node whose snapshot alloc holds 11993 dynamic ports;
    Select and Commit in the order a, b, a, b, a: rows 0, 0, 0, 0, nil.

    The dynamic range 20000-32000 has 12001 ports, counted per node by
    AddAllocs whichever group placed them (network.go:144-193: b's shared
    ports, a's task network ports). 11993 + 2 (a) + 2 (b) + 2 (a) + 2 (b) =
    12001: the fifth Select asks for 2 with none free, on eth0 and on eth1
    alike, and AssignNetwork's last error is getDynamicPortsPrecise's
    ("dynamic port selection failed", network.go:421-462). On the engine the
    b commits are another group's plan entries on a multi-device node
    (other_dyn), and each moves a's tables (md_other)."""
    node = _two_node_pair()[0]
    held = Allocation(node_id="n0", job_id="held", task_group="x", cpu_shares=10, memory_mb=10, disk_mb=10,
                      dyn_ports=11993)
    st = stack_cls()
    st.SetState([node], [held])
    st.SetJob(_two_group_job())
    st.SetNodes([0])
    st.EnableMetrics(True)
    rows = []
    for g in (0, 1, 0, 1, 0):
        r = st.SelectRaw(g)
        rows.append(r.row)
        if r.row >= 0:
            st.Commit(g, r.row)
    assert rows == [0, 0, 0, 0, -1]
    assert st.LastMetrics()["DimensionExhausted"] == {"network: dynamic port selection failed": 1}


def _two_nic(nodes, row):
    return len(nodes[row].networks) > 1


def _count_loop_parity(n, count, job, min_two_nic):
    nodes, allocs = nic_cluster(n, seed=41)
    perm = synth.shuffle(n, 4)
    _, _, ro = run_place(OracleGenericStack, nodes, allocs, job, perm, count=count)
    _, _, re = run_place(_engine, nodes, allocs, job, perm, count=count)
    assert_same_placements(re, ro)
    placed = [x.row for x in ro if x.row >= 0]
    on_two = sum(_two_nic(nodes, r) for r in placed)
    print("placed %d of %d, %d on two-device nodes" % (len(placed), count, on_two))
    assert 0 < len(placed) < count
    assert on_two >= min_two_nic


BUG_SHAPE = dict(gports=(8080,), mbits=350)
GROUP_SHAPES = {
    # a group static port outside 20000-32000 and a task bandwidth ask: nothing
    # that AssignNetwork reads moves with a placement (build_md's first fit
    # must end at once, not count towards kMdUnbounded)
    "static-8080+350mbits": (BUG_SHAPE, 400),
    # the static port counts in the dynamic range: commit_dyn = 1
    "static-25000+350mbits": (dict(gports=(25000,), mbits=350), 400),
    "static-443+2-task-dyn": (dict(gports=(443,), tdyn=2), 400),
    "statics-8080-5000+2dyn+700mbits": (dict(gports=(8080, 5000), gdyn=2, mbits=700), 400),
    # no static port: nothing is consumed but cpu (1500 of 3900: two per node),
    # so the count is raised above what 300 nodes hold
    "1dyn+350mbits-1-task-dyn": (dict(gdyn=1, mbits=350, tdyn=1, cpu=1500), 700),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(GROUP_SHAPES))
def test_multi_nic_group_network_count_loop(shape):
    """pe_place's count loop for a group network beside the task network, on
    300 nodes of which 152 have two devices: every record equal to the
    oracle's, the loop ending short of the count, and at least 20 placements
    on two-device nodes (the oracle alone: 180 / 127, 201 / 142, 225 / 138,
    100 / 77 placed / on two-device nodes for the four static shapes)."""
    kw, count = GROUP_SHAPES[shape]
    _count_loop_parity(300, count, group_task_job(count=count, **kw), 20)


@pytest.mark.gpu
def test_multi_nic_group_static_port_40_nodes():
    """The shape that made build_md's first fit spin (a group static port
    outside the dynamic range, a task network asking bandwidth only), alone on
    40 nodes of which 21 have two devices: the group port admits one placement
    per node, so the oracle places 24 of 60, 18 of them on two-device nodes."""
    _count_loop_parity(40, 60, group_task_job(count=60, **BUG_SHAPE), 10)


def _stop_loop(job, metrics, count=400, stops_after=(10, 40)):
    """The caller's Select / Commit loop on the oracle and the engine, every
    record (and with `metrics` every AllocMetric) compared. After the
    placements `stops_after`, StopAllocs of up to twenty snapshot allocs that
    hold bandwidth on two-device nodes the group is already placed on (taken
    from the oracle's records): the engine drops its speculation and rebuilds
    the group's tables with those placements replayed onto their devices.
    Returns (placed rows, the rows with stops, the later placements on them,
    the engine)."""
    nodes, allocs = nic_cluster(300, seed=41)
    perm = synth.shuffle(300, 4)
    row_of = {nd.id: k for k, nd in enumerate(nodes)}
    sts = []
    for cls in (OracleGenericStack, _engine):
        st = cls()
        st.SetState(nodes, allocs)
        st.SetJob(job)
        st.SetNodes(perm)
        if metrics:
            st.EnableMetrics(True)
        sts.append(st)
    placed, stopped, freed, later = [], set(), set(), 0
    for _ in range(count):
        ro, re = (st.SelectRaw(0) for st in sts)
        assert_same_placements([re], [ro])
        if metrics:
            assert sts[1].LastMetrics() == sts[0].LastMetrics()
        if ro.row < 0:
            break
        for st in sts:
            st.Commit(0, ro.row)
        later += ro.row in freed
        placed.append(ro.row)
        if len(placed) in stops_after:
            have = {r for r in placed if _two_nic(nodes, r)}
            pick = [i for i, a in enumerate(allocs)
                    if i not in stopped and a.net_mbits > 0 and row_of[a.node_id] in have][:20]
            assert pick
            for st in sts:
                st.StopAllocs(pick)
            stopped.update(pick)
            freed.update(row_of[allocs[i].node_id] for i in pick)
    assert len(stopped) >= 20
    return placed, freed, later, sts[1]


@pytest.mark.gpu
def test_multi_nic_served_loop_task_port_with_stops():
    """Select / Commit without metrics and without preemption is served from
    the speculative count loop; nic_job(350, (8080,)) on a multi-device
    cluster, with stops after placements 10 and 40. The task port 8080 goes on
    the device's address, so a two-device node takes two placements: one lands
    on a node after a stop freed bandwidth under the group's first placement
    (the replayed md_hist decides which device is left)."""
    placed, _, later, eng = _stop_loop(nic_job(350, (8080,), count=400), metrics=False)
    assert 50 < len(placed) < 400
    assert later >= 1
    assert eng.SpeculationStats()[1] > 0   # Selects answered from records


@pytest.mark.gpu
def test_multi_nic_served_loop_group_port_with_stops():
    """The same loop for the group static port 8080 beside 350 MBits. The
    group port admits one placement per node (the pin above), so no later
    placement can land on a node the group already holds, freed or not: the
    rebuilt tables must keep those nodes shut while the loop goes on to other
    two-device nodes."""
    placed, _, later, eng = _stop_loop(group_task_job(count=400, **BUG_SHAPE), metrics=False)
    assert 50 < len(placed) < 400
    assert later == 0 and len(set(placed)) == len(placed)
    nodes, _ = nic_cluster(300, seed=41)
    assert sum(_two_nic(nodes, r) for r in placed[40:]) >= 20
    assert eng.SpeculationStats()[1] > 0


@pytest.mark.gpu
def test_multi_nic_metrics_loop_group_port_with_stops():
    """The loop with AllocMetric on (per-Select path, no speculation) and the
    same mid-loop stops: every Select's maps equal the oracle's."""
    placed, _, later, _ = _stop_loop(group_task_job(count=400, **BUG_SHAPE), metrics=True)
    assert 50 < len(placed) < 400 and later == 0


@pytest.mark.gpu
@pytest.mark.parametrize("metrics", [False, True], ids=["plain", "metrics"])
def test_multi_nic_other_groups_dynamic_ports_on_a_cluster(metrics):
    """120 nodes, every third holding an alloc with 11980-11999 dynamic ports
    (1 to 10 further pairs fit); Selects of a (task network, 2 dynamic ports)
    with commits of b (group network, 2 dynamic ports) in between, both
    landing on the same nodes. Each b commit is another group's plan entry:
    a's multi-device tables are stale after it and are rebuilt with b's ports
    counted (other_dyn). Record by record against the oracle."""
    nodes, allocs = nic_cluster(120, seed=43)
    rng = np.random.Generator(np.random.PCG64(7))
    near = set()
    for k in range(0, 120, 3):
        allocs.append(Allocation(node_id=nodes[k].id, job_id="ports", task_group="x", cpu_shares=10, memory_mb=10,
                                 disk_mb=10, dyn_ports=int(rng.integers(11980, 12000))))
        near.add(k)
    job = _two_group_job(count=200)
    perm = synth.shuffle(120, 5)
    sts = []
    for cls in (OracleGenericStack, _engine):
        st = cls()
        st.SetState(nodes, allocs)
        st.SetJob(job)
        st.SetNodes(perm)
        if metrics:
            st.EnableMetrics(True)
        sts.append(st)
    got = {0: [], 1: []}
    exhausted = 0
    for i in range(150):
        for g in ((0, 1) if i % 3 else (0,)):   # two Selects of a in a row now and then
            ro, re = (st.SelectRaw(g) for st in sts)
            assert_same_placements([re], [ro])
            if metrics:
                assert sts[1].LastMetrics() == sts[0].LastMetrics()
            assert ro.row >= 0
            exhausted += g == 0 and ro.nodes_exhausted > 0
            for st in sts:
                st.Commit(g, ro.row)
            got[g].append(ro.row)
    shared = {r for r in got[0] if r in near and _two_nic(nodes, r)} & set(got[1])
    print("a Selects with exhausted nodes: %d; near-full two-device nodes holding both groups: %d"
          % (exhausted, len(shared)))
    assert exhausted >= 5 and len(shared) >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [3, 4])
def test_multi_nic_preempt_retry_group_port(seed):
    """test_multi_nic_preempt_retry's loop (eviction candidates on eth0 only)
    for a job that adds the group static port 8080 to the 700 MBits task ask:
    the preempted sets equal the oracle's, and both sides agree on every
    refusal (the oracle evicts on 67 and 71 Selects and refuses none)."""
    nodes, allocs = nic_cluster(200, seed=seed, busy=0.8, absent=0.0, mixed=False)
    job = group_task_job((8080,), 0, 700, count=150, priority=70, cpu=1500)
    cfg = SchedulerConfig(preempt_service=True)
    perm = synth.shuffle(len(nodes), 2)
    sts = []
    for cls in (OracleGenericStack, _engine):
        st = cls(config=cfg)
        st.SetState(nodes, allocs)
        st.SetJob(job)
        st.SetNodes(perm)
        sts.append(st)
    evicting = refused = 0
    for _ in range(150):
        ro, re = (st.SelectRaw(0) for st in sts)
        assert_same_placements([re], [ro])
        if ro.row < 0:
            (ro, eo), (re, ee) = (_select_or_refuse(st, SelectOptions(preempt=True)) for st in sts)
            assert (eo is None) == (ee is None), (eo, ee)
            if eo is not None:
                refused += 1
                break
            assert_same_placements([re], [ro])
            assert sorted(re.preempted) == sorted(ro.preempted)
            if ro.row < 0:
                break
            evicting += bool(ro.preempted)
        for st in sts:
            st.Commit(0, ro.row, ro.preempted)
    print("evicting Selects: %d, refused: %d" % (evicting, refused))
    assert evicting > 0 and refused == 0


def _record_key(r):
    if r is None:
        return None
    return (r.row, r.final_score, tuple(r.scores), r.nodes_evaluated, r.nodes_filtered, r.nodes_exhausted,
            r.new_offset, tuple(r.preempted))


@pytest.mark.gpu
def test_multi_nic_inplace_update_fallback():
    """pe_inplace_update refuses a task network on a multi-device cluster;
    InplaceUpdate's fallback=True answer (the per-Select sequence on the
    engine) equals inplace_update_by_select on the oracle, and so do the
    placements and the eligibility memo afterwards."""
    from nomad_amd.stack import Unsupported, inplace_update_by_select
    nodes, allocs = nic_cluster(200, seed=51)
    rng = np.random.Generator(np.random.PCG64(52))
    for k in rng.integers(0, 200, size=60):   # an older version's allocs, several on some nodes
        nd = nodes[int(k)]
        dev = nd.networks[int(rng.integers(0, len(nd.networks)))].device
        allocs.append(Allocation(node_id=nd.id, job_id="nic", task_group="web", cpu_shares=100, memory_mb=64,
                                 disk_mb=100, net_mbits=200, net_device=dev))
    job = nic_job(450, (), count=60)
    job.version = 3
    own = [i for i, a in enumerate(allocs) if a.job_id == "nic"]
    upd = [own[int(k)] for k in rng.permutation(len(own))]

    def make(cls):
        st = cls()
        st.SetState(nodes, allocs)
        st.SetJob(job)
        return st

    with pytest.raises(Unsupported):
        make(_engine).InplaceUpdate(0, upd, fallback=False)
    eng, ora = make(_engine), make(OracleGenericStack)
    re, se = eng.InplaceUpdate(0, upd)
    ro, so = inplace_update_by_select(ora, 0, upd)
    assert [int(x) for x in se] == [int(x) for x in so]
    assert [_record_key(r) for r in re] == [_record_key(r) for r in ro]
    assert {0, 2} <= set(so)   # updated in place, and exhausted where 450 no longer fits the device
    perm = synth.shuffle(200, 8)
    for st in (eng, ora):
        st.SetNodes(perm)
    for _ in range(30):
        xo, xe = (st.SelectRaw(0) for st in (ora, eng))
        assert_same_placements([xe], [xo])
        if xo.row < 0:
            break
        for st in (eng, ora):
            st.Commit(0, xo.row)
    assert eng.Eligibility() == ora.Eligibility()


def _system_engine(**kw):
    from nomad_amd.stack import SystemStack
    return SystemStack(**kw)


def _sys_after(st, rows, extra):
    """The state after a system pass: the eligibility maps and a further
    SystemPlace of a group that was not listed."""
    el = st.Eligibility()
    st.SetNodes(rows)
    sc, ss, p = st.SystemPlace(extra)
    return {"job": el["job"], "tgs": el["tgs"]}, np.where(ss == 0, sc, np.nan), ss, p


def _same_system(a, o):
    """SystemPlaceGroups*' results: outcomes, counts and evictions equal, the
    FinalScores within 1e-12 relative of the oracle's (README)."""
    assert np.array_equal(a[1], o[1]) and np.array_equal(a[2], o[2]) and a[3] == o[3]
    m = o[1] == 0
    assert np.allclose(a[0][m], o[0][m], rtol=1e-12, atol=0.0)
    assert np.isnan(a[0][~m]).all()
    if len(o) > 4:
        assert a[4] == o[4]
    if len(o) > 5:
        assert a[5]["failed"] == o[5]["failed"]
        assert set(a[5]["scores"]) == set(o[5]["scores"])
        for key, named in o[5]["scores"].items():
            assert set(named) == set(a[5]["scores"][key])
            for name, v in named.items():
                assert np.isclose(a[5]["scores"][key][name], v, rtol=1e-12, atol=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("call", ["groups", "preempt", "metrics"])
def test_multi_nic_system_groups_fallback(call):
    """pe_system_place_groups* refuse a task network on a multi-device
    cluster; the wrappers' fallback=True answers equal the oracle's by-select
    helpers for a two-group system job whose first group has a task network,
    and the state afterwards is the same."""
    from nomad_amd import stack as S
    nodes, allocs = nic_cluster(200, seed=52, busy=0.6, absent=0.0, mixed=False)
    job = synth.mock_system_job("sys-nic-groups")
    job.priority = 70
    net = NetworkResource(mode="host", mbits=450, dynamic_ports=1)
    mk = lambda name, cpu, nw=None: TaskGroup(name=name, count=1, ephemeral_disk_mb=50, tasks=[   # noqa: E731
        Task(name=name, driver="exec", cpu=cpu, memory_mb=64, network=nw)])
    job.task_groups = [mk("a", 300, net), mk("b", 1500), mk("extra", 400)]
    cfg = SchedulerConfig(preempt_system=True) if call != "groups" else None
    rows = synth.shuffle(200, 3)
    name, helper = {"groups": ("SystemPlaceGroups", S.system_place_groups_by_select),
                    "preempt": ("SystemPlaceGroupsPreempt", S.system_place_groups_preempt_by_select),
                    "metrics": ("SystemPlaceGroupsMetrics", S.system_place_groups_metrics_by_select)}[call]

    def make(cls):
        st = cls(config=cfg)
        st.SetState(nodes, allocs)
        st.SetJob(job)
        st.SetNodes(rows)
        if call == "metrics":
            st.EnableMetrics(True)
        return st

    with pytest.raises(S.Unsupported):
        getattr(make(_system_engine), name)([0, 1], fallback=False)
    eng, ora = make(_system_engine), make(OracleSystemStack)
    ra = getattr(eng, name)([0, 1])
    ro = helper(ora, [0, 1])
    _same_system(ra, ro)
    two = np.array([_two_nic(nodes, int(r)) for r in rows])
    assert (ro[1][two, 0] == 0).sum() >= 20 and (ro[1][:, 0] == 2).any()
    if call != "groups":
        assert ro[4]   # some entry evicted
    (ea, sa, ta, pa), (eo, so, to, po) = (_sys_after(st, rows, 2) for st in (eng, ora))
    assert ea == eo and np.array_equal(ta, to) and pa == po
    assert np.allclose(sa[to == 0], so[to == 0], rtol=1e-12, atol=0.0)


@pytest.mark.gpu
def test_multi_nic_system_stack_group_port():
    """test_multi_nic_system_stack's comparison for the group static port
    beside the task bandwidth ask, on 300 nodes."""
    nodes, allocs = nic_cluster(300, seed=21)
    job = group_task_job(job_id="sys-nic-group", **BUG_SHAPE)
    job.type = 2
    out = []
    for cls in (OracleSystemStack, _system_engine):
        st = cls()
        st.SetState(nodes, allocs)
        st.SetJob(job)
        st.SetNodes(list(range(len(nodes))))
        out.append(st.SystemPlace(0))
    (so, to, po), (se, te, pe) = out
    assert po == pe and (to == te).all()
    m = to == 0
    assert (so[m] == se[m]).all()
    assert 0 < po < len(nodes)
    assert sum(_two_nic(nodes, r) for r in np.flatnonzero(m)) >= 20
