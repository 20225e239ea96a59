"""Known-answer tests ported from the reference's nomad/structs/network_test.go,
as far as a Select shows a NetworkIndex: what a task network ask is offered
(AssignNetwork), what the index counts as used (SetNode, AddAllocs) and which
addresses it tries (yieldIP) are read from whether the node takes the ask and,
when it does not, from the DimensionExhausted text.
"""
import pytest

from nomad_amd import synth
from nomad_amd.structs import Allocation, Job, NetworkResource, Task, TaskGroup
from tests.kat import STACKS, both, kind_of, mk, select_on

MIN_DYNAMIC_PORT, MAX_DYNAMIC_PORT = 20000, 32000     # structs/network.go:14-20


def net_node(cidr, reserved_host_ports=()):
    n = synth.mock_node("n0")
    n.networks = [NetworkResource(mode="host", device="eth0", cidr=cidr, mbits=1000)]
    n.reserved_host_ports = list(reserved_host_ports)
    n.compute_class()
    return n


def task_job(mbits=0, dyn=0, ports=(), labels=()):
    net = NetworkResource(device="eth0", mbits=mbits, dynamic_ports=dyn, reserved_ports=list(ports),
                          port_labels=list(labels))
    return Job(id="net", task_groups=[TaskGroup(name="web", count=1, ephemeral_disk_mb=10, tasks=[
        Task(name="web", driver="exec", cpu=100, memory_mb=64, network=net)])])


def held():
    """TestNetworkIndex_AssignNetwork's allocs: 20 MBits with ports 8000 and 9000,
    50 MBits with port 10000, all on 192.168.0.100."""
    return [Allocation(node_id="n0", job_id="a", task_group="web", cpu_shares=100, memory_mb=64, net_mbits=20,
                       ports=[("192.168.0.100", 8000), ("192.168.0.100", 9000)]),
            Allocation(node_id="n0", job_id="b", task_group="api", cpu_shares=100, memory_mb=64, net_mbits=50,
                       ports=[("192.168.0.100", 10000)])]


def ask(kind, node, allocs, job, trace):
    st = mk(kind.generic(), [node], allocs, job, metrics=True)
    r = select_on(st, node)
    trace.append(r)
    return r, st.LastMetrics()["DimensionExhausted"]


@pytest.mark.parametrize("name", STACKS)
def test_assign_network_bandwidth_and_collision(name):
    """network_test.go:206-305 TestNetworkIndex_AssignNetwork on a one-address
    network, with :90-143 TestNetworkIndex_AddAllocs (UsedBandwidth 70, the three
    ports used) and :55-88 TestNetworkIndex_SetNode (ReservedHostPorts 22 used):
    with 70 of 1000 MBits held an ask of 930 is offered and 931 is "bandwidth
    exceeded"; a static port an alloc holds, or the node reserves, collides."""
    def scenario(kind):
        node = net_node("192.168.0.100/32", reserved_host_ports=[22])
        trace = []
        r, _ = ask(kind, node, held(), task_job(mbits=930), trace)
        assert r.row == 0
        r, dims = ask(kind, node, held(), task_job(mbits=931), trace)
        assert r.row == -1 and dims == {"network: bandwidth exceeded": 1}
        r, dims = ask(kind, node, held(), task_job(mbits=1000), trace)          # the reference's own ask
        assert r.row == -1 and dims == {"network: bandwidth exceeded": 1}
        for port in (8000, 9000, 10000, 22):
            r, dims = ask(kind, node, held(), task_job(ports=[port], labels=["main"]), trace)
            assert r.row == -1 and dims == {"network: reserved port collision main=%d" % port: 1}
        r, _ = ask(kind, node, held(), task_job(dyn=3, ports=[2345], labels=["main"]), trace)   # reserved + dynamic
        assert r.row == 0
        r, _ = ask(kind, node, [], task_job(mbits=1000), trace)                 # nothing held: the whole link
        assert r.row == 0
        return trace
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_assign_network_walks_the_cidr(name):
    """network_test.go:178-204 TestNetworkIndex_yieldIP and :253-263 of
    TestNetworkIndex_AssignNetwork: on 192.168.0.100/30 port 8000 is held on .100
    and the ask for it is offered the next address, .101, so the node takes it.
    The oracle gives the reference's answer; the engine places task static ports
    only where the network's CIDR is one known address and refuses this case."""
    kind = kind_of(name)
    node = net_node("192.168.0.100/30")
    job = task_job(ports=[8000], labels=["main"])
    if kind.is_oracle:
        r, _ = ask(kind, node, held(), job, [])
        assert r.row == 0
        return
    from nomad_amd.stack import Unsupported
    with pytest.raises(Unsupported):
        ask(kind, node, held(), job, [])


@pytest.mark.parametrize("name", STACKS)
def test_assign_network_cidr_bandwidth(name):
    """The bandwidth step of TestNetworkIndex_AssignNetwork on its own /30 network:
    bandwidth is per device, whichever address is offered."""
    def scenario(kind):
        node = net_node("192.168.0.100/30")
        trace = []
        r, _ = ask(kind, node, held(), task_job(mbits=930), trace)
        assert r.row == 0
        r, dims = ask(kind, node, held(), task_job(mbits=931), trace)
        assert r.row == -1 and dims == {"network: bandwidth exceeded": 1}
        return trace
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_assign_network_dynamic_contention(name):
    """network_test.go:309-352 TestNetworkIndex_AssignNetwork_Dynamic_Contention: the
    node reserves every dynamic port but the last (32000); a one-port ask is still
    offered it, a two-port ask is "dynamic port selection failed"."""
    def scenario(kind):
        node = net_node("192.168.0.100/32", reserved_host_ports=range(MIN_DYNAMIC_PORT, MAX_DYNAMIC_PORT))
        trace = []
        r, _ = ask(kind, node, [], task_job(dyn=1), trace)
        assert r.row == 0
        r, dims = ask(kind, node, [], task_job(dyn=2), trace)
        assert r.row == -1 and dims == {"network: dynamic port selection failed": 1}
        return trace
    both(kind_of(name), scenario)
