"""Known-answer tests ported from the reference's scheduler/stack_test.go
(TestServiceStack_SetNodes 57-82 and _Select_ConstraintFilter 310-348 are in
test_reference_kats.py, _Select_CSI 234-308 in test_csi.py).

The reference's GenericStack shuffles the nodes in SetNodes; here the visit
order is an input, so a case whose answer must not depend on the order runs on
both orders. The SystemStack keeps the order it is given. Every engine case
also equals the oracle bit for bit.
"""
import pytest

from nomad_amd import synth
from nomad_amd.stack import SelectOptions
from tests.kat import STACKS, both, kind_of, mk


def mock_nodes(n, prefix="n"):
    return [synth.mock_node("%s%d" % (prefix, i)) for i in range(n)]


def overflow_nodes():
    """Two mock nodes, the second with its whole CPU reserved."""
    nodes = mock_nodes(2)
    nodes[1].reserved_cpu = nodes[1].cpu_shares
    nodes[1].compute_class()
    return nodes


def foo_job():
    job = synth.mock_job()
    job.task_groups[0].tasks[0].driver = "foo"
    return job


def foo_node(nid, value):
    n = synth.mock_node(nid)
    n.attributes["driver.foo"] = value
    n.compute_class()
    return n


@pytest.mark.parametrize("name", STACKS)
def test_service_stack_select_preferring_nodes(name):
    """stack_test.go:124-166 TestServiceStack_Select_PreferringNodes: a preferred
    node outside the stack's node set is selected; one that fails the job's
    constraint (kernel.name windows) is passed over for the stack's own node."""
    def scenario(kind):
        own, pref, pref_win = synth.mock_node("own"), synth.mock_node("pref"), synth.mock_node("pref-win")
        pref_win.attributes["kernel.name"] = "windows"
        pref_win.compute_class()
        st = mk(kind.generic(), [own, pref, pref_win], [], synth.mock_job())
        st.SetNodes([own])
        a = st.Select(0, SelectOptions(preferred_nodes=["pref"]))
        assert a is not None and a.node.id == "pref"
        b = st.Select(0, SelectOptions(preferred_nodes=["pref-win"]))
        assert b is not None and b.node.id == "own"
        return [a, b]
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_service_stack_select_metrics_reset(name):
    """stack_test.go:168-202 TestServiceStack_Select_MetricsReset: with four nodes the
    limit is 2 and each Select evaluates 2 nodes; the second Select's count starts
    from zero again."""
    def scenario(kind):
        nodes = mock_nodes(4)
        st = mk(kind.generic(), nodes, [], synth.mock_job())
        assert st.SetNodes(nodes) == 2
        a, b = st.SelectRaw(0), st.SelectRaw(0)
        assert a.row >= 0 and a.nodes_evaluated == 2
        assert b.row >= 0 and b.nodes_evaluated == 2
        return [a, b]
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_service_stack_select_driver_filter(name):
    """stack_test.go:204-232 TestServiceStack_Select_DriverFilter: only the node
    with driver.foo = 1 takes a task of driver foo, wherever it stands."""
    def scenario(kind):
        nodes = [foo_node("zero", "1"), synth.mock_node("one")]
        trace = []
        for order in ([0, 1], [1, 0]):
            st = mk(kind.generic(), nodes, [], foo_job())
            st.SetNodes(order)
            r = st.SelectRaw(0)
            assert r.row == 0 and r.nodes_filtered == 1
            trace.append(r)
        return trace
    both(kind_of(name), scenario)


def check_overflow(st, r, fit_row):
    assert r.row == fit_row
    assert r.nodes_exhausted == 1
    m = st.LastMetrics()
    assert m["ClassExhausted"] == {"linux-medium-pci": 1}
    assert len(m["ScoreMetaData"]) == 1


@pytest.mark.parametrize("name", STACKS)
def test_service_stack_select_binpack_overflow(name):
    """stack_test.go:350-391 TestServiceStack_Select_BinPack_Overflow: the node whose
    CPU is all reserved is exhausted (NodesExhausted 1, ClassExhausted of its node
    class 1) and the other is selected, with score metadata for that one node."""
    def scenario(kind):
        nodes = overflow_nodes()
        trace = []
        for order in ([0, 1], [1, 0]):
            st = mk(kind.generic(), nodes, [], synth.mock_job(), metrics=True)
            st.SetNodes(order)
            r = st.SelectRaw(0)
            check_overflow(st, r, 0)
            trace.append(r)
        return trace
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_system_stack_set_nodes_and_metrics_reset(name):
    """stack_test.go:393-413 TestSystemStack_SetNodes (the nodes are visited in the
    order given: no shuffle, no limit) and :453-487 TestSystemStack_Select_MetricsReset
    (each Select evaluates 1 node, counted from zero)."""
    def scenario(kind):
        nodes = mock_nodes(8)
        st = mk(kind.system(), nodes, [], synth.mock_job())
        st.SetNodes(nodes)
        a, b = st.SelectRaw(0), st.SelectRaw(0)
        assert a.row == 0 and a.nodes_evaluated == 1
        assert b.row >= 0 and b.nodes_evaluated == 1
        # every node in turn, in the order given (one Select per node, as the system scheduler does)
        per = []
        for i, n in enumerate(nodes):
            st.SetNodes([n])
            per.append(st.SelectRaw(0))
            assert per[-1].row == i
        return [a, b] + per
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_system_stack_select_driver_filter(name):
    """stack_test.go:489-526 TestSystemStack_Select_DriverFilter: driver.foo = 1
    passes, driver.foo = 0 on a new stack filters the node."""
    def scenario(kind):
        trace = []
        for value, want in (("1", 0), ("0", -1)):
            node = foo_node("zero", value)
            st = mk(kind.system(), [node], [], foo_job())
            st.SetNodes([node])
            r = st.SelectRaw(0)
            assert r.row == want and r.nodes_filtered == (0 if want == 0 else 1)
            trace.append(r)
        return trace
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_system_stack_select_constraint_filter(name):
    """stack_test.go:528-567 TestSystemStack_Select_ConstraintFilter: NodesFiltered 1,
    ClassFiltered[linux-medium-pci] 1, ConstraintFiltered["${attr.kernel.name} =
    freebsd"] 1, and the freebsd node is selected."""
    def scenario(kind):
        nodes = mock_nodes(2)
        nodes[1].attributes["kernel.name"] = "freebsd"
        nodes[1].compute_class()
        job = synth.mock_job()
        job.constraints[0].rtarget = "freebsd"
        st = mk(kind.system(), nodes, [], job, metrics=True)
        st.SetNodes(nodes)
        r = st.SelectRaw(0)
        assert r.row == 1 and r.nodes_filtered == 1
        m = st.LastMetrics()
        assert m["ClassFiltered"] == {"linux-medium-pci": 1}
        assert m["ConstraintFiltered"] == {"${attr.kernel.name} = freebsd": 1}
        return [r]
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_system_stack_select_binpack_overflow(name):
    """stack_test.go:569-611 TestSystemStack_Select_BinPack_Overflow: the first node
    is exhausted, the second selected; NodesExhausted 1, ClassExhausted 1, one
    ScoreMetaData entry."""
    def scenario(kind):
        nodes = overflow_nodes()[::-1]          # the full one first
        st = mk(kind.system(), nodes, [], synth.mock_job(), metrics=True)
        st.SetNodes(nodes)
        r = st.SelectRaw(0)
        check_overflow(st, r, 1)
        return [r]
    both(kind_of(name), scenario)
