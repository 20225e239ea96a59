"""Known-answer tests ported from the reference's scheduler/feasible_test.go:
the checker tables that no other file cites (host volumes, network modes and
the bridge upgrade path, driver info / compatibility / health, the
FeasibilityWrapper's use of the eligibility memo, checkSetContainsAny and
checkAttributeConstraint).

A checker's verdict is read at the Stack boundary as nodes_filtered of a Select
over the one node. The FeasibilityWrapper memoises task-group verdicts per
computed class, and host volumes, drivers and NodeResources.Networks are not
part of the class hash (node_class.go:43-50), so every table row runs on a
fresh stack; test_shared_class_reuses_the_first_verdict pins the memoised
behaviour itself.
"""
import pytest

from nomad_amd import synth
from nomad_amd.structs import Allocation, Constraint, DriverInfo, Job, NetworkResource, Task, TaskGroup
from tests.kat import STACKS, both, kind_of, mk, select_on
from tests.test_reference_kats_attribute import CHECKERS as ATTR_CHECKERS
from tests.test_semantics import CHECKERS as CONSTRAINT_CHECKERS


def job_of(drivers=("exec",), network=None, host_volumes=(), constraints=()):
    tasks = [Task(name="t%d" % i, driver=d, cpu=100, memory_mb=64) for i, d in enumerate(drivers)]
    return Job(id="feas", constraints=list(constraints), task_groups=[TaskGroup(
        name="web", count=1, ephemeral_disk_mb=10, network=network, host_volumes=list(host_volumes), tasks=tasks)])


def passes(kind, node, job, trace, placed=True):
    """The task group's checkers on one node, on a stack of its own."""
    st = mk(kind.generic(), [node], [], job)
    r = select_on(st, node)
    trace.append(r)
    assert r.nodes_evaluated == 1
    assert r.nodes_filtered in (0, 1)
    if r.nodes_filtered == 0 and placed:
        assert r.row == 0 and r.nodes_exhausted == 0      # every node here has room for the ask
    return r.nodes_filtered == 0


def table(kind, rows):
    """rows: (node, job, expected verdict[, whether a passing node must also be placed])."""
    trace = []
    for i, (node, job, want, *placed) in enumerate(rows):
        assert passes(kind, node, job, trace, *placed) == want, i
    return trace


def vol_node(nid, volumes):
    n = synth.mock_node(nid)
    n.host_volumes = dict(volumes)
    return n


@pytest.mark.parametrize("name", STACKS)
def test_host_volume_checker(name):
    """feasible_test.go:84-164 TestHostVolumeChecker (the request of type "nothost"
    is dropped by SetVolumes and is no host volume ask here) and :166-232
    TestHostVolumeChecker_ReadOnly."""
    def scenario(kind):
        ask = [("foo", False), ("bar", False)]
        nodes = [vol_node("n0", {}), vol_node("n1", {"foo": False}), vol_node("n2", {"foo": False, "bar": False}),
                 vol_node("n3", {"foo": False, "bar": False}), vol_node("n4", {"foo": False, "baz": False})]
        rows = [(nodes[0], job_of(host_volumes=ask), False),      # no volumes, some requested
                (nodes[1], job_of(host_volumes=ask), False),      # mismatched set
                (nodes[2], job_of(host_volumes=ask), True),       # happy path
                (nodes[3], job_of(), True),                       # none requested
                (nodes[4], job_of(), True)]
        ro, rw = vol_node("ro", {"foo": True}), vol_node("rw", {"foo": False})
        rows += [(ro, job_of(host_volumes=[("foo", False)]), False),   # read-write request, read-only host
                 (ro, job_of(host_volumes=[("foo", True)]), True),
                 (rw, job_of(host_volumes=[("foo", True)]), True),
                 (rw, job_of(host_volumes=[("foo", False)]), True)]
        return table(kind, rows)
    both(kind_of(name), scenario)


def mode_node(nid, mode, version="0.12.0"):
    """TestNetworkChecker's node(mode): mock.Node() plus a network of `mode`; the
    bridge nodes carry the aliases public and private instead of default."""
    n = synth.mock_node(nid)
    if mode:
        n.networks.append(NetworkResource(mode=mode, device="", cidr="", mbits=0))
    if mode == "bridge":
        n.host_network_aliases = ["private", "public"]
        n.addresses = [("public", "192.168.0.100", ""), ("private", "192.168.0.101", "")]
    n.attributes["nomad.version"] = version
    n.meta.update({"public_network": "public", "private_network": "private", "wrong_network": "empty"})
    n.compute_class()
    return n


def port_ask(mode, host_network=None):
    if host_network is None:
        return NetworkResource(mode=mode)
    return NetworkResource(mode=mode, dynamic_ports=1, host_network=host_network)


# feasible_test.go:463-564: (ask, verdict on [bridge, bridge, cni/mynet]). The row with two
# ports on two host networks (:475-495) needs a host network per port, which a
# NetworkResource here does not carry: its single-port halves are the two rows after it.
NETWORK_CASES = [
    (("host", None), [True, True, True]),
    (("bridge", None), [True, True, False]),
    (("bridge", "${meta.public_network}"), [True, True, False]),
    (("bridge", "${meta.private_network}"), [True, True, False]),
    (("bridge", "${meta.wrong_network}"), [False, False, False]),
    (("bridge", "${meta.nonetwork}"), [False, False, False]),
    (("bridge", "public"), [True, True, False]),
    (("bridge", "${meta.private_network}-nonexisting"), [False, False, False]),
    (("cni/mynet", None), [False, False, True]),
    (("cni/nonexistent", None), [False, False, False]),
]


@pytest.mark.parametrize("name", STACKS)
def test_network_checker(name):
    """feasible_test.go:430-572 TestNetworkChecker: host, bridge and cni/* modes, and
    a port's host network given literally or through ${meta.*}."""
    def scenario(kind):
        nodes = [mode_node("n0", "bridge"), mode_node("n1", "bridge"), mode_node("n2", "cni/mynet")]
        # The checker's verdict is what the reference asserts. A ${...} host network that
        # passes it is not yet resolved again by bin-pack (rank.go:250-270 does; DESIGN
        # section 49 lists TestBinPackIterator_Network_Interpolation_* as open), so those
        # rows do not ask for a placement.
        rows = [(n, job_of(network=port_ask(*ask)), w, not (ask[1] or "").startswith("${"))
                for ask, want in NETWORK_CASES for n, w in zip(nodes, want)]
        return table(kind, rows)
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_network_checker_bridge_upgrade_path(name):
    """feasible_test.go:574-602: a client older than 0.12 never fingerprinted a
    bridge network and still takes a bridge ask; a 0.12 client without one does not."""
    def scenario(kind):
        job = job_of(network=port_ask("bridge"))
        return table(kind, [(mode_node("old", "", "0.11.0"), job, True),
                            (mode_node("new", "", "0.12.0"), job, False)])
    both(kind_of(name), scenario)


def driver_node(nid, drivers=None, attrs=()):
    n = synth.mock_node(nid)
    if drivers is not None:
        n.drivers = dict(drivers)
    n.attributes.update(dict(attrs))
    n.compute_class()
    return n


@pytest.mark.parametrize("name", STACKS)
def test_driver_checker(name):
    """feasible_test.go:604-652 TestDriverChecker_DriverInfo (detected and healthy,
    unhealthy, undetected), :653-702 TestDriverChecker_Compatibility (no
    DriverInfo: the driver.* attribute through ParseBool) and :704-765
    Test_HealthChecks (one driver per node)."""
    def scenario(kind):
        mock = synth.mock_node("m").drivers
        two = job_of(drivers=("exec", "foo"))
        rows = [(driver_node("i0", dict(mock, foo=DriverInfo(True, True))), two, True),
                (driver_node("i1", dict(mock, foo=DriverInfo(True, False))), two, False),
                (driver_node("i2", dict(mock, foo=DriverInfo(False, False))), two, False)]
        for i, (v, want) in enumerate([("1", True), ("0", False), ("true", True), ("False", False)]):
            rows.append((driver_node("c%d" % i, {}, {"driver.foo": v}), two, want))
        rows += [(driver_node("h0", {"foo": DriverInfo(True, True)}, {"driver.foo": "1"}), job_of(("foo",)), True),
                 (driver_node("h1", {"bar": DriverInfo(True, False)}, {"driver.bar": "1"}), job_of(("bar",)), False),
                 (driver_node("h2", {"baz": DriverInfo(False, False)}, {"driver.baz": "0"}), job_of(("baz",)), False)]
        return table(kind, rows)
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_shared_class_reuses_the_first_verdict(name):
    """Reference behaviour the tables above step around: drivers are not in the
    computed class, so on one stack the FeasibilityWrapper applies the first
    node's task-group verdict to every later node of the class
    (feasible.go:1080-1147, node_class.go:43-50), whichever way it went."""
    def scenario(kind):
        mock = synth.mock_node("m").drivers
        good = driver_node("good", dict(mock, foo=DriverInfo(True, True)))
        bad = driver_node("bad", dict(mock, foo=DriverInfo(True, False)))
        assert good.computed_class == bad.computed_class
        trace = []
        for order, want in (([good, bad], [0, 0]), ([bad, good], [1, 1])):
            st = mk(kind.generic(), [good, bad], [], job_of(drivers=("exec", "foo")))
            for n, w in zip(order, want):
                r = select_on(st, n)
                assert r.nodes_filtered == w, (n.id, w)
                trace.append(r)
        return trace
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_constraint_checker(name):
    """feasible_test.go:767-825 TestConstraintChecker: datacenter = dc1, kernel.name
    is linux, node.class != linux-medium-pci and attr.foo is_set hold together on
    the third node only."""
    def scenario(kind):
        nodes = [synth.mock_node("n%d" % i) for i in range(3)]
        nodes[0].attributes["kernel.name"] = "freebsd"
        nodes[1].datacenter = "dc2"
        nodes[2].node_class = "large"
        nodes[2].attributes["foo"] = "bar"
        for n in nodes:
            n.compute_class()
        job = job_of()
        job.task_groups[0].constraints = [
            Constraint("${node.datacenter}", "dc1", "="), Constraint("${attr.kernel.name}", "linux", "is"),
            Constraint("${node.class}", "linux-medium-pci", "!="), Constraint("${attr.foo}", "", "is_set")]
        return table(kind, [(nodes[0], job, False), (nodes[1], job, False), (nodes[2], job, True)])
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_resolve_constraint_target(name):
    """feasible_test.go:827-900 TestResolveConstraintTarget, seen through constraints on
    mock.Node(): a target that resolves equals the node's value ("=" holds, "!="
    does not); one that does not resolve is not set, and "=" fails even against ""."""
    def scenario(kind):
        node = synth.mock_node("the-id")
        found = [("${node.unique.id}", node.id), ("${node.datacenter}", node.datacenter),
                 ("${node.unique.name}", node.name), ("${node.class}", node.node_class),
                 ("${attr.kernel.name}", node.attributes["kernel.name"]), ("${meta.pci-dss}", node.meta["pci-dss"])]
        rows = []
        for target, value in found:
            rows += [(node, job_of(constraints=[Constraint(target, value, "=")]), True),
                     (node, job_of(constraints=[Constraint(target, value, "!=")]), False),
                     (node, job_of(constraints=[Constraint(target, "", "is_set")]), True)]
        for target in ("${node.foo}", "${attr.rand}", "${meta.rand}"):
            rows += [(node, job_of(constraints=[Constraint(target, "", "is_set")]), False),
                     (node, job_of(constraints=[Constraint(target, "", "is_not_set")]), True),
                     (node, job_of(constraints=[Constraint(target, "", "=")]), False)]
        return table(kind, rows)
    both(kind_of(name), scenario)


@pytest.mark.parametrize("name", STACKS)
def test_task_group_distinct_hosts(name):
    """feasible_test.go:1356-1419 TestDistinctHostsIterator_TaskGroupDistinctHosts: a
    group-level distinct_hosts skips the node that holds an alloc of the same job
    and group, not the one whose alloc of that group name belongs to another job;
    a group without the constraint takes both nodes."""
    def scenario(kind):
        nodes = [synth.mock_node("n0"), synth.mock_node("n1")]
        allocs = [Allocation(node_id="n0", job_id="foo", task_group="example"),
                  Allocation(node_id="n1", job_id="bar", task_group="example")]
        task = lambda: [Task(name="t", driver="exec", cpu=100, memory_mb=64)]   # noqa: E731
        job = Job(id="foo", task_groups=[
            TaskGroup(name="example", count=2, ephemeral_disk_mb=10, tasks=task(),
                      constraints=[Constraint("", "", "distinct_hosts")]),
            TaskGroup(name="baz", count=2, ephemeral_disk_mb=10, tasks=task())])
        st = mk(kind.generic(), nodes, allocs, job)
        trace = [select_on(st, n, tg=0) for n in nodes]
        assert [r.row for r in trace] == [-1, 1] and trace[0].nodes_filtered == 1
        other = [select_on(st, n, tg=1) for n in nodes]
        assert [r.row for r in other] == [0, 1]
        return trace + other
    both(kind_of(name), scenario)


def _elig_case(kind, node, job, elig):
    st = mk(kind.generic(), [node], [], job)
    if elig:
        st.PutEligibility(elig)
    r = select_on(st, node)
    return st, r


@pytest.mark.parametrize("name", STACKS)
def test_feasibility_wrapper_uses_the_memo(name):
    """feasible_test.go:2226-2338 TestFeasibilityWrapper_*: the reference counts the
    calls of mocked checkers; here a checker that was not called shows as a verdict
    the node's own attributes would not give.
      JobIneligible: the class is marked ineligible and a fit node is dropped;
      JobAndTg_Eligible: job and group marked eligible, the failing group checker
        (a missing driver) is not run and the node comes out;
      JobEligible_TgIneligible: the group marked ineligible drops a fit node;
      JobEscapes / JobEligible_TgEscaped: with an escaping constraint the checkers
        run on the node itself and the class gets no verdict either way."""
    def scenario(kind):
        trace = []
        fit = synth.mock_node("fit")
        cc = fit.computed_class
        _, r = _elig_case(kind, fit, job_of(), {"job": {cc: False}})
        assert r.row == -1 and r.nodes_filtered == 1
        trace.append(r)
        nodrv = driver_node("nodrv")
        _, r = _elig_case(kind, nodrv, job_of(drivers=("exec", "foo")), None)
        assert r.row == -1 and r.nodes_filtered == 1                  # the checker alone says no
        trace.append(r)
        _, r = _elig_case(kind, nodrv, job_of(drivers=("exec", "foo")),
                          {"job": {nodrv.computed_class: True}, "tgs": {"web": {nodrv.computed_class: True}}})
        assert r.row == 0 and r.nodes_filtered == 0
        trace.append(r)
        _, r = _elig_case(kind, fit, job_of(), {"job": {cc: True}, "tgs": {"web": {cc: False}}})
        assert r.row == -1 and r.nodes_filtered == 1
        trace.append(r)
        # escaped job constraint that fails: the job's status for the class stays escaped
        esc = [Constraint("${node.unique.id}", "someone-else", "=")]
        st, r = _elig_case(kind, fit, job_of(constraints=esc), None)
        assert r.row == -1 and r.nodes_filtered == 1
        e = st.Eligibility()
        assert e["escaped"] and cc not in e["job"]
        trace.append(r)
        # escaped group constraint that passes: the node comes out, the group's status stays escaped
        job = job_of()
        job.task_groups[0].constraints = [Constraint("${node.unique.id}", "fit", "=")]
        st, r = _elig_case(kind, fit, job, {"job": {cc: True}})
        assert r.row == 0
        e = st.Eligibility()
        assert e["escaped"] and cc not in e["tgs"].get("web", {})
        trace.append(r)
        return trace
    both(kind_of(name), scenario)


@pytest.mark.parametrize("check", CONSTRAINT_CHECKERS)
def test_set_contains_any(check):
    """feasible_test.go:2340-2346 TestSetContainsAny."""
    for l, r, want in [("a", "a", True), ("a,b", "a", True), ("  a,b  ", "a ", True), ("b", "a", False)]:
        assert check("set_contains_any", l, r) == want, (l, r)


S = lambda s: (s, "")   # noqa: E731  NewStringAttribute

# feasible_test.go:2686-2817 TestCheckAttributeConstraint: (op, lVal, rVal, result); None = nil
CHECK_ATTRIBUTE = [
    ("=", S("foo"), "foo", True), ("=", None, None, False), ("is", S("foo"), "foo", True),
    ("==", S("foo"), "foo", True), ("!=", S("foo"), "foo", False), ("!=", None, "foo", True),
    ("!=", S("foo"), None, True), ("!=", S("foo"), "bar", True), ("not", S("foo"), "bar", True),
    ("version", S("1.2.3"), "~> 1.0", True), ("regexp", S("foobarbaz"), "[\\w]+", True),
    ("<", S("foo"), "bar", False), ("set_contains", S("foo,bar,baz"), "foo,  bar  ", True),
    ("set_contains_all", S("foo,bar,baz"), "foo,  bar  ", True), ("set_contains", S("foo,bar,baz"), "foo,bam", False),
    ("set_contains_any", S("foo,bar,baz"), "foo,bam", True), ("is_set", S("foo,bar,baz"), None, True),
    ("is_set", None, None, False), ("is_not_set", S("foo,bar,baz"), None, False), ("is_not_set", None, None, True),
]


@pytest.mark.parametrize("check", ATTR_CHECKERS)
def test_check_attribute_constraint(check):
    for op, l, r, want in CHECK_ATTRIBUTE:
        assert check(op, l, r) == want, (op, l, r)
    # checkSetContainsAny on attributes, TestSetContainsAny's rows
    for l, r, want in [("a", "a", True), ("a,b", "a", True), ("  a,b  ", "a ", True), ("b", "a", False)]:
        assert check("set_contains_any", S(l), r) == want, (l, r)
