"""pe_place_destructive: computePlacements' loop over its `destructive` list
(generic_sched.go:493-649) in one call. Per update AppendStoppedAlloc(prev)
(:543-547), Select (:552), AppendAlloc on an option (:627); on nil
PopUpdate(prev) (:639-645) and the loop ends (:521-525).

The yardstick is the oracle driven through place_destructive_by_select, the
per-call sequence. Records are compared with test_plan_stops' `_key`: equal, not
close. Every GPU scenario first shows, on the oracle alone, that it tests the
interleaving: its records differ from those of the same loop with no stops and
from those with every stop applied up front."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest

from nomad_amd import abi, synth
from nomad_amd.stack import place_destructive_by_select
from nomad_amd.structs import (Affinity, Allocation, Constraint, CSIVolumeRequest, NetworkResource, RequestedDevice,
                               SchedulerConfig, Spread, SpreadTarget, Task, TaskGroup)
from oracle.oracle import OracleGenericStack
from tests.test_plan_stops import _key

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nomad_pe.h")
LIB = os.path.join(ROOT, "nomad_amd", "libnomadpe.so")

ASK_CPU = 500          # job_c2's ask, and what an own alloc of the older version holds
LENGTHS = (1, 2, 63, 64, 65, 100, 127, 128, 129, 300)


# ---- scenarios --------------------------------------------------------------------

def _job_with_own_allocs(n, own, seed, tight=0.5, per_node=1):
    """A C2-shaped cluster where job 'svc-c2' (an older version) already holds
    `own` allocs, `per_node` on each of own / per_node random nodes (the same
    node may be drawn twice when own exceeds the nodes). A `tight` fraction of
    those nodes is filled by a foreign alloc so that the ask fits only after
    one of the node's own allocs has been stopped."""
    nodes, allocs = synth.cluster_c2(n, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    groups = max(1, own // per_node)
    picks = rng.choice(n, size=groups, replace=False) if groups <= n else rng.integers(0, n, size=groups)
    used = {}
    for a in allocs:
        used[a.node_id] = used.get(a.node_id, 0) + a.cpu_shares
    held = {}
    for k in picks:
        for _ in range(per_node):
            allocs.append(Allocation(node_id=nodes[int(k)].id, job_id="svc-c2", task_group="web",
                                     cpu_shares=ASK_CPU, memory_mb=256, disk_mb=150, priority=50))
            held[int(k)] = held.get(int(k), 0) + 1
    for k in sorted(held):
        nd = nodes[k]
        if rng.random() >= tight:
            continue
        spare = int(rng.integers(0, ASK_CPU))            # free cpu once the filler is in: less than the ask
        fill = nd.cpu_shares - nd.reserved_cpu - used.get(nd.id, 0) - ASK_CPU * held[k] - spare
        if fill > 0:
            allocs.append(Allocation(node_id=nd.id, job_id="filler", task_group="tg", cpu_shares=fill, memory_mb=16,
                                     disk_mb=10, priority=50))
    job = synth.job_c2(max(own, 1))
    job.version = 7
    own_idx = [i for i, a in enumerate(allocs) if a.job_id == "svc-c2"]
    return nodes, allocs, job, own_idx


class Scenario:
    def __init__(self, nodes, allocs, job, perm, upd, batch=False, prep=None):
        self.nodes, self.allocs, self.job, self.perm, self.upd = nodes, allocs, job, perm, [int(a) for a in upd]
        self.batch, self.prep = batch, prep

    def stack(self, cls, **kw):
        st = cls(batch=self.batch, **kw)
        st.SetState(self.nodes, self.allocs)
        st.SetJob(self.job)
        st.SetNodes(self.perm)
        if self.prep:
            self.prep(st)
        return st

    def oracle(self):
        return self.stack(OracleGenericStack)

    def engine(self, **kw):
        from nomad_amd.stack import GenericStack
        return self.stack(GenericStack, **kw)


def _length(n, batch):
    own = 64 if n >= 8 else 2 * n + 1
    nodes, allocs, job, own_idx = _job_with_own_allocs(n, own, seed=100 + n, tight=0.5 if n >= 8 else 1.0)
    return Scenario(nodes, allocs, job, synth.shuffle(n, n + 3), own_idx[:64], batch=batch)


def _ahead_of_cursor(sc, own_idx, updates, siblings=False):
    """The update list chosen update by update on the oracle: the next own
    alloc whose node lies a few positions past the cursor, so its stop lands
    inside the window the loop has already evaluated; with `siblings`, the
    node's other own allocs follow at once (their stops meet the placement the
    first one made room for)."""
    st = sc.oracle()
    n = len(sc.perm)
    pos_of = {int(r): p for p, r in enumerate(sc.perm)}
    at = {}
    for ai in own_idx:
        at.setdefault(pos_of[st.row(sc.allocs[ai].node_id)], []).append(ai)
    upd, used, queue = [], set(), []
    for k in range(updates):
        pick = None
        while queue and pick is None:
            ai = queue.pop(0)
            pick = ai if ai not in used else None
        if pick is None:
            off = st.GetCursor()[0]
            for d in range(1 + (k % 3) * 5, 48):
                free = [ai for ai in at.get((off + d) % n, ()) if ai not in used]
                if free:
                    pick = free[0]
                    if siblings:
                        queue = free[1:]
                    break
        if pick is None:
            break
        used.add(pick)
        upd.append(pick)
        st.StopAllocs([pick])
        r = st.SelectRaw(0)
        if r.row < 0:
            st.PopUpdate(pick)
            break
        st.Commit(0, r.row)
    sc.upd = upd
    return sc


def _cut(n, seed, per_node=1):
    """The updated allocs' nodes at positions just ahead of the cursor, every
    such node full until one of its own allocs is stopped."""
    nodes, allocs, job, own_idx = _job_with_own_allocs(n, (n // 2) * per_node, seed=seed, tight=1.0, per_node=per_node)
    sc = Scenario(nodes, allocs, job, synth.shuffle(n, seed + 2), [])
    return _ahead_of_cursor(sc, own_idx, 40, siblings=per_node > 1)


def _mixed():
    """Two own allocs per node (updates that share a node), a listed alloc that
    is terminal, and one that an earlier pe_plan_stop already stopped."""
    nodes, allocs, job, own_idx = _job_with_own_allocs(150, 48, seed=171, tight=0.7, per_node=2)
    upd = own_idx[:40]
    allocs[upd[5]].terminal = True
    stopped = upd[9]
    return Scenario(nodes, allocs, job, synth.shuffle(150, 172), upd, prep=lambda st: st.StopAllocs([stopped]))


NIL_AT = 6


def _nil():
    """Every node is full. Updates 0..NIL_AT-1 each free room for one placement;
    update NIL_AT's previous alloc is too small for its stop to make room."""
    n = 14
    nodes, _ = synth.cluster_c2(n, seed=181, other_allocs=False)
    allocs = []
    for k, nd in enumerate(nodes):
        cap = nd.cpu_shares - nd.reserved_cpu
        if k < 10:
            own_cpu = 100 if k == NIL_AT else ASK_CPU
            allocs.append(Allocation(node_id=nd.id, job_id="svc-c2", task_group="web", cpu_shares=own_cpu,
                                     memory_mb=256, disk_mb=150, priority=50))
            allocs.append(Allocation(node_id=nd.id, job_id="filler", task_group="tg", cpu_shares=cap - own_cpu - 7 * k,
                                     memory_mb=16, disk_mb=10, priority=50))
        else:
            allocs.append(Allocation(node_id=nd.id, job_id="filler", task_group="tg", cpu_shares=cap - 50 - k,
                                     memory_mb=16, disk_mb=10, priority=50))
    job = synth.job_c2(10)
    job.version = 7
    upd = [i for i, a in enumerate(allocs) if a.job_id == "svc-c2"]
    return Scenario(nodes, allocs, job, synth.shuffle(n, 182), upd)


def _devices():
    """A C5-style snapshot where every instance that matches the ask is taken:
    own allocs of the older version hold two instances each (one or two such
    allocs per node), background allocs the rest. A stop returns two instances
    to dev_free and makes its node the one option; a node's second stop meets
    the placement the first one made room for."""
    n = 120
    nodes, allocs = synth.cluster_c5(n, seed=191)
    row = {nd.id: k for k, nd in enumerate(nodes)}
    free = {k: nd.devices[0].healthy for k, nd in enumerate(nodes) if nd.devices}
    for a in allocs:
        for _, c in a.devices:
            free[row[a.node_id]] -= c
    rng = np.random.Generator(np.random.PCG64(192))
    for k in sorted(free):
        if nodes[k].devices[0].name == "1080ti":          # the ask's device constraint filters these
            continue
        own = 0 if free[k] < 2 else (2 if free[k] >= 4 and rng.random() < 0.5 else 1)
        for _ in range(own):
            allocs.append(Allocation(node_id=nodes[k].id, job_id="svc-c5", task_group="infer", cpu_shares=1000,
                                     memory_mb=2048, disk_mb=150, priority=80, devices=[(0, 2)]))
        if free[k] > 2 * own:
            allocs.append(Allocation(node_id=nodes[k].id, job_id="batch-x", task_group="train", cpu_shares=100,
                                     memory_mb=64, disk_mb=10, priority=20, devices=[(0, free[k] - 2 * own)]))
    upd = [i for i, a in enumerate(allocs) if a.job_id == "svc-c5"]
    job = synth.job_c5(len(upd))
    job.version = 7
    upd = [upd[int(k)] for k in rng.permutation(len(upd))][:48]
    return Scenario(nodes, allocs, job, synth.shuffle(n, 193), upd)


def _large():
    nodes, allocs, job, own_idx = _job_with_own_allocs(2500, 400, seed=62)
    return Scenario(nodes, allocs, job, synth.shuffle(2500, 8), own_idx[::2])


SCENARIOS = {"cut300": lambda: _cut(300, 151), "cut100": lambda: _cut(100, 161), "mixed": _mixed, "nil": _nil,
             "devices": _devices, "large": _large}
for _n in LENGTHS:
    SCENARIOS["len%d-svc" % _n] = functools.partial(_length, _n, False)
    SCENARIOS["len%d-batch" % _n] = functools.partial(_length, _n, True)


def _count_loop(st, k):
    out = []
    for _ in range(k):
        r = st.SelectRaw(0)
        out.append(_key(r))
        if r.row < 0:
            break
        st.Commit(0, r.row)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The scenario and the oracle's records: the interleaved loop (the
    yardstick), the same loop with no stops, and with all stops up front.
    Computed once and shared; nothing changes it afterwards."""
    sc = SCENARIOS[name]()
    inter = [_key(r) for r in place_destructive_by_select(sc.oracle(), 0, sc.upd)]
    none = _count_loop(sc.oracle(), len(sc.upd))
    st = sc.oracle()
    st.StopAllocs(sc.upd)
    front = _count_loop(st, len(sc.upd))
    return sc, inter, none, front


def _keys(records):
    return [_key(r) for r in records]


# ---- CPU, no device ---------------------------------------------------------------

def test_header_library_and_binding_declare_the_entry():
    from nomad_amd.stack import GenericStack
    assert "pe_place_destructive" in abi.ENGINE_SYMBOLS
    assert callable(getattr(GenericStack, "PlaceDestructive", None))
    with open(HEADER) as fh:
        text = fh.read()
    assert "int pe_place_destructive(pe_stack* s, uint32_t tg_index, const uint32_t* allocs, uint32_t n, " \
           "pe_ranked_node* out,\n                         uint32_t* placed);" in text
    assert hasattr(C.CDLL(LIB), "pe_place_destructive")


def test_oracle_stop_is_visible_to_its_own_select_only_and_a_failure_pops_it():
    # two nodes of 3900 usable cpu, each with a filler (3200) and a previous alloc (600): the ask (500)
    # fits a node once its previous alloc is stopped, and then only once. Update 2's previous alloc is a
    # small one (150) on node 0.
    nodes, _ = synth.cluster_c1(2, seed=3)
    prev = [Allocation(node_id=nd.id, job_id="other", task_group="tg", cpu_shares=600, memory_mb=64, disk_mb=10)
            for nd in nodes]
    small = Allocation(node_id=nodes[0].id, job_id="other", task_group="tg", cpu_shares=150, memory_mb=10, disk_mb=10)
    fill = [Allocation(node_id=nd.id, job_id="other", task_group="tg", cpu_shares=nd.cpu_shares - 100 - 600 - 250,
                       memory_mb=64, disk_mb=10) for nd in nodes]
    job = synth.mock_job(count=3)

    def stack():
        st = OracleGenericStack()
        st.SetState(nodes, prev + [small] + fill)
        st.SetJob(job)
        st.SetNodes([0, 1])
        return st

    def probe(st):
        # alloc 0's stop is popped if it is its node's last entry; then, with node 0's filler stopped,
        # the option's score tells which of the node's allocs are in the proposed state
        st.PopUpdate(0)
        st.StopAllocs([3])
        st.SetNodes([0])
        return _key(st.SelectRaw(0))

    st = stack()
    assert st.SelectRaw(0).row < 0                      # nothing fits while the previous allocs stand
    recs = place_destructive_by_select(st, 0, [0, 1, 2])
    # Select 0 saw stop 0 alone (node 1 still full), Select 1 saw stop 1; update 2's stop frees too little
    assert [r.row for r in recs] == [0, 1, -1]
    assert recs[0].nodes_exhausted == 1 and recs[2].nodes_exhausted == 2
    got = probe(st)
    # the same by hand, update 2's stop taken back (popped), and left standing
    popped, kept = stack(), stack()
    for o, pop in ((popped, True), (kept, False)):
        for ai in (0, 1):
            o.StopAllocs([ai])
            o.Commit(0, o.SelectRaw(0).row)
        o.StopAllocs([2])
        assert o.SelectRaw(0).row < 0
        if pop:
            o.PopUpdate(2)
    assert got == probe(popped) and got[0] == 0
    assert got != probe(kept)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario_tests_the_interleaving(name):
    sc, inter, none, front = reference(name)
    assert len(sc.upd) == len(set(sc.upd)) and len(sc.upd) >= 1
    assert inter != none, "the loop with no stops gives the same records"
    assert inter != front, "all stops up front give the same records"
    assert sum(1 for k in inter if k[0] >= 0) >= 1


def test_cut_scenarios_free_the_winner_and_an_exhausted_node():
    for name in ("cut300", "cut100"):
        sc, inter, _, _ = reference(name)
        st = sc.oracle()
        rows = [st.row(sc.allocs[ai].node_id) for ai in sc.upd]
        assert len(sc.upd) >= 20
        assert any(k[0] == row for k, row in zip(inter, rows)), "no Select won by the node just freed"
        found = False
        for ai, row in zip(sc.upd, rows):
            st.SetNodes([row])
            before = st.SelectRaw(0)
            st.StopAllocs([ai])
            after = st.SelectRaw(0)
            st.PopUpdate(ai)
            found = found or (before.row < 0 and before.nodes_exhausted == 1 and after.row == row)
        assert found, "no node that is exhausted before its stop and an option after it"


def test_mixed_scenario_holds_its_three_kinds():
    sc, inter, _, _ = reference("mixed")
    node = [sc.allocs[a].node_id for a in sc.upd]
    assert len(set(node)) < len(node)
    assert sum(1 for a in sc.upd if sc.allocs[a].terminal) == 1
    assert len(inter) == len(sc.upd)


@pytest.mark.parametrize("name", ["len1-svc", "len2-batch", "devices"])
def test_a_stop_meets_a_placement_of_the_same_call(name):
    # the row of a later stop already holds a placement of the loop: with a device ask the order of
    # that placement's offer and the stop's returned instances matters
    sc, inter, _, _ = reference(name)
    st = sc.oracle()
    rows = [st.row(sc.allocs[ai].node_id) for ai in sc.upd]
    assert any(rows[i] in {k[0] for k in inter[:i]} for i in range(1, len(inter)))


def test_nil_scenario_runs_out_at_its_update():
    sc, inter, _, _ = reference("nil")
    assert len(inter) == NIL_AT + 1 and inter[-1][0] == -1 and all(k[0] >= 0 for k in inter[:-1])


# ---- GPU --------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("batch", [False, True], ids=["svc", "batch"])
@pytest.mark.parametrize("n", LENGTHS)
def test_parity_over_list_lengths(n, batch):
    sc, inter, _, _ = reference("len%d-%s" % (n, "batch" if batch else "svc"))
    eng = sc.engine()
    assert eng.limit == (2 if batch else max(2, int(np.ceil(np.log2(n))) if n > 1 else 2))
    assert _keys(eng.PlaceDestructive(0, sc.upd, fallback=False)) == inter
    ora = sc.oracle()
    place_destructive_by_select(ora, 0, sc.upd)
    assert eng.GetCursor() == ora.GetCursor()


@gpu
@pytest.mark.parametrize("name", ["cut300", "cut100"])
def test_stops_inside_the_cached_window(name):
    sc, inter, _, _ = reference(name)
    eng = sc.engine()
    assert _keys(eng.PlaceDestructive(0, sc.upd, fallback=False)) == inter


@gpu
def test_one_upload_one_launch_one_synchronisation():
    # two calls over one list are the sequence too; the first call after SetNodes also carries the node list
    sc, inter, _, _ = reference("len300-svc")
    eng = sc.engine()
    first = _keys(eng.PlaceDestructive(0, sc.upd[:20], fallback=False))
    assert eng.place_destructive_stats() == (2, 1, 2)     # launches, synchronisations, uploads
    rest = _keys(eng.PlaceDestructive(0, sc.upd[20:], fallback=False))
    assert eng.place_destructive_stats() == (1, 1, 1)     # whatever n: 44 updates here
    assert first + rest == inter


@gpu
def test_stops_that_share_a_node_or_change_nothing():
    sc, inter, _, _ = reference("mixed")
    eng, ora = sc.engine(), sc.oracle()
    assert _keys(eng.PlaceDestructive(0, sc.upd, fallback=False)) == inter
    place_destructive_by_select(ora, 0, sc.upd)
    eng.SetNodes(sc.perm)
    ora.SetNodes(sc.perm)
    assert _keys(eng.Place(0, 12)) == _count_loop(ora, 12)   # build_job_counts from the mirrors


@gpu
def test_nil_pops_its_stop_and_ends_the_loop():
    sc, inter, _, _ = reference("nil")
    eng, ora = sc.engine(), sc.oracle()
    got = eng.PlaceDestructive(0, sc.upd, fallback=False)
    assert _keys(got) == inter and len(got) == NIL_AT + 1 and got[-1].row == -1
    place_destructive_by_select(ora, 0, sc.upd)
    assert eng.GetCursor() == ora.GetCursor() and eng.Eligibility() == ora.Eligibility()
    # allocs[k] is back in the proposed state: its node answers as the oracle's does, and is full
    row = eng.row(sc.allocs[sc.upd[NIL_AT]].node_id)
    for st in (eng, ora):
        st.SetNodes([row])
    r = eng.SelectRaw(0)
    assert _key(r) == _key(ora.SelectRaw(0)) and r.row < 0 and r.nodes_exhausted == 1
    for st in (eng, ora):
        st.SetNodes(sc.perm)
    rest = sc.upd[NIL_AT + 1:]
    assert _keys(eng.PlaceDestructive(0, rest, fallback=False)) == _keys(place_destructive_by_select(ora, 0, rest))
    assert _keys(eng.Place(0, 4)) == _count_loop(ora, 4)


@gpu
def test_device_asks_take_the_returned_instances():
    sc, inter, _, _ = reference("devices")
    eng, ora = sc.engine(), sc.oracle()
    got = eng.PlaceDestructive(0, sc.upd, fallback=False)
    assert _keys(got) == inter
    rows = [eng.row(sc.allocs[a].node_id) for a in sc.upd]
    assert any(r.row == row and r.device_offers for r, row in zip(got, rows))
    place_destructive_by_select(ora, 0, sc.upd)
    assert _keys(eng.Place(0, 10)) == _count_loop(ora, 10)


@gpu
def test_later_state_equals_the_per_call_sequence():
    sc, inter, _, _ = reference("len300-svc")
    a, b, ora = sc.engine(), sc.engine(), sc.oracle()
    assert _keys(a.PlaceDestructive(0, sc.upd, fallback=False)) == inter
    assert _keys(place_destructive_by_select(b, 0, sc.upd)) == inter
    place_destructive_by_select(ora, 0, sc.upd)
    assert a.GetCursor() == b.GetCursor() == ora.GetCursor()
    assert a.Eligibility() == b.Eligibility() == ora.Eligibility()
    last = sc.upd[-1]
    row = a.row(sc.allocs[last].node_id)
    got = []
    for st in (a, b, ora):
        st.PopUpdate(last)
        st.SetNodes([row])
        one = _key(st.SelectRaw(0))
        st.SetNodes(sc.perm)
        got.append([one] + _count_loop(st, 20))           # forces build_job_counts from the mirrors
    assert got[0] == got[1] == got[2]
    assert a.Eligibility() == b.Eligibility()


@gpu
def test_one_larger_run():
    sc, inter, _, _ = reference("large")
    eng = sc.engine()
    assert len(sc.upd) == 200
    assert _keys(eng.PlaceDestructive(0, sc.upd, fallback=False)) == inter


def _refusals():
    """name -> (match, job mutation, stack keywords, preparation, cluster mutation)"""
    def aff(job):
        job.task_groups[0].affinities = [Affinity("${node.class}", "class-1", "=", 50)]

    def spread(job):
        job.spreads = [Spread("${node.class}", 60, [SpreadTarget("class-1", 40)])]

    def distinct(job):
        job.task_groups[0].constraints = [Constraint("${node.class}", "100", "distinct_property")]

    def sibling(job):
        job.task_groups.append(TaskGroup(name="aff", count=1, affinities=[Affinity("${node.class}", "class-2", "=", 50)],
                                         tasks=[Task(name="aff", driver="exec", cpu=100, memory_mb=64)]))

    def cores(job):
        job.task_groups[0].tasks[0].cores = 1

    def static_group(job):
        job.task_groups[0].network = NetworkResource(mode="host", reserved_ports=[8080], port_labels=["http"])

    def static_task(job):
        job.task_groups[0].tasks[0].network = NetworkResource(mode="host", mbits=10, reserved_ports=[8080],
                                                              port_labels=["http"])

    def task_net(job):
        job.task_groups[0].tasks[0].network = NetworkResource(mode="host", mbits=10, dynamic_ports=1)

    def same_name(job):
        job.task_groups.append(copy.deepcopy(job.task_groups[0]))

    def too_many_devices(job):
        job.task_groups[0].tasks[0].devices = [RequestedDevice("nvidia/gpu", 300)]

    def alloc_cores(nodes, allocs, upd):
        nd = next(x for x in nodes if x.id == allocs[upd[0]].node_id)
        nd.total_cores = 4
        nd.reservable_cores = [0, 1, 2, 3]
        allocs[upd[0]].reserved_cores = [1]

    def two_nics(nodes, allocs, upd):
        nodes[0].networks = [NetworkResource(mode="host", device="eth0", cidr="10.0.0.1/32", ip="10.0.0.1", mbits=1000),
                             NetworkResource(mode="host", device="eth1", cidr="10.128.0.1/32", ip="10.128.0.1",
                                             mbits=1000)]
        nodes[0].compute_class()

    return {
        "node affinities": ("full passes", aff, {}, None, None),
        "spreads": ("full passes", spread, {}, None, None),
        "distinct_property": ("distinct_property", distinct, {}, None, None),
        "a latched limit": ("latched", sibling, {}, lambda st: st.SelectRaw(1), None),
        "metrics on": ("pe_set_metrics on", None, {}, lambda st: st.EnableMetrics(True), None),
        "a preempting stack": ("preempting stack", None, {"config": SchedulerConfig(preempt_service=True)}, None, None),
        "several devices": ("several devices", None, {"devices": [0, 0]}, None, None),
        "a reserved-cores ask": ("cores", cores, {}, None, None),
        "an alloc with reserved cores": ("holds reserved cores", None, {}, None, alloc_cores),
        "static ports in the group network": ("static port", static_group, {}, None, None),
        "static ports in a task network": ("static port", static_task, {}, None, None),
        "a task network with multi-device nodes": ("multi-device", task_net, {}, None, two_nics),
        "two groups of one name": ("one name", same_name, {}, None, None),
        "the group's own reason": ("device request count above 255", too_many_devices, {}, None, None),
    }


def _refusal_scenario(case):
    match, mutate, kw, prep, cluster = _refusals()[case]
    nodes, allocs, job, own_idx = _job_with_own_allocs(120, 24, seed=201)
    upd = own_idx[:16]
    if mutate:
        mutate(job)
    if cluster:
        cluster(nodes, allocs, upd)
    return match, kw, Scenario(nodes, allocs, job, synth.shuffle(120, 202), upd, prep=prep)


@gpu
@pytest.mark.parametrize("case", sorted(_refusals()))
def test_refusals_leave_the_handle_as_it_was(case):
    from nomad_amd.stack import Unsupported
    match, kw, sc = _refusal_scenario(case)
    eng, fresh = sc.engine(**kw), sc.engine(**kw)
    cursor, elig = eng.GetCursor(), eng.Eligibility()
    with pytest.raises(Unsupported, match=match):
        eng.PlaceDestructive(0, sc.upd, fallback=False)
    assert eng.GetCursor() == cursor and eng.Eligibility() == elig
    try:
        want = _keys(place_destructive_by_select(fresh, 0, sc.upd))
    except Unsupported:
        # the engine's own Select refuses this job too: the refused handle's answer as well
        with pytest.raises(Unsupported):
            place_destructive_by_select(eng, 0, sc.upd)
        return
    # cursor, plan and NodeUpdate untouched: the fallback's sequence answers as a fresh handle's does
    assert _keys(eng.PlaceDestructive(0, sc.upd)) == want
    assert eng.GetCursor() == fresh.GetCursor() and eng.Eligibility() == fresh.Eligibility()
    fresh.SetNodes(sc.perm)
    eng.SetNodes(sc.perm)
    assert _count_loop(eng, 5) == _count_loop(fresh, 5)


@gpu
def test_refusal_of_a_csi_group():
    from nomad_amd.stack import Unsupported
    from tests.test_csi import csi_job, engine_with, kat
    nodes, volumes, node_volumes = kat()
    allocs = [Allocation(node_id=nodes[0].id, job_id="csi-job", task_group="web", cpu_shares=100, memory_mb=64)]
    eng = engine_with(nodes, volumes, node_volumes, csi_job([CSIVolumeRequest("volume-id")], count=2), allocs=allocs)
    cursor = eng.GetCursor()
    with pytest.raises(Unsupported, match="CSI requests"):
        eng.PlaceDestructive(0, [0], fallback=False)
    assert eng.GetCursor() == cursor


@gpu
def test_refusal_beyond_the_overlay_of_one_launch():
    from nomad_amd.stack import GenericStack, Unsupported
    nodes, allocs = synth.cluster_c2(3000, seed=61)
    assert len(allocs) > 2049
    eng = GenericStack()
    eng.SetState(nodes, allocs)
    eng.SetJob(synth.job_c2(10))
    eng.SetNodes(synth.shuffle(3000, 7))
    cursor = eng.GetCursor()
    lst = np.arange(2049, dtype=np.uint32)
    out, placed = (abi.pe_ranked_node * 1)(), C.c_uint32(0)    # refused before anything is written
    with pytest.raises(Unsupported, match="overlay of one launch"):
        eng._check(eng._lib.pe_place_destructive(eng._h, 0, lst.ctypes.data_as(abi.u32p), len(lst), out,
                                                 C.byref(placed)))
    assert eng.GetCursor() == cursor and placed.value == 0


@gpu
def test_invalid_arguments_change_nothing():
    from nomad_amd.stack import EngineError
    sc, inter, _, _ = reference("len100-svc")
    eng = sc.engine()
    cursor, elig = eng.GetCursor(), eng.Eligibility()
    for tg, lst in ((1, sc.upd[:4]), (0, sc.upd[:3] + [len(sc.allocs)]), (0, sc.upd[:3] + [sc.upd[1]])):
        with pytest.raises(EngineError) as err:
            eng.PlaceDestructive(tg, lst, fallback=False)
        assert err.value.code == abi.PE_EINVAL
        assert eng.GetCursor() == cursor and eng.Eligibility() == elig
    assert eng.PlaceDestructive(0, [], fallback=False) == []
    assert _keys(eng.PlaceDestructive(0, sc.upd, fallback=False)) == inter     # nothing had changed


@gpu
def test_state_errors():
    from nomad_amd.stack import EngineError, GenericStack, SystemStack
    sc, _, _, _ = reference("len100-svc")
    lst = np.asarray(sc.upd[:2], dtype=np.uint32)
    out, placed = (abi.pe_ranked_node * 2)(), C.c_uint32(0)

    def call(st):
        with pytest.raises(EngineError) as err:
            st._check(st._lib.pe_place_destructive(st._h, 0, lst.ctypes.data_as(abi.u32p), 2, out, C.byref(placed)))
        return err.value.code

    system = SystemStack()
    system.SetState(sc.nodes, sc.allocs)
    system.SetJob(synth.mock_system_job())
    system.SetNodes(sc.perm)
    assert call(system) == abi.PE_ESTATE
    no_job = GenericStack()
    no_job.SetState(sc.nodes, sc.allocs)
    assert call(no_job) == abi.PE_ESTATE
    no_list = GenericStack()
    no_list.SetState(sc.nodes, sc.allocs)
    no_list.SetJob(sc.job)
    assert call(no_list) == abi.PE_ESTATE
