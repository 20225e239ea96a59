"""In-place updates of task groups with CSI volumes in one call
(pe_inplace_update_csi).

The oracle has no CSI, so parity rests on two independent references, both
built here from what the tree has:

  A. `by_select`: the per-alloc sequence (pe_plan_stop, pe_set_nodes([row]),
     pe_csi_alloc_index, pe_select, pe_plan_pop_update and, on an option,
     pe_plan_stop + pe_commit) on a second engine handle with metrics off.
     Engine against engine everything is bit-equal.
  B. `model`: the oracle stack on the job without its CSI requests, driven
     through the same sequence, with the Python `csi_code` of tests/test_csi.py
     laid over it. CSIVolumeChecker runs behind the wrapper's job and group
     checks (feasible.go:1141-1149), so an update reaches it when the oracle's
     Select did not fail in the wrapper: it returned an option, an exhausted
     node, or a node DistinctHostsIterator filtered. Such an update with a
     code other than 0 is status 1 with a nil record, is not committed to the
     oracle's plan, and with metrics on records {ClassFiltered[NodeClass]: 1,
     ConstraintFiltered[pe_csi_reason_text]: 1}. Every other update is the
     oracle's answer. B is the only reference with metrics on. On the generic
     stack the scores are compared bit for bit; on the system stacks within
     the 1e-12 relative the other in-place tests use against the oracle there.

`test_model_by_hand` pins B itself on a 4-node cluster without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from nomad_amd import abi, synth
from nomad_amd.structs import (Allocation, CSINodePlugin, CSIVolume, CSIVolumeRequest, Constraint, DriverInfo, SchedulerConfig,
                               Spread, SpreadTarget, Task, TaskGroup)
from oracle.oracle import OracleGenericStack, OracleSystemStack
from tests.test_csi import NS, csi_code, plain
from tests.test_inplace_update import _key, _keys, _loop, _multi_own
from tests.test_inplace_update_metrics import _distinct_hosts, _same_metrics_oracle
from tests.test_inplace_update_preempt import _hand as _preempt_hand, _same_oracle, _seeded

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nomad_amd", "libnomadpe.so")
PRE = SchedulerConfig(preempt_system=True)
MAPS = ("ClassFiltered", "ConstraintFiltered", "ClassExhausted", "DimensionExhausted")
NODE_REASONS = (abi.PE_CSI_NO_PLUGIN, abi.PE_CSI_UNHEALTHY, abi.PE_CSI_MAX_VOLUMES)
REQS = [CSIVolumeRequest("va"), CSIVolumeRequest("vb", per_alloc=True),
        CSIVolumeRequest("vc", read_only=True, per_alloc=True)]
REGEXP = Constraint("${node.class}", "^class-[3-7]$", "regexp")
TARGET = Spread("${node.class}", 60, [SpreadTarget("class-0", 30), SpreadTarget("class-1", 20)])
EVEN = Spread("${node.class}", 50, [])
FULL = {"p0": CSINodePlugin(True), "p1": CSINodePlugin(True), "p2": CSINodePlugin(True)}


# ---- shapes ---------------------------------------------------------------------------------

def volumes_for(job_id):
    """tests/test_csi.py's random_cluster volumes for `job_id`: request 0 (va)
    passes at the volume level because its write claims are all the job's own;
    request 1 (vb, per_alloc): index 0 and 5 pass, 1 has no write claims, 2 and
    4 are held by another job / a lost alloc, 3 exists in another namespace
    only; request 2 (vc, read only, per_alloc) has no read claims at index 0.
    At index 5 every request passes at the volume level."""
    return [
        CSIVolume("va", NS, "p0", write_free_claims=False, write_allocs=[(NS, job_id), (NS, job_id)]),
        CSIVolume("vb[0]", NS, "p1"),
        CSIVolume("vb[1]", NS, "p1", write_schedulable=False),
        CSIVolume("vb[2]", NS, "p1", write_free_claims=False, write_allocs=[(NS, job_id), ("other", job_id)]),
        CSIVolume("vb[4]", NS, "p1", write_free_claims=False, write_allocs=[None]),
        CSIVolume("vb[5]", NS, "p1"),
        CSIVolume("vc[0]", NS, "p2", read_schedulable=False),
        CSIVolume("vc[5]", NS, "p2", write_schedulable=False),
        CSIVolume("vb[3]", "other", "p0"),
        CSIVolume("filler-0", NS, "p0"), CSIVolume("filler-1", NS, "p1"), CSIVolume("filler-2", NS, "p2"),
    ]


class Shape:
    """A cluster, a job whose group 0 carries REQS, the update list and each
    update's alloc index."""

    def __init__(self, nodes, allocs, job, upd, seed, p_full=0.8, idx=None, reqs=REQS, volumes=None):
        rng = np.random.Generator(np.random.PCG64(seed))
        self.nodes, self.allocs, self.job, self.upd = nodes, allocs, job, list(upd)
        job.task_groups[0].csi_volumes = list(reqs)
        if all(g.name != "plain" for g in job.task_groups):   # a group without CSI for the later state
            job.task_groups.append(TaskGroup(name="plain", count=1, tasks=[Task(name="plain", cpu=300, memory_mb=128)]))
        self.reqs = list(reqs)
        self.volumes = volumes_for(job.id) if volumes is None else volumes
        in_use = ["filler-0", "filler-1", "filler-2", "va", "vb[0]"]
        self.node_volumes = {}
        for nd in nodes:
            if nd.csi_node_plugins:
                continue                                      # (a hand-made node)
            if rng.random() < p_full:
                nd.csi_node_plugins = dict(FULL)
            else:
                for p in rng.permutation(3)[:int(rng.integers(0, 4))]:
                    nd.csi_node_plugins["p%d" % p] = CSINodePlugin(bool(rng.random() < 0.7),
                                                                   [1, 2, (1 << 63) - 1][int(rng.integers(0, 3))])
                m = int(rng.integers(0, 5))
                if m:
                    self.node_volumes[nd.id] = [in_use[int(i)] for i in rng.integers(0, len(in_use), m)]
        if idx is None:
            idx = [int(rng.choice([5, 5, 5, 5, 5, 5, 5, 0, 1, 2, 3, 4])) for _ in self.upd]
        self.idx = list(idx)
        self.by_id = {nd.id: nd for nd in nodes}

    def code(self, i):
        nd = self.by_id[self.allocs[self.upd[i]].node_id]
        return csi_code(nd, self.reqs, "[%d]" % self.idx[i], self.volumes, self.node_volumes, NS, self.job.id)

    def engine(self, system=False, config=None, metrics=False, csi=True):
        from nomad_amd.stack import GenericStack, SystemStack
        e = (SystemStack if system else GenericStack)(config=config)
        e.SetState(self.nodes, self.allocs)
        if csi:
            e.SetCSI(self.volumes, self.node_volumes)
        e.SetJob(self.job)
        if metrics:
            e.EnableMetrics(True)
        return e

    def oracle(self, system=False, config=None):
        o = (OracleSystemStack if system else OracleGenericStack)(config=config)
        o.SetState(self.nodes, self.allocs)
        o.SetJob(plain(self.job))
        o.EnableMetrics(True)      # the maps tell a wrapper failure from distinct_hosts; they change no record
        return o


def generic_shape(n=64, own=200, seed=71, constraint=None, spreads=None, **kw):
    nodes, allocs, job, upd = _multi_own(n, own, seed=seed)
    if constraint is not None:
        job.constraints.append(constraint)
    if spreads:
        job.task_groups[0].spreads = list(spreads)
    return Shape(nodes, allocs, job, upd, seed + 1000, **kw)


def reasons_shape():
    """A job constraint that fails whole classes, and half of the nodes with a random plugin set."""
    return generic_shape(constraint=REGEXP, p_full=0.5)


def system_shape(n=64, seed=95, **kw):
    nodes, allocs, job, upd = _seeded(n, seed)
    return Shape(nodes, allocs, job, upd, seed + 1000, **kw)


# ---- reference A: the per-alloc sequence ------------------------------------------------------

def by_select(st, tg, upd, idx=None):
    """inplace_update_by_select plus pe_csi_alloc_index before each Select."""
    node_row = st.state.alloc_table.node_row
    records, status = [], []
    for i, ai in enumerate(upd):
        row = int(node_row[ai])
        st.StopAllocs([ai])
        st.SetNodes(np.asarray([row], dtype=np.uint32))
        if idx is not None:
            st.CSIAllocIndex(tg, idx[i])
        r = st.SelectRaw(tg)
        st.PopUpdate(ai)
        if r.row >= 0:
            st.StopAllocs([ai])
            st.Commit(tg, r.row)
            records.append(r)
            status.append(0)
        else:
            records.append(None)
            status.append(1 if r.nodes_filtered else 2)
    return records, status


# ---- reference B: the model ---------------------------------------------------------------------

_LIBS = {}


def reason_text(reason, plugin, volume, node_id):
    """pe_csi_reason_text (stateless, no device)."""
    if "lib" not in _LIBS:
        _LIBS["lib"] = abi.bind_csi_reason_text(C.CDLL(LIB))
    lib = _LIBS["lib"]
    need = lib.pe_csi_reason_text(reason, plugin.encode(), volume.encode(), node_id.encode(), None, 0)
    assert need > 0
    buf = C.create_string_buffer(need)
    assert lib.pe_csi_reason_text(reason, plugin.encode(), volume.encode(), node_id.encode(), buf, need) == need
    return buf.value.decode()


def csi_maps(shape, i, code):
    """What CSIVolumeChecker.Feasible records (feasible.go:251-259) for update i failing with `code`."""
    nd = shape.by_id[shape.allocs[shape.upd[i]].node_id]
    q, reason = code >> 3, code & 7
    r = shape.reqs[q]
    vol = r.source + ("[%d]" % shape.idx[i] if r.per_alloc else "")
    plugin = ""
    if reason in NODE_REASONS:
        plugin = next(v.plugin_id for v in shape.volumes if (v.namespace, v.id) == (NS, vol))
    text = reason_text(reason, plugin, vol, nd.id if reason in NODE_REASONS else "")
    m = {k: {} for k in MAPS}
    if nd.node_class:
        m["ClassFiltered"][nd.node_class] = 1
    m["ConstraintFiltered"][text] = 1
    m["ScoreMetaData"] = []
    return m


def model(shape, o, tg=0, csi=True):
    """(records, status, maps, reached): `reached[i]` the update got past the wrapper.
    `csi` False: the oracle's answer alone, every node available."""
    node_row = o.state.alloc_table.node_row
    records, status, maps, reached = [], [], [], []
    for i, ai in enumerate(shape.upd):
        o.StopAllocs([ai])
        o.SetNodes(np.asarray([int(node_row[ai])], dtype=np.uint32))
        r = o.SelectRaw(tg)
        m = o.LastMetrics()
        o.PopUpdate(ai)
        past = r.row >= 0 or not r.nodes_filtered or m["ConstraintFiltered"] == {"distinct_hosts": 1}
        code = shape.code(i) if past and csi else 0
        reached.append(past)
        if code:
            records.append(None)
            status.append(1)
            maps.append(csi_maps(shape, i, code))
            continue
        maps.append(m)
        if r.row >= 0:
            o.StopAllocs([ai])
            o.Commit(tg, r.row)
            records.append(r)
            status.append(0)
        else:
            records.append(None)
            status.append(1 if r.nodes_filtered else 2)
    return records, status, maps, reached


# ---- comparisons ----------------------------------------------------------------------------------

def same_as_model(got, want, exact):
    a, b = _keys(got[:2]), _keys(want[:2])
    assert a[1] == b[1]
    if exact:
        assert a[0] == b[0]
    else:
        _same_oracle(a, b)
    if got[2] is not None:
        _same_metrics_oracle(got[2], want[2])


def same_after(shape, stacks, seed, system=False, count=12):
    """Later observable state: the eligibility memo everywhere; placements of
    the group without CSI, engine against engine bit for bit and the rows
    against the oracle."""
    n = len(shape.nodes)
    perm = synth.shuffle(n, seed)
    elig = [st.Eligibility() for st in stacks]
    assert all(e == elig[0] for e in elig[1:]), elig
    runs = []
    for st in stacks:
        st.SetNodes(perm)
        runs.append(_loop(st, 1 if system else count, tg=1))
    engines = [r for st, r in zip(stacks, runs) if not type(st).__name__.startswith("Oracle")]
    assert all(r == engines[0] for r in engines[1:])
    if not system:
        assert all(r == runs[0] for r in runs[1:])
    else:
        assert all([k and k[0] for k in r] == [k and k[0] for k in runs[0]] for r in runs[1:])


def run_all(shape, system=False, config=None, metrics=False, seed=12):
    """The call (metrics on or off), reference A on a second handle (metrics
    off) and reference B; returns (engine, the call's answer, the model's)."""
    e = shape.engine(system, config, metrics=metrics)
    got = e.InplaceUpdateCSI(0, shape.upd, shape.idx, fallback=False)
    assert (got[2] is not None) == metrics
    o = shape.oracle(system, config)
    want = model(shape, o)
    same_as_model(got, want, exact=not system)
    e2 = shape.engine(system, config)
    a = by_select(e2, 0, shape.upd, shape.idx)
    assert _keys(got[:2]) == _keys(a)                  # engine against engine: bit for bit
    if system and config is not None:                  # the preempted sets, position by position
        full = e.InplaceUpdatePreempted()
        for i, r in enumerate(a[0]):
            assert full.get(i, []) == (list(r.preempted) if r is not None else []), i
    same_after(shape, (e, o, e2), seed, system=system)
    return e, got, want


def facts(shape, want):
    """What an answer exercises."""
    records, status, maps, reached = want
    unavailable = [i for i in range(len(status)) if reached[i] and shape.code(i)]
    return dict(status=[status.count(c) for c in (0, 1, 2)], unavailable=len(unavailable),
                reasons={shape.code(i) & 7 for i in unavailable},
                wrapper_and_unavailable=sum(1 for i in range(len(status)) if not reached[i] and shape.code(i)),
                keys={next(iter(maps[i]["ConstraintFiltered"])) for i in unavailable})


# ---- CPU: the model by hand -----------------------------------------------------------------------

def hand_shape():
    """Four mock nodes (3900 usable cpu), the job asks 2000 cpu and vol (per_alloc) on plugin foo:
     node 0  runs foo; own allocs 0 and 1 (500 cpu each). Update 0 has index 3 (vol[3] is
             missing), update 1 index 0: unavailable, then updated;
     node 1  runs no plugin; own alloc 2, index 0: "CSI plugin foo is missing from client";
     node 2  runs foo; a foreign alloc holds 3000 cpu: own alloc 3 with index 3 is unavailable
             (status 1, not 2), own alloc 4 with index 0 is exhausted on cpu;
     node 3  a windows node (the job's kernel.name constraint fails) without a plugin; own
             alloc 5: the constraint's reason, not the CSI one."""
    nodes, _ = synth.cluster_c1(4, seed=4)
    nodes[0].csi_node_plugins = {"foo": CSINodePlugin(True)}
    nodes[2].csi_node_plugins = {"foo": CSINodePlugin(True)}
    nodes[1].csi_node_plugins = {"bar": CSINodePlugin(True)}
    nodes[3].csi_node_plugins = {"bar": CSINodePlugin(True)}
    nodes[3].attributes["kernel.name"] = "windows"
    nodes[3].compute_class()
    own = dict(job_id="mock-service-0", task_group="web", cpu_shares=500, memory_mb=256, disk_mb=150)
    allocs = [Allocation(node_id=nodes[k].id, **own) for k in (0, 0, 1, 2, 2, 3)]
    allocs.append(Allocation(node_id=nodes[2].id, job_id="other", task_group="tg", cpu_shares=3000, memory_mb=64,
                             disk_mb=10))
    job = synth.mock_job(count=6)
    job.task_groups[0].tasks[0].cpu = 2000
    reqs = [CSIVolumeRequest("vol", per_alloc=True)]
    return Shape(nodes, allocs, job, [0, 1, 2, 3, 4, 5], 1, idx=[3, 0, 0, 3, 0, 3], reqs=reqs,
                 volumes=[CSIVolume("vol[0]", NS, "foo")])


def test_model_by_hand():
    s = hand_shape()
    records, status, maps, reached = model(s, s.oracle())
    assert status == [1, 0, 1, 1, 2, 1]
    assert reached == [True, True, True, True, True, False]
    assert [r is not None for r in records] == [False, True, False, False, False, False]
    assert records[1].row == 0 and records[1].nodes_evaluated == 1
    cls = s.nodes[0].node_class
    missing = {"ClassFiltered": {cls: 1}, "ConstraintFiltered": {"missing CSI Volume vol[3]": 1}}
    for i, want in ((0, missing), (3, missing),
                    (2, {"ClassFiltered": {cls: 1},
                         "ConstraintFiltered": {"CSI plugin foo is missing from client " + s.nodes[1].id: 1}}),
                    (5, {"ClassFiltered": {cls: 1}, "ConstraintFiltered": {"${attr.kernel.name} = linux": 1}})):
        assert {k: maps[i][k] for k in MAPS} == dict({k: {} for k in MAPS}, **want), i
        assert maps[i]["ScoreMetaData"] == []
    assert maps[4]["DimensionExhausted"] == {"cpu": 1} and maps[4]["ConstraintFiltered"] == {}
    assert len(maps[1]["ScoreMetaData"]) == 1 and maps[1]["ScoreMetaData"][0][0] == s.nodes[0].id
    # the unavailable updates were not committed: node 0 holds alloc 0's 500 and the updated 2000
    o = s.oracle()
    model(s, o)
    o.SetNodes([0])
    assert o.Select(1) is not None                      # 2500 + the plain group's 300 <= 3900
    f = facts(s, (records, status, maps, reached))
    assert f["unavailable"] == 3 and f["wrapper_and_unavailable"] == 1


def test_shapes_reach_what_the_gpu_tests_rely_on():
    """By the model alone: the seeded shapes hold every reason 1 to 7, two keys
    per plugin reason, nodes that fail a constraint and are unavailable, and
    nodes distinct_hosts would filter that are unavailable."""
    s = reasons_shape()
    f = facts(s, model(s, s.oracle()))
    assert f["reasons"] == {1, 2, 3, 4, 5, 6, 7}, f
    for word in ("is missing from client", "is unhealthy on client", "has the maximum number of volumes"):
        assert len({k for k in f["keys"] if word in k}) >= 2, (word, f["keys"])
    assert f["wrapper_and_unavailable"] >= 5 and min(f["status"]) >= 1, f
    for escaped in (False, True):
        s, first = memo_shape(escaped)
        o = s.oracle()
        want = model(s, o)
        assert memo_facts(s, first, o, want) >= 3
        if escaped:      # the per-node check fails two later listed nodes, with its own reason
            texts = [next(iter(m["ConstraintFiltered"]), "") for m in want[2]]
            assert sum(1 for t in texts if "node.unique.id" in t) >= 2
    s = distinct_shape()
    want = model(s, s.oracle())
    plain_run = model(s, s.oracle(), csi=False)
    both = [i for i in range(len(s.upd)) if s.code(i) and
            plain_run[2][i]["ConstraintFiltered"] == {"distinct_hosts": 1}]
    assert len(both) >= 2 and all(want[1][i] == 1 and "CSI" in next(iter(want[2][i]["ConstraintFiltered"]))
                                  for i in both)


def distinct_shape():
    nodes, allocs, job, upd = _distinct_hosts()
    for nd in nodes[:20]:
        nd.csi_node_plugins = dict(FULL)
    for nd in nodes[3:8] + nodes[12:16]:
        nd.csi_node_plugins = {"p0": CSINodePlugin(True), "p1": CSINodePlugin(False), "p2": CSINodePlugin(True)}
    return Shape(nodes, allocs, job, upd, 5, idx=[5] * len(upd))


# ---- GPU: parity ------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("metrics", [False, True])
def test_generic_every_reason_and_constraints(metrics):
    s = reasons_shape()
    e, got, want = run_all(s, metrics=metrics)
    assert 0 in got[1] and 1 in got[1] and 2 in got[1]
    if metrics:     # the texts of all seven reasons, compared with pe_csi_reason_text through the model
        f = facts(s, want)
        assert f["reasons"] == {1, 2, 3, 4, 5, 6, 7}
        got_keys = {next(iter(m["ConstraintFiltered"])) for m in got[2] if m["ConstraintFiltered"]}
        assert f["keys"] <= got_keys


@gpu
@pytest.mark.parametrize("metrics", [False, True])
def test_distinct_hosts_and_unavailable_reports_csi(metrics):
    s = distinct_shape()
    run_all(s, metrics=metrics, seed=14)


@gpu
@pytest.mark.parametrize("config", [None, PRE], ids=["system", "preempting"])
@pytest.mark.parametrize("metrics", [False, True])
def test_system_stacks(config, metrics):
    s = system_shape()
    e, got, want = run_all(s, system=True, config=config, metrics=metrics)
    f = facts(s, want)
    assert f["unavailable"] >= 10 and f["status"][0] >= 10
    if config is not None:
        assert any(r is not None and r.preempted for r in got[0])


@gpu
@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_the_code_is_per_update_not_per_node(order):
    s = hand_shape()
    s.upd = [s.upd[k] for k in order] + s.upd[2:]
    s.idx = [s.idx[k] for k in order] + s.idx[2:]
    e, got, want = run_all(s, metrics=True)
    assert got[1][:2] == ([1, 0] if order == (0, 1) else [0, 1])
    assert got[1][2:] == [1, 1, 2, 1]


@gpu
@pytest.mark.parametrize("metrics", [False, True])
def test_unavailable_on_an_exhausted_node_then_an_evicting_update(metrics):
    """tests/test_inplace_update_preempt.py's hand cluster: evict_a holds the own
    allocs 3 and 7, and each of their updates evicts. Update 3 is unavailable
    (vb[3] is missing): status 1, no eviction, no entry among the preempted
    sets; the later update 7 on that node still evicts."""
    nodes, allocs, job, upd = _preempt_hand()
    for nd in nodes:
        nd.csi_node_plugins = dict(FULL)
    s = Shape(nodes, allocs, job, upd, 3, idx=[3, 5, 5, 5, 5])
    plain_run = model(s, s.oracle(True, PRE), csi=False)
    assert plain_run[1][0] == 0 and plain_run[0][0].preempted       # its plain fit is exhausted: it would evict
    e, got, want = run_all(s, system=True, config=PRE, metrics=metrics)
    assert got[1][0] == 1 and got[1][4] == 0 and got[0][4].preempted
    full = e.InplaceUpdatePreempted()
    assert 0 not in full and 4 in full
    assert sorted(full[4]) == sorted(want[0][4].preempted)


def memo_shape(escaped):
    """The first listed node of every class is unavailable (it runs no plugin);
    with `escaped` the group also has a per-node check that two later listed
    nodes fail."""
    nodes, allocs, job, upd = _multi_own(64, 120, seed=75)
    first = {}
    for i in upd:
        nd = next(x for x in nodes if x.id == allocs[i].node_id)
        first.setdefault(nd.computed_class, nd)
    for nd in nodes:
        nd.csi_node_plugins = dict(FULL)
    for nd in first.values():
        nd.csi_node_plugins = {"p1": CSINodePlugin(True)}
    if escaped:
        later = [allocs[i].node_id for i in upd[40:] if allocs[i].node_id not in {x.id for x in first.values()}]
        job.task_groups[0].constraints = [Constraint("${node.unique.id}", later[0], "!="),
                                          Constraint("${node.unique.id}", later[5], "!=")]
    return Shape(nodes, allocs, job, upd, 9, idx=[5] * len(upd)), first


def memo_facts(s, first, o, want):
    """The first listed update of each class the wrapper lets through is
    unavailable, and the class is eligible afterwards."""
    classes = o.GetClasses(o.Eligibility())
    seen, n = set(), 0
    for i, ai in enumerate(s.upd):
        c = s.by_id[s.allocs[ai].node_id].computed_class
        if c in seen:
            continue
        seen.add(c)
        if want[3][i]:
            assert want[1][i] == 1 and s.code(i) and classes[c] is True, (i, c)
            n += 1
    return n


@gpu
@pytest.mark.parametrize("escaped", [False, True])
@pytest.mark.parametrize("metrics", [False, True])
def test_unavailable_node_of_an_unknown_class_memoises_it_eligible(escaped, metrics):
    """same_after compares pe_get_eligibility with the oracle's, whose facts
    test_shapes_reach_what_the_gpu_tests_rely_on pins."""
    s, first = memo_shape(escaped)
    run_all(s, metrics=metrics, seed=16)


@gpu
@pytest.mark.parametrize("spread", [TARGET, EVEN], ids=["target", "even"])
def test_spreads_with_unavailable_updates_in_the_list(spread):
    s = generic_shape(seed=79, spreads=[spread])
    per_node = {}
    for i in s.upd:
        per_node[s.allocs[i].node_id] = per_node.get(s.allocs[i].node_id, 0) + 1
    assert max(per_node.values()) >= 5
    e, got, want = run_all(s, metrics=False)                 # score parts and FinalScore: bit for bit (A and B)
    mid = [i for i, st in enumerate(got[1]) if st == 1 and want[3][i] and s.code(i)]
    assert len([i for i in mid if 10 < i < len(s.upd) - 10]) >= 10
    assert any(k is not None and k[2][-1] != 0.0 for k in _keys(got[:2])[0])
    e_on, got_on, _ = run_all(s, metrics=True)
    assert _keys(got_on[:2]) == _keys(got[:2])
    # statuses only (out == NULL, metrics off)
    alone = s.engine()
    rc, _, status, updated = raw_csi(alone, s.upd, s.idx, records=False)
    assert rc == abi.PE_OK and status == got[1] and updated == got[1].count(0)
    e2 = s.engine()
    by_select(e2, 0, s.upd, s.idx)
    same_after(s, (alone, e2), 21)


def raw_csi(st, upd, idx, records=True, tg=0):
    n = len(upd)
    arr = np.asarray(upd or [0], dtype=np.uint32)
    ix = None if idx is None else np.asarray(idx or [0], dtype=np.uint32)
    out = (abi.pe_ranked_node * max(1, n))() if records else None
    status = np.full(max(1, n), 255, dtype=np.uint8)
    updated = C.c_uint32(0)
    rc = st._lib.pe_inplace_update_csi(st._h, tg, arr.ctypes.data_as(abi.u32p),
                                       None if ix is None else ix.ctypes.data_as(abi.u32p), n, out,
                                       status.ctypes.data_as(abi.u8p), C.byref(updated))
    return rc, out, status[:n].tolist(), updated.value


@gpu
def test_terminal_alloc_and_alloc_of_another_group():
    nodes, allocs, job, upd = _multi_own(64, 120, seed=77)
    allocs[upd[3]].terminal = True
    allocs[upd[8]].terminal = True
    allocs[upd[5]].task_group = "plain"
    allocs[upd[11]].task_group = "plain"
    s = Shape(nodes, allocs, job, upd, 78)
    s.idx[3], s.idx[5] = 5, 5
    s.idx[8], s.idx[11] = 3, 3
    run_all(s, metrics=False, seed=18)
    run_all(s, metrics=True, seed=18)


@gpu
def test_many_node_groups_and_a_long_group():
    """More than 256 node groups (several workgroups) and 70 listed updates on one node."""
    nodes, allocs, job, upd = _multi_own(340, 600, seed=81)
    big = nodes[7]
    big.cpu_shares, big.memory_mb = 200000, 400000
    big.compute_class()
    base = len(allocs)
    for _ in range(70):
        allocs.append(Allocation(node_id=big.id, job_id="svc-c2", task_group="web", cpu_shares=100, memory_mb=64,
                                 disk_mb=10, priority=50))
    rng = np.random.Generator(np.random.PCG64(82))
    upd = upd + list(range(base, base + 70))
    upd = [upd[int(k)] for k in rng.permutation(len(upd))]
    s = Shape(nodes, allocs, job, upd, 83)
    assert len({allocs[i].node_id for i in upd}) > 256
    e, got, want = run_all(s, metrics=False, seed=19)
    on_big = [st for i, st in zip(upd, got[1]) if allocs[i].node_id == big.id]
    assert len(on_big) >= 70 and 0 in on_big and 1 in on_big


# ---- GPU: launches, the index afterwards, NULL indices ----------------------------------------------

def per_alloc_shape(n_vol, idx, n_extra_plugins=0):
    """`n_vol` healthy volumes vol[k] on plugin foo, which every node runs, and
    `n_extra_plugins` further volumes vol[100 + k] on plugins of their own that no node runs."""
    nodes, allocs, job, upd = _multi_own(64, len(idx), seed=85)
    for nd in nodes:
        nd.csi_node_plugins = {"foo": CSINodePlugin(True)}
    volumes = [CSIVolume("vol[%d]" % k, NS, "foo") for k in range(n_vol)]
    volumes += [CSIVolume("vol[%d]" % (100 + k), NS, "plugin-%d" % k) for k in range(n_extra_plugins)]
    return Shape(nodes, allocs, job, upd[:len(idx)], 86, idx=idx, reqs=[CSIVolumeRequest("vol", per_alloc=True)],
                 volumes=volumes)


@gpu
def test_launches_are_the_distinct_record_sets():
    # vol[0], vol[1] on foo and a missing vol[70]: two record sets
    s = per_alloc_shape(64, [0, 70, 1, 70, 0, 1, 70, 0])
    e = s.engine()
    before = e.csi_avail_launches()
    got = e.InplaceUpdateCSI(0, s.upd, s.idx, fallback=False)
    assert e.csi_avail_launches() - before == 2
    assert [st == 1 for st in got[1]] == [i == 70 for i in s.idx]
    # sixty-four healthy per_alloc volumes on one plugin: one set
    s = per_alloc_shape(64, list(range(64)))
    e = s.engine()
    before = e.csi_avail_launches()
    got = e.InplaceUpdateCSI(0, s.upd, s.idx, fallback=False)
    assert e.csi_avail_launches() - before == 1
    assert 1 not in got[1]
    same_as_model(got, model(s, s.oracle()), exact=True)


@gpu
def test_index_and_dirty_state_afterwards_and_null_indices():
    s = generic_shape(seed=87, own=60)
    s.idx[-1] = 2
    e, e2 = s.engine(), s.engine()
    got = e.InplaceUpdateCSI(0, s.upd, s.idx, fallback=False)
    a = by_select(e2, 0, s.upd, s.idx)
    assert _keys(got[:2]) == _keys(a)

    def codes(idx):
        return [csi_code(nd, s.reqs, "[%d]" % idx, s.volumes, s.node_volumes, NS, s.job.id) for nd in s.nodes]
    assert list(e.CSICheck(0)) == codes(2)             # the last listed update's index, its column current
    perm = synth.shuffle(len(s.nodes), 31)
    for st in (e, e2):
        st.SetNodes(perm)
    x, y = e.SelectRaw(0, None), e2.SelectRaw(0, None)
    assert _key(x) == _key(y)
    e.CSIAllocIndex(0, 5)
    e2.CSIAllocIndex(0, 5)
    assert list(e.CSICheck(0)) == codes(5)
    for st in (e, e2):
        st.SetNodes(perm)
    assert _key(e.SelectRaw(0, None)) == _key(e2.SelectRaw(0, None))
    # alloc_idx == NULL: every update uses the index the handle holds
    for held in (5, 1):
        n = generic_shape(seed=87, own=60, idx=[held] * 60)
        e3 = n.engine()
        e3.CSIAllocIndex(0, held)
        got3 = e3.InplaceUpdateCSI(0, n.upd, None, fallback=False)
        same_as_model(got3, model(n, n.oracle()), exact=True)
        assert list(e3.CSICheck(0)) == codes(held)


@gpu
def test_group_without_csi_requests_is_the_spread_call_byte_for_byte():
    nodes, allocs, job, upd = _multi_own(64, 150, seed=79)
    job.task_groups[0].spreads = [TARGET]
    from nomad_amd.stack import GenericStack
    res = []
    for name in ("csi", "spread"):
        st = GenericStack()
        st.SetState(nodes, allocs)
        st.SetJob(job)
        st.EnableMetrics(True)
        if name == "csi":
            before = st.csi_avail_launches()
            rc, out, status, updated = raw_csi(st, upd, list(range(len(upd))))    # alloc_idx is ignored
            assert st.csi_avail_launches() == before
        else:
            arr = np.asarray(upd, dtype=np.uint32)
            out = (abi.pe_ranked_node * len(upd))()
            stat = np.full(len(upd), 255, dtype=np.uint8)
            up = C.c_uint32(0)
            rc = st._lib.pe_inplace_update_spread(st._h, 0, arr.ctypes.data_as(abi.u32p), len(upd), out,
                                                  stat.ctypes.data_as(abi.u8p), C.byref(up))
            status, updated = stat.tolist(), up.value
        assert rc == abi.PE_OK
        res.append((bytes(out), status, updated, st.InplaceMetrics(status)))
    assert res[0] == res[1]
    assert 0 in res[0][1] and 2 in res[0][1]


# ---- GPU: refusals ----------------------------------------------------------------------------------

def untouched(e, fresh, cursor, elig):
    """tests/test_csi_place.py's assert_untouched: the cursor and limit, the
    memo, and a Select of the group without CSI (the plan and the node list)."""
    assert e.GetCursor() == cursor
    assert e.Eligibility() == elig
    assert _key(e.SelectRaw(1)) == _key(fresh.SelectRaw(1))
    assert e.csi_avail_launches() == fresh.csi_avail_launches()


def refused(s, call, match, system=False, config=None, metrics=False, csi=True, held=4):
    from nomad_amd.stack import Unsupported
    e = s.engine(system, config, metrics=metrics, csi=csi)
    f = s.engine(system, config, metrics=metrics, csi=csi)
    perm = synth.shuffle(len(s.nodes), 41)
    for st in (e, f):
        st.SetNodes(perm)
        if csi:
            st.CSIAllocIndex(0, held)
    cursor, elig = e.GetCursor(), e.Eligibility()
    with pytest.raises(Unsupported, match=match):
        call(e)
    untouched(e, f, cursor, elig)
    if csi and not metrics:         # the group's alloc index: the held one still decides its column
        want = [csi_code(nd, s.reqs, "[%d]" % held, s.volumes, s.node_volumes, NS, s.job.id) for nd in s.nodes]
        assert list(e.CSICheck(0)) == want


@gpu
def test_nine_record_sets_are_refused_and_eight_are_not():
    idx = [0] + [100 + k for k in range(abi.PE_MAX_CSI_SETS)]
    s = per_alloc_shape(1, idx, n_extra_plugins=abi.PE_MAX_CSI_SETS)
    refused(s, lambda e: e.InplaceUpdateCSI(0, s.upd, s.idx, fallback=False), "distinct CSI record sets", held=0)
    e = s.engine()
    got = e.InplaceUpdateCSI(0, s.upd[:-1], s.idx[:-1], fallback=False)
    assert got[1][0] != 1 and got[1][1:] == [1] * (len(idx) - 2)


@gpu
def test_other_refusals_leave_the_handle_untouched():
    s = generic_shape(seed=88, own=40)

    def call(e):
        return e.InplaceUpdateCSI(0, s.upd, s.idx, fallback=False)
    # a CSI group without a table: refused as pe_select refuses it
    refused(s, call, "CSI volumes", csi=False)
    # what pe_inplace_update_spread refuses: distinct_property
    d = generic_shape(seed=88, own=40)
    d.job.task_groups[0].constraints = [Constraint("${node.class}", "3", "distinct_property")]
    refused(d, lambda e: e.InplaceUpdateCSI(0, d.upd, d.idx, fallback=False), "distinct_property")
    # ... and on a preempting stack with metrics on the same list
    p = system_shape()
    p.job.task_groups[0].constraints = [Constraint("${node.class}", "3", "distinct_property")]
    refused(p, lambda e: e.InplaceUpdateCSI(0, p.upd, p.idx, fallback=False), "distinct_property", system=True,
            config=PRE, metrics=True)


@gpu
def test_non_uniform_class_is_refused_untouched():
    """Drivers are not hashed into the computed class: a listed node whose
    driver is unhealthy makes its class non-uniform for the group's checks
    (tests/test_csi.py's csi_select case)."""
    s = generic_shape(seed=89, own=40)
    nd = s.by_id[s.allocs[s.upd[7]].node_id]
    cls = nd.computed_class
    driver = s.job.task_groups[0].tasks[0].driver
    nd.drivers = dict(nd.drivers, **{driver: DriverInfo(detected=True, healthy=False)})
    assert nd.computed_class == cls and sum(1 for x in s.nodes if x.computed_class == cls) > 1
    refused(s, lambda e: e.InplaceUpdateCSI(0, s.upd, s.idx, fallback=False), "CSI volumes with computed classes")


@gpu
def test_the_four_earlier_calls_still_refuse_a_csi_group():
    s = system_shape()
    for name, kw in (("InplaceUpdate", dict()), ("InplaceUpdatePreempt", dict(config=PRE)),
                     ("InplaceUpdateMetrics", dict(config=PRE, metrics=True)),
                     ("InplaceUpdateSpread", dict(config=PRE, metrics=True))):
        refused(s, lambda e: getattr(e, name)(0, s.upd, fallback=False), "CSI volumes", system=True, **kw)
    g = generic_shape(seed=88, own=40)
    for name in ("InplaceUpdate", "InplaceUpdateMetrics", "InplaceUpdateSpread"):
        refused(g, lambda e: getattr(e, name)(0, g.upd, fallback=False), "CSI volumes")


@gpu
def test_python_fallback_is_the_per_alloc_sequence():
    """Nine record sets: the call refuses, the fallback answers as reference A."""
    idx = [0] + [100 + k for k in range(abi.PE_MAX_CSI_SETS)]
    s = per_alloc_shape(1, idx, n_extra_plugins=abi.PE_MAX_CSI_SETS)
    e, e2 = s.engine(), s.engine()
    got = e.InplaceUpdateCSI(0, s.upd, s.idx)
    assert got[2] is None and _keys(got[:2]) == _keys(by_select(e2, 0, s.upd, s.idx))
    same_as_model(got, model(s, s.oracle()), exact=True)
