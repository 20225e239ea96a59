"""In-place updates on a preempting system stack in one call
(pe_inplace_update_preempt). Ground truth is the per-call
sequence (AppendStoppedAlloc, SetNodes([node]), Select, PopUpdate and, on an
option, the stop again plus a plain AppendAlloc) on
OracleSystemStack(config=PRE), run by nomad_amd.stack.inplace_update_by_select:
the oracle's Select evicts where the plain fit fails, and the helper commits
with Commit, never CommitPreempt, as inplaceUpdate never reads
option.PreemptedAllocs (util.go:759-802). The same helper on a second engine
handle is the second witness on the shapes of at most 69 updates. Engine
against engine the records are bit-equal; engine against oracle statuses,
rows, counters and preempted lists are exact and the scores agree within the
project's 1e-12 relative (README)."""
import ctypes as C

import numpy as np
import pytest

from nomad_amd import abi, synth
from nomad_amd.stack import SelectOptions, inplace_preempted_from_csr, inplace_update_by_select
from nomad_amd.structs import Allocation, RequestedDevice, SchedulerConfig, Spread, SpreadTarget
from oracle.oracle import OracleSystemStack
from tests.test_inplace_update import _key, _keys, _multi_own
from tests.test_system_groups_preempt import _hand_cluster

gpu = pytest.mark.gpu

PRE = SchedulerConfig(preempt_system=True)
RTOL = 1e-12


def _setup(cls, nodes, allocs, job, **kw):
    st = cls(**kw)
    st.SetState(nodes, allocs)
    st.SetJob(job)
    return st


def _engine(**kw):
    from nomad_amd.stack import SystemStack
    return SystemStack(**kw)


def _own(nd, job="mock-system-0", tg="web", **kw):
    """An alloc of the job's older version: mock.SystemJob's resources."""
    f = dict(cpu_shares=500, memory_mb=256, disk_mb=300, net_mbits=50, dyn_ports=1, priority=100)
    f.update(kw)
    return Allocation(node_id=nd.id, job_id=job, task_group=tg, **f)


def _hand():
    """_hand_cluster's four nodes with one own alloc of 500 cpu on each and a
    second one on evict_a; the group asks 2000 cpu. Allocs 0-2 are the hand
    cluster's x, y, z; the update list is the own allocs 3-7."""
    nodes, allocs = _hand_cluster()
    job = synth.mock_system_job()
    job.version = 2
    job.task_groups[0].tasks[0].cpu = 2000
    for nd in nodes + [nodes[0]]:
        allocs.append(_own(nd, memory_mb=64, disk_mb=10, net_mbits=0, dyn_ports=0))
    return nodes, allocs, job, list(range(3, 8))


def _seeded(n, seed):
    """cluster_c4(n, seed) without its filler allocs. Nodes 0-5 hold 40 small
    allocs of mixed low priorities beside one own alloc (41 allocs: beyond the
    narrowest eviction width, and an eviction of 23 of them); nodes 6-11 hold
    a low-priority alloc with 960 of the 1000 MBits beside one own alloc (the
    update's 50 MBits need PreemptForNetwork); the others hold a preemptible
    2000-cpu alloc, a priority-95 one that no eviction can move, and one or
    two own allocs, each with its own probability (four draws per such node, in
    this order). The job asks 2500 cpu. Returns the update list: the own
    allocs in shuffled order. The oracle's answer: (64, 95) 66 updates,
    statuses 58 / 3 / 5, 14 evicting, six on the 41-alloc nodes with 23
    preempted each, six preempting the 960-MBit alloc; (400, 97) 417 updates,
    331 / 51 / 35, 44 evicting, 8 that follow an evicting update on their node."""
    nodes, _ = synth.cluster_c4(n, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    allocs = []
    low = dict(job_id="low", task_group="tg", memory_mb=64, disk_mb=10)
    for k, nd in enumerate(nodes):
        if k < 12:
            nd.attributes["kernel.name"] = "linux"
            nd.cpu_shares = 4000 if k < 6 else 16000
            nd.compute_class()
        if k < 6:
            for j in range(40):
                allocs.append(Allocation(node_id=nd.id, cpu_shares=80, priority=10 + j % 5, **low))
            allocs.append(_own(nd))
        elif k < 12:
            allocs.append(Allocation(node_id=nd.id, cpu_shares=500, priority=20, net_mbits=960, **low))
            allocs.append(_own(nd))
        else:
            r = rng.random(4)
            if r[0] < 0.30:
                allocs.append(Allocation(node_id=nd.id, cpu_shares=2000, priority=20, **low))
            if r[1] < 0.15:
                allocs.append(Allocation(node_id=nd.id, job_id="high", task_group="tg", cpu_shares=3000, memory_mb=64,
                                         disk_mb=10, priority=95))
            if r[2] < 0.8:
                allocs.append(_own(nd))
            if r[3] < 0.25:
                allocs.append(_own(nd))
    job = synth.mock_system_job()
    job.version = 4
    job.task_groups[0].tasks[0].cpu = 2500
    own = [i for i, a in enumerate(allocs) if a.job_id == job.id]
    upd = [own[int(k)] for k in rng.permutation(len(own))]
    return nodes, allocs, job, upd


def _oracle(nodes, allocs, job, upd, config=PRE, prep=None):
    st = _setup(OracleSystemStack, nodes, allocs, job, config=config)
    if prep:
        prep(st)
    return st, inplace_update_by_select(st, 0, upd)


_CACHE = {}


def _seeded_oracle(n, seed):
    """The seeded shape and the oracle's answer on it, computed once."""
    if (n, seed) not in _CACHE:
        shape = _seeded(n, seed)
        _CACHE[(n, seed)] = (shape, _oracle(*shape)[1])
    return _CACHE[(n, seed)]


def _facts(nodes, allocs, upd, res):
    """What an answer exercises: evicting updates, the widest evicted node,
    the longest preempted list, updates that evict the 960-MBit alloc, and
    evicting or plain updates that follow an evicting one on their node."""
    records, status = res
    per_node = {}
    for a in allocs:
        per_node[a.node_id] = per_node.get(a.node_id, 0) + 1
    evicting = [i for i, r in enumerate(records) if r is not None and r.preempted]
    seen, follow = set(), 0
    for i, r in enumerate(records):
        nid = allocs[upd[i]].node_id
        follow += nid in seen
        if r is not None and r.preempted:
            seen.add(nid)
    return dict(n=len(upd), status=[status.count(c) for c in (0, 1, 2)], evicting=len(evicting),
                wide=sum(1 for i in evicting if per_node[allocs[upd[i]].node_id] > 32),
                longest=max([len(records[i].preempted) for i in evicting] or [0]),
                mbits=sum(1 for i in evicting if any(allocs[a].net_mbits == 960 for a in records[i].preempted)),
                follow=follow)


def _same_exact(a, b):
    assert a[1] == b[1]
    assert a[0] == b[0]


def _same_oracle(a, o):
    """Engine record keys against the oracle's: everything exact but the
    scores, those within RTOL; the maximum relative difference is printed."""
    assert a[1] == o[1]
    worst = 0.0
    for x, y in zip(a[0], o[0]):
        assert (x is None) == (y is None)
        if x is None:
            continue
        assert x[0] == y[0] and x[3:7] == y[3:7] and x[8:] == y[8:], (x, y)   # row, counters, cursor, offers
        # the engine lists PreemptedAllocs by increasing slot of the node's alloc list
        # (increasing alloc-table row), the oracle in the Preemptor's order: the same set
        assert list(x[7]) == sorted(y[7]) and len(set(y[7])) == len(y[7]), (x, y)
        assert len(x[2]) == len(y[2])
        for p, q in zip((x[1],) + x[2], (y[1],) + y[2]):
            d = abs(p - q) / max(abs(q), 1e-300) if p != q else 0.0
            worst = max(worst, d)
    print("max relative score difference engine vs oracle: %.3e" % worst)
    assert worst <= RTOL


def _three(nodes, allocs, job, upd, prep=None):
    """The new call on one engine handle, the helper on the oracle and on a
    second engine handle; returns the three stacks after the comparison."""
    eng = _setup(_engine, nodes, allocs, job, config=PRE)
    eng2 = _setup(_engine, nodes, allocs, job, config=PRE)
    for st in (eng, eng2):
        if prep:
            prep(st)
    ora, ro = _oracle(nodes, allocs, job, upd, prep=prep)
    a = _keys(eng.InplaceUpdatePreempt(0, upd, fallback=False))
    c = _keys(inplace_update_by_select(eng2, 0, upd))
    _same_exact(a, c)
    _same_oracle(a, _keys(ro))
    return (eng, ora, eng2), ro


# ---- CPU: the semantics on the oracle, the CSR decoding ------------------------------

def test_evicts_again_and_leaves_the_plan_untouched():
    nodes, allocs, job, upd = _hand()
    ora, (records, status) = _oracle(nodes, allocs, job, upd)
    assert status == [0, 0, 2, 1, 0]
    # updates 0 and 4 (evict_a's two own allocs) both preempt alloc 0: the first
    # eviction never reached the plan, the node is over-committed, x goes again
    assert [r and r.preempted for r in records] == [[0], [], None, None, [0]]   # (evict_b's update fits beside y)
    ora.SetNodes([0])
    assert ora.SelectRaw(0, SelectOptions(preempt=True)).preempted == [0]   # x is still in ProposedAllocs
    _, (records, status) = _oracle(nodes, allocs, job, upd, config=None)
    assert status == [2, 0, 2, 1, 2]
    assert [r and r.preempted for r in records] == [None, [], None, None, None]


def test_inplace_preempted_csr_decoding():
    assert inplace_preempted_from_csr([], [0], []) == {}
    updates, off, rows = np.array([1, 5, 6], np.uint32), np.array([0, 2, 3, 6], np.uint32), \
        np.array([7, 9, 4, 1, 2, 3], np.uint32)
    assert inplace_preempted_from_csr(updates, off, rows) == {1: [7, 9], 5: [4], 6: [1, 2, 3]}


# ---- GPU ------------------------------------------------------------------------------

@gpu
def test_hand_cluster():
    nodes, allocs, job, upd = _hand()
    (eng, ora, eng2), ro = _three(nodes, allocs, job, upd)
    assert ro[1] == [0, 0, 2, 1, 0]
    assert eng.InplaceUpdatePreempted() == {0: [0], 4: [0]}
    for st in (eng, ora, eng2):
        st.SetNodes([0])
    sel = [_key(st.SelectRaw(0, SelectOptions(preempt=True))) for st in (eng, ora, eng2)]
    assert sel[0] == sel[2] and sel[0][8 - 1] == (0,)
    _same_oracle(([sel[0]], [0]), ([sel[1]], [0]))


def _after(stacks, nodes, allocs, upd, ro):
    """Later observable state on all three handles: PopUpdate of one updated
    alloc, the eligibility memo, SystemPlace over the rows without own allocs
    and one SelectRaw with preempt=True."""
    done = next(upd[i] for i, st in enumerate(ro[1]) if st == 0)
    have = {a.node_id for a in allocs if a.job_id == "mock-system-0"}
    rest = np.asarray([k for k, nd in enumerate(nodes) if nd.id not in have], dtype=np.uint32)
    res = []
    for st in stacks:
        st.PopUpdate(done)
        elig = st.Eligibility()
        st.SetNodes(rest)
        sc, status, placed = st.SystemPlace(0)
        st.SetNodes([int(stacks[0].state.alloc_table.node_row[done])])
        sel = _key(st.SelectRaw(0, SelectOptions(preempt=True)))
        res.append((elig, list(np.asarray(status)), placed, np.asarray(sc).copy(), sel))
    for other in res[1:]:
        assert res[0][0] == other[0] and res[0][1] == other[1] and res[0][2] == other[2]
    np.testing.assert_array_equal(res[0][3], res[2][3])
    np.testing.assert_allclose(res[0][3], res[1][3], rtol=RTOL, atol=0, equal_nan=True)
    assert res[0][4] == res[2][4]
    _same_oracle(([res[0][4]], [0]), ([res[1][4]], [0]))


@gpu
def test_seeded_small_three_way():
    (nodes, allocs, job, upd), ro = _seeded_oracle(64, 95)
    f = _facts(nodes, allocs, upd, ro)
    print(f)
    assert len(upd) <= 69
    assert all(f["status"]) and f["wide"] == 6 and f["longest"] == 23 and f["mbits"] == 6
    stacks, _ = _three(nodes, allocs, job, upd)
    assert stacks[0].InplaceUpdatePreempted() == {i: sorted(r.preempted) for i, r in enumerate(ro[0]) if r and r.preempted}
    _after(stacks, nodes, allocs, upd, ro)


@gpu
def test_seeded_larger_against_the_oracle():
    (nodes, allocs, job, upd), ro = _seeded_oracle(400, 97)
    f = _facts(nodes, allocs, upd, ro)
    print(f)
    plain = _oracle(nodes, allocs, job, upd, config=None)[1]
    assert all(f["status"])
    assert sum(1 for x, y in zip(ro[1], plain[1]) if x != y) >= 20
    assert f["wide"] >= 1 and (abi.PE_MAX_PREEMPT >= 23 or f["longest"] > abi.PE_MAX_PREEMPT)
    assert f["mbits"] >= 1 and f["follow"] >= 2
    eng = _setup(_engine, nodes, allocs, job, config=PRE)
    _same_oracle(_keys(eng.InplaceUpdatePreempt(0, upd, fallback=False)), _keys(ro))
    assert eng.InplaceUpdatePreempted() == {i: sorted(r.preempted) for i, r in enumerate(ro[0]) if r and r.preempted}


@gpu
def test_max_parallel_candidates_after_a_committed_preemption():
    # 16 nodes of 3900 usable cpu; a priority-20 candidate of job "mp" on each,
    # max_parallel 1 and 2 in turn, beside one own alloc: 2000 + the ask's 2500
    # needs the eviction. Before the call a Select with preempt on node 15 and
    # its CommitPreempt put one "mp" alloc into the plan's preemption counts,
    # which the max_parallel penalty (preemption.go:220-240) then reads
    nodes, _ = synth.cluster_c1(16, seed=31)
    allocs = [Allocation(node_id=nd.id, job_id="mp", task_group="tg", cpu_shares=2000, memory_mb=64, disk_mb=10,
                         priority=20, max_parallel=1 + k % 2) for k, nd in enumerate(nodes)]
    allocs += [Allocation(node_id=nd.id, job_id="mp", task_group="tg", cpu_shares=300, memory_mb=64, disk_mb=10,
                          priority=20, max_parallel=1 + k % 2) for k, nd in enumerate(nodes) if k % 3 == 0]
    base = len(allocs)
    allocs += [_own(nd) for nd in nodes[:15]]
    job = synth.mock_system_job()
    job.version = 3
    job.task_groups[0].tasks[0].cpu = 2500
    upd = [base + int(k) for k in np.random.Generator(np.random.PCG64(32)).permutation(15)]

    def prep(st):
        st.SetNodes([15])
        r = st.SelectRaw(0, SelectOptions(preempt=True))
        assert r.row == 15 and r.preempted
        st.Commit(0, r.row, r.preempted)      # CommitPreempt

    stacks, ro = _three(nodes, allocs, job, upd, prep=prep)
    assert ro[1].count(0) == 15 and all(r.preempted for r in ro[0])


@gpu
@pytest.mark.parametrize("kind", ["generic", "system"])
def test_without_preemption_it_is_the_plain_call(kind):
    from nomad_amd.stack import GenericStack
    nodes, allocs, job, upd = _multi_own(64, 200, seed=71)
    cls = GenericStack if kind == "generic" else _engine
    a, c = _setup(cls, nodes, allocs, job), _setup(cls, nodes, allocs, job)
    n = len(upd)
    arr = np.asarray(upd, dtype=np.uint32)
    out = (abi.pe_ranked_node * n)()
    status = np.full(n, 255, dtype=np.uint8)
    updated = C.c_uint32(0)
    a._check(a._lib.pe_inplace_update_preempt(a._h, 0, arr.ctypes.data_as(abi.u32p), n, out,
                                              status.ctypes.data_as(abi.u8p), C.byref(updated)))
    out2 = (abi.pe_ranked_node * n)()
    status2 = np.full(n, 255, dtype=np.uint8)
    c._check(c._lib.pe_inplace_update(c._h, 0, arr.ctypes.data_as(abi.u32p), n, out2,
                                      status2.ctypes.data_as(abi.u8p), C.byref(updated)))
    assert bytes(out) == bytes(out2) and status.tolist() == status2.tolist()
    assert 0 in status and 2 in status
    up, of, al, ne = abi.u32p(), abi.u32p(), abi.u32p(), C.c_uint32(7)
    assert a._lib.pe_inplace_update_preempted(a._h, C.byref(up), C.byref(of), C.byref(al), C.byref(ne)) == abi.PE_OK
    assert ne.value == 0
    perm = synth.shuffle(64, 12)
    runs = []
    for st in (a, c):
        st.SetNodes(perm)
        runs.append([_key(st.Select(0)) for _ in range(3)])
    assert runs[0] == runs[1]


def _refusal_shapes():
    def device(nodes, allocs, job):
        job.task_groups[0].tasks[0].devices = [RequestedDevice("nvidia/gpu", 1)]

    def crowded(nodes, allocs, job):
        allocs.extend(Allocation(node_id=nodes[4].id, job_id="tiny", task_group="tg", cpu_shares=1, memory_mb=1,
                                 disk_mb=1, priority=20) for _ in range(1030))

    return {"a device ask": device, "metrics on": None, "a node of 1030 allocs": crowded}


@gpu
def test_a_spread_is_refused_as_by_the_plain_call():
    # a system stack has no SpreadIterator (stack.go:207-283) and drops the job's
    # spreads; where they count, on a generic stack, the new entry is
    # pe_inplace_update and refuses them as it does
    from nomad_amd.stack import GenericStack
    from oracle.oracle import OracleGenericStack
    nodes, allocs, job, upd = _multi_own(64, 60, seed=79)
    job.task_groups[0].spreads = [Spread("${node.class}", 60, [SpreadTarget("class-1", 40),
                                                             SpreadTarget("class-2", 30)])]
    eng = _setup(GenericStack, nodes, allocs, job)
    arr = np.asarray(upd, dtype=np.uint32)
    status = np.full(len(upd), 255, dtype=np.uint8)
    rc = eng._lib.pe_inplace_update_preempt(eng._h, 0, arr.ctypes.data_as(abi.u32p), len(upd), None,
                                            status.ctypes.data_as(abi.u8p), None)
    assert rc == abi.PE_EUNSUPPORTED and set(status.tolist()) == {255}
    ora = _setup(OracleGenericStack, nodes, allocs, job)
    assert _keys(inplace_update_by_select(eng, 0, upd)) == _keys(inplace_update_by_select(ora, 0, upd))


@gpu
@pytest.mark.parametrize("case", sorted(_refusal_shapes()))
def test_refusals_leave_the_handle_as_it_was(case):
    from nomad_amd.stack import Unsupported
    nodes, allocs = synth.cluster_c4(40, seed=80)
    allocs = [Allocation(node_id=nd.id, job_id="low", task_group="tg", cpu_shares=2000, memory_mb=64, disk_mb=10,
                         priority=20) for nd in nodes[::3]]
    edit = _refusal_shapes()[case]
    job = synth.mock_system_job()
    job.task_groups[0].tasks[0].cpu = 2500
    if edit:
        edit(nodes, allocs, job)
    base = len(allocs)
    allocs += [_own(nd) for nd in nodes[::2]]
    upd = list(range(base, len(allocs)))
    eng = _setup(_engine, nodes, allocs, job, config=PRE)
    if case == "metrics on":
        eng.EnableMetrics(True)
    with pytest.raises(Unsupported):
        eng.InplaceUpdatePreempt(0, upd, fallback=False)
    if case == "metrics on":
        eng.EnableMetrics(False)
    try:
        got = _keys(inplace_update_by_select(eng, 0, upd))     # the refusal changed nothing
    except Unsupported:
        # the engine's own preempting Select refuses this snapshot too: a fresh handle's answer
        with pytest.raises(Unsupported):
            inplace_update_by_select(_setup(_engine, nodes, allocs, job, config=PRE), 0, upd)
        return
    _same_oracle(got, _keys(_oracle(nodes, allocs, job, upd)[1]))


@gpu
def test_argument_errors_the_accessor_and_statuses_only():
    from nomad_amd.stack import EngineError, Unsupported
    nodes, allocs, job, upd = _hand()
    eng = _setup(_engine, nodes, allocs, job, config=PRE)
    pre_args = [C.byref(x) for x in (abi.u32p(), abi.u32p(), abi.u32p(), C.c_uint32(0))]
    assert eng._lib.pe_inplace_update_preempted(eng._h, *pre_args) == abi.PE_ESTATE      # before any call
    for bad, tg in (([upd[0], upd[1], upd[0]], 0), ([upd[0], len(allocs)], 0), (upd[:3], 5)):
        with pytest.raises(EngineError) as e:
            eng.InplaceUpdatePreempt(tg, bad, fallback=False)
        assert e.value.code == abi.PE_EINVAL and not isinstance(e.value, Unsupported)
    assert eng._lib.pe_inplace_update_preempted(eng._h, *pre_args) == abi.PE_ESTATE      # the failed calls left none
    # out == NULL: the statuses and the CSR all the same
    arr = np.asarray(upd, dtype=np.uint32)
    status = np.full(len(upd), 255, dtype=np.uint8)
    updated = C.c_uint32(0)
    eng._check(eng._lib.pe_inplace_update_preempt(eng._h, 0, arr.ctypes.data_as(abi.u32p), len(upd), None,
                                                  status.ctypes.data_as(abi.u8p), C.byref(updated)))
    assert status.tolist() == [0, 0, 2, 1, 0] and updated.value == 3
    assert eng.InplaceUpdatePreempted() == {0: [0], 4: [0]}
    # the plain entry keeps its refusal on this stack, and ends the CSR's validity only when it runs
    with pytest.raises(Unsupported):
        eng.InplaceUpdate(0, upd, fallback=False)
    assert eng.InplaceUpdatePreempted() == {0: [0], 4: [0]}
    eng.ResetPlan()
    eng.SetJob(job)
    assert eng.InplaceUpdatePreempt(0, [], fallback=False) == ([], [])
    assert eng.InplaceUpdatePreempted() == {}
