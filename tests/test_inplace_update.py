"""Batched in-place update check (pe_inplace_update):
inplaceUpdate's loop (scheduler/util.go:692-806) for a list of snapshot allocs
in one launch. Ground truth is the per-call sequence (AppendStoppedAlloc,
SetNodes([node]), Select, PopUpdate, and on an option the stop again plus
AppendAlloc) on the oracle, run by nomad_amd.stack.inplace_update_by_select;
the same helper on a second engine handle is the second witness. Records are
compared bit for bit, scores included: both paths run the same arithmetic."""
import numpy as np
import pytest

from nomad_amd import abi, synth
from nomad_amd.stack import inplace_update_by_select
from nomad_amd.structs import Allocation, Constraint, SchedulerConfig, Spread, SpreadTarget, Task, TaskGroup
from oracle.oracle import OracleGenericStack, OracleSystemStack


def _key(r):
    if r is None:
        return None
    return (r.row, r.final_score, tuple(r.scores), r.nodes_evaluated, r.nodes_filtered, r.nodes_exhausted,
            r.new_offset, tuple(r.preempted), tuple(r.device_offers))


def _keys(res):
    records, status = res
    return [_key(r) for r in records], [int(x) for x in status]


def _loop(st, count, tg=0):
    out = []
    for _ in range(count):
        opt = st.Select(tg)
        out.append(_key(opt))
        if opt is None:
            break
        st.Commit(tg, opt.row)
    return out


def _setup(cls, nodes, allocs, job, **kw):
    st = cls(**kw)
    st.SetState(nodes, allocs)
    st.SetJob(job)
    return st


def _multi_own(n, own, seed, cpu=900, mem=512):
    """A C2-shaped cluster where an older version of job 'svc-c2' holds `own`
    allocs on nodes drawn with replacement (several per node), beside the
    foreign ones; the updated job asks for `cpu` / `mem`. Returns the update
    list in shuffled order."""
    nodes, allocs = synth.cluster_c2(n, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    for k in rng.integers(0, n, size=own):
        allocs.append(Allocation(node_id=nodes[int(k)].id, job_id="svc-c2", task_group="web",
                                 cpu_shares=500, memory_mb=256, disk_mb=150, priority=50))
    job = synth.job_c2(own)
    job.version = 7
    job.task_groups[0].tasks[0].cpu = cpu
    job.task_groups[0].tasks[0].memory_mb = mem
    own_idx = [i for i, a in enumerate(allocs) if a.job_id == "svc-c2"]
    upd = [own_idx[int(k)] for k in rng.permutation(len(own_idx))]
    return nodes, allocs, job, upd


# ---- C1: the helper and the order semantics (CPU) ---------------------------------

@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_helper_updates_in_list_order(order):
    # one mock node: 4000 - 100 reserved = 3900 usable cpu; the job's allocs
    # hold 500 (alloc 0) and 1000 (alloc 1). The updated group asks 2000: with
    # the first listed alloc stopped the node holds at most 1000 + 2000 <=
    # 3900, so that update fits; for the second one the node holds the updated
    # 2000, and 2000 + 2000 > 3900 whichever alloc is stopped
    nodes, _ = synth.cluster_c1(1, seed=4)
    allocs = [Allocation(node_id=nodes[0].id, job_id="mock-service-0", task_group="web", cpu_shares=c,
                         memory_mb=256, disk_mb=150) for c in (500, 1000)]
    job = synth.mock_job(count=2)
    job.task_groups[0].tasks[0].cpu = 2000
    job.task_groups.append(TaskGroup(name="probe", count=1, tasks=[Task(name="p", driver="exec", cpu=1000,
                                                                        memory_mb=64)]))
    st = _setup(OracleGenericStack, nodes, allocs, job)
    records, status = inplace_update_by_select(st, 0, list(order))
    assert status == [0, 2]
    assert records[0] is not None and records[0].row == 0 and records[1] is None
    # which alloc was replaced shows in what is left: the updated 2000 beside
    # alloc 1's 1000 leaves 900 (the probe's 1000 does not fit), beside alloc
    # 0's 500 it leaves 1400 (it fits)
    st.SetNodes([0])
    assert (st.Select(1) is not None) == (order[0] == 1)
    # only the replaced alloc's stop is in NodeUpdate: PopUpdate of the other
    # changes nothing, PopUpdate of it brings the old alloc back beside the new
    st.PopUpdate(order[1])
    assert (st.Select(1) is not None) == (order[0] == 1)
    st.PopUpdate(order[0])
    assert st.Select(1) is None                      # 2000 + 500 + 1000 + the probe's 1000 > 3900


# ---- engine vs the per-call sequence (GPU) -----------------------------------------

def _three(nodes, allocs, job, upd, prep=None, system=False, config=None):
    """The batched call on one engine handle, the helper on the oracle and on
    a second engine handle: [(stack, (record keys, statuses))] x 3."""
    from nomad_amd.stack import GenericStack, SystemStack
    eng_cls, ora_cls = (SystemStack, OracleSystemStack) if system else (GenericStack, OracleGenericStack)
    out = []
    for cls, batched in ((eng_cls, True), (ora_cls, False), (eng_cls, False)):
        st = _setup(cls, nodes, allocs, job, config=config)
        if prep:
            prep(st)
        res = st.InplaceUpdate(0, upd, fallback=False) if batched else inplace_update_by_select(st, 0, upd)
        out.append((st, _keys(res)))
    return out


def _assert_same_after(stacks, n, seed, count=30):
    """Later observable state: plain placements and the eligibility memo."""
    perm = synth.shuffle(n, seed)
    runs, elig = [], []
    for st in stacks:
        st.SetNodes(perm)
        runs.append(_loop(st, count))
        elig.append(st.Eligibility())
    assert runs[0] == runs[1] == runs[2]
    assert elig[0] == elig[1] == elig[2]
    return runs[0]


@pytest.mark.gpu
def test_several_own_allocs_per_node():
    from nomad_amd.stack import GenericStack
    nodes, allocs, job, upd = _multi_own(64, 200, seed=71)
    per_node = {}
    for i in upd:
        per_node[allocs[i].node_id] = per_node.get(allocs[i].node_id, 0) + 1
    assert max(per_node.values()) >= 5 and min(per_node.values()) == 1   # from one to several per node
    (eng, a), (ora, b), (eng2, c) = _three(nodes, allocs, job, upd)
    assert a[1] == b[1] == c[1]
    assert a[0] == b[0] == c[0]
    assert 0 in a[1] and 2 in a[1]
    _assert_same_after((eng, ora, eng2), 64, 12)
    # a new evaluation on the handle starts from the snapshot again
    eng.ResetPlan()
    eng.SetJob(job)
    eng.SetNodes(synth.shuffle(64, 13))
    fresh = _setup(GenericStack, nodes, allocs, job)
    fresh.SetNodes(synth.shuffle(64, 13))
    assert _key(eng.Select(0)) == _key(fresh.Select(0))


@pytest.mark.gpu
def test_filtered_updates_and_the_eligibility_memo():
    nodes, allocs, job, upd = _multi_own(64, 200, seed=72)
    job.constraints.append(Constraint("${node.class}", "^class-[3-7]$", "regexp"))
    (eng, a), (ora, b), (eng2, c) = _three(nodes, allocs, job, upd)
    assert a == b == c
    assert 1 in a[1] and 0 in a[1]
    cls = [st.GetClasses(st.Eligibility()) for st in (eng, ora, eng2)]
    assert cls[0] == cls[1] == cls[2]
    assert True in cls[1].values() and False in cls[1].values()
    _assert_same_after((eng, ora, eng2), 64, 14)


def _c5_own(n, seed):
    """C5 cluster where job 'svc-c5' (an older version) holds two instances of
    the GPU group on the nodes that had two free: its ask fits again only when
    the old alloc's instances are discounted."""
    nodes, allocs = synth.cluster_c5(n, seed=seed)
    held = {}
    for a in allocs:
        held[a.node_id] = held.get(a.node_id, 0) + sum(c for _, c in a.devices)
    tight = set()   # the own allocs whose node has fewer than two instances free beside them
    for nd in nodes:
        free = nd.devices[0].healthy - held.get(nd.id, 0) if nd.devices else 0
        if free >= 2:
            if free - 2 < 2:
                tight.add(len(allocs))
            allocs.append(Allocation(node_id=nd.id, job_id="svc-c5", task_group="infer", cpu_shares=1000,
                                     memory_mb=2048, disk_mb=150, priority=80, devices=[(0, 2)]))
    job = synth.job_c5(100)
    job.version = 3
    upd = [i for i, a in enumerate(allocs) if a.job_id == "svc-c5"]
    rng = np.random.Generator(np.random.PCG64(seed + 2))
    return nodes, allocs, job, [upd[int(k)] for k in rng.permutation(len(upd))], tight


@pytest.mark.gpu
def test_device_instances_of_the_old_alloc_are_discounted():
    nodes, allocs, job, upd, tight = _c5_own(300, seed=73)
    (eng, a), (ora, b), (eng2, c) = _three(nodes, allocs, job, upd)
    assert a == b == c
    # updates that fit only because the old alloc's two instances came back
    assert sum(1 for i, st in zip(upd, a[1]) if st == 0 and i in tight) >= 10
    assert 1 in a[1]                                               # the 11 GiB model fails the device constraint
    assert all(len(k[8]) == 1 for k in a[0] if k is not None)      # the device offers ride in the records
    _assert_same_after((eng, ora, eng2), 300, 15, count=20)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["distinct_hosts", "anti_affinity"])
def test_own_collision_is_discounted(kind):
    # nodes 0-9 hold one alloc of the group, nodes 10-19 two
    nodes, allocs = synth.cluster_c2(40, seed=74)
    base = len(allocs)
    for k in list(range(20)) + list(range(10, 20)):
        allocs.append(Allocation(node_id=nodes[k].id, job_id="svc-c2", task_group="web",
                                 cpu_shares=500, memory_mb=256, disk_mb=150, priority=50))
    job = synth.job_c2(30)
    job.version = 2
    if kind == "distinct_hosts":
        job.task_groups[0].constraints = [Constraint("", "", "distinct_hosts")]
    upd = [base + int(k) for k in np.random.Generator(np.random.PCG64(5)).permutation(30)]
    (eng, a), (ora, b), (eng2, c) = _three(nodes, allocs, job, upd)
    assert a == b == c
    row = eng.row
    two = {row(nodes[k].id) for k in range(10, 20)}
    for i, key, st in zip(upd, a[0], a[1]):
        on_two = row(allocs[i].node_id) in two
        if kind == "distinct_hosts":
            # alone on its node the alloc's own collision is gone; with a second
            # alloc of the group there the node stays taken for both
            assert st == (1 if on_two else 0)
        elif st == 0:
            # binpack alone, or binpack + the penalty for the other alloc of the group
            assert len(key[2]) == (2 if on_two else 1)
    _assert_same_after((eng, ora, eng2), 40, 16, count=12)


@pytest.mark.gpu
def test_dynamic_ports_and_bandwidth_of_the_old_alloc():
    # mock.Job's group network asks two dynamic ports; the old allocs hold two
    # each, foreign ones hold bandwidth and ports as well
    nodes, _ = synth.cluster_c1(24, seed=82)
    rng = np.random.Generator(np.random.PCG64(83))
    allocs = [Allocation(node_id=nodes[int(k)].id, job_id="other", task_group="tg", cpu_shares=300, memory_mb=300,
                         disk_mb=100, net_mbits=200, dyn_ports=3) for k in rng.integers(0, 24, size=20)]
    base = len(allocs)
    for k in rng.integers(0, 24, size=60):
        allocs.append(Allocation(node_id=nodes[int(k)].id, job_id="mock-service-0", task_group="web", cpu_shares=500,
                                 memory_mb=256, disk_mb=150, dyn_ports=2))
    job = synth.mock_job(count=60)
    job.version = 5
    job.task_groups[0].tasks[0].cpu = 800
    upd = [base + int(k) for k in rng.permutation(60)]
    (eng, a), (ora, b), (eng2, c) = _three(nodes, allocs, job, upd)
    assert a == b == c
    assert 0 in a[1] and 2 in a[1]
    _assert_same_after((eng, ora, eng2), 24, 20, count=15)


@pytest.mark.gpu
def test_system_stack():
    n = 3000
    nodes, allocs = synth.cluster_c4(n, seed=75)
    rng = np.random.Generator(np.random.PCG64(76))
    have = rng.random(n) < 0.8
    base = len(allocs)
    for k in range(n):
        if have[k]:
            allocs.append(Allocation(node_id=nodes[k].id, job_id="mock-system-0", task_group="web", cpu_shares=500,
                                     memory_mb=256, disk_mb=300, net_mbits=50, dyn_ports=1, priority=100))
    job = synth.mock_system_job()
    job.version = 4
    job.task_groups[0].tasks[0].cpu = 1500
    upd = [base + int(k) for k in rng.permutation(len(allocs) - base)]
    from nomad_amd.stack import SystemStack
    eng = _setup(SystemStack, nodes, allocs, job)
    ora = _setup(OracleSystemStack, nodes, allocs, job)
    a = _keys(eng.InplaceUpdate(0, upd, fallback=False))
    b = _keys(inplace_update_by_select(ora, 0, upd))
    assert a[1] == b[1]
    assert {0, 1, 2} <= set(a[1])
    assert [k and (k[0], k[1]) for k in a[0]] == [k and (k[0], k[1]) for k in b[0]]
    rest = np.asarray([k for k in range(n) if not have[k]], dtype=np.uint32)
    res = []
    for st in (eng, ora):
        st.SetNodes(rest)
        sc, status, placed = st.SystemPlace(0)
        res.append((list(np.asarray(status)), placed, np.asarray(sc).copy()))
        assert st.Eligibility() == eng.Eligibility()
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    np.testing.assert_array_equal(res[0][2], res[1][2])


@pytest.mark.gpu
def test_earlier_stops_and_commits_then_pop_update():
    nodes, allocs, job, upd = _multi_own(64, 200, seed=77)
    foreign = [i for i, a in enumerate(allocs) if a.job_id != "svc-c2"]
    stop = foreign[::3]

    def prep(st):
        st.StopAllocs(stop)
        st.SetNodes(synth.shuffle(64, 17))
        assert len(_loop(st, 20)) == 20

    (eng, a), (ora, b), (eng2, c) = _three(nodes, allocs, job, upd, prep=prep)
    assert a == b == c
    assert 0 in a[1] and 2 in a[1]
    # an updated alloc that is its node's last NodeUpdate entry, and one that is not
    done = {}
    for i, st in zip(upd, a[1]):
        if st == 0:
            done.setdefault(allocs[i].node_id, []).append(i)
    last = next(v[-1] for v in done.values() if len(v) >= 2)
    not_last = next(v[0] for v in done.values() if len(v) >= 2 and v[-1] != last)
    for st in (eng, ora, eng2):
        st.PopUpdate(not_last)     # nothing changes
        st.PopUpdate(last)         # the old alloc is back beside the updated one
    _assert_same_after((eng, ora, eng2), 64, 18)


@pytest.mark.gpu
def test_pending_speculation_is_flushed_first():
    from nomad_amd.stack import GenericStack
    from tests.test_spec_view import CCaller, ViewAnswers, protocol_answers
    nodes, allocs, job, upd = _multi_own(64, 120, seed=78)
    perm = synth.shuffle(64, 19)
    eng = _setup(GenericStack, nodes, allocs, job)
    ora = _setup(OracleGenericStack, nodes, allocs, job)
    eng.SetNodes(perm)
    ora.SetNodes(perm)
    vc = ViewAnswers(eng)
    a = protocol_answers(vc, 10, preempt=False)
    b = protocol_answers(CCaller(ora), 10, preempt=False)
    assert vc.served > 0 and eng.SpeculationStats()[3] > 10        # records of the run are still pending
    ra = _keys(eng.InplaceUpdate(0, upd, fallback=False))
    rb = _keys(inplace_update_by_select(ora, 0, upd))
    assert ra == rb
    eng.SetNodes(perm)
    ora.SetNodes(perm)
    a += protocol_answers(vc, 10, preempt=False)
    b += protocol_answers(CCaller(ora), 10, preempt=False)
    assert a == b and len(a) == 20
    assert eng.Eligibility() == ora.Eligibility()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["spread", "system_preempt"])
def test_refusals_leave_the_handle_as_it_was(kind):
    from nomad_amd.stack import GenericStack, SystemStack, Unsupported
    if kind == "spread":
        nodes, allocs, job, upd = _multi_own(64, 60, seed=79)
        job.task_groups[0].spreads = [Spread("${node.class}", 60, [SpreadTarget("class-1", 40),
                                                                 SpreadTarget("class-2", 30)])]
        eng_cls, ora_cls, cfg = GenericStack, OracleGenericStack, None
    else:
        nodes, allocs = synth.cluster_c4(200, seed=80)
        base = len(allocs)
        for k in range(0, 200, 2):
            allocs.append(Allocation(node_id=nodes[k].id, job_id="mock-system-0", task_group="web", cpu_shares=500,
                                     memory_mb=256, disk_mb=300, net_mbits=50, dyn_ports=1, priority=100))
        job = synth.mock_system_job()
        job.task_groups[0].tasks[0].cpu = 1500
        upd = list(range(base, len(allocs)))
        eng_cls, ora_cls, cfg = SystemStack, OracleSystemStack, SchedulerConfig(preempt_system=True)
    ora = _setup(ora_cls, nodes, allocs, job, config=cfg)
    want = _keys(inplace_update_by_select(ora, 0, upd))
    eng = _setup(eng_cls, nodes, allocs, job, config=cfg)
    with pytest.raises(Unsupported):
        eng.InplaceUpdate(0, upd, fallback=False)
    key = (lambda r: r) if kind == "spread" else (lambda r: [k and (k[0], k[1]) for k in r])
    got = _keys(inplace_update_by_select(eng, 0, upd))     # the refusal changed nothing
    assert got[1] == want[1] and key(got[0]) == key(want[0])
    eng2 = _setup(eng_cls, nodes, allocs, job, config=cfg)
    got = _keys(eng2.InplaceUpdate(0, upd))                # fallback=True: the helper answers
    assert got[1] == want[1] and key(got[0]) == key(want[0])


@pytest.mark.gpu
def test_statuses_only_when_no_records_are_asked_for():
    # out == NULL (nomad_pe.h): the same outcomes and the same state, no records
    import ctypes as C
    from nomad_amd.stack import GenericStack
    nodes, allocs, job, upd = _multi_own(64, 120, seed=84)
    eng = _setup(GenericStack, nodes, allocs, job)
    eng2 = _setup(GenericStack, nodes, allocs, job)
    want = _keys(eng2.InplaceUpdate(0, upd, fallback=False))
    a = np.asarray(upd, dtype=np.uint32)
    status = np.full(len(upd), 255, dtype=np.uint8)
    updated = C.c_uint32(0)
    eng._check(eng._lib.pe_inplace_update(eng._h, 0, a.ctypes.data_as(abi.u32p), len(upd), None,
                                          status.ctypes.data_as(abi.u8p), C.byref(updated)))
    assert [int(x) for x in status] == want[1] and updated.value == want[1].count(0)
    assert 0 in want[1] and 2 in want[1]
    perm = synth.shuffle(64, 21)
    eng.SetNodes(perm)
    eng2.SetNodes(perm)
    assert _loop(eng, 20) == _loop(eng2, 20)


@pytest.mark.gpu
def test_argument_errors():
    from nomad_amd.stack import EngineError, GenericStack, Unsupported
    nodes, allocs, job, upd = _multi_own(64, 60, seed=81)
    eng = _setup(GenericStack, nodes, allocs, job)
    ora = _setup(OracleGenericStack, nodes, allocs, job)
    for bad, tg in (([upd[0], upd[1], upd[0]], 0), ([upd[0], len(allocs)], 0), (upd[:3], 5)):
        with pytest.raises(EngineError) as e:
            eng.InplaceUpdate(tg, bad, fallback=False)
        assert e.value.code == abi.PE_EINVAL and not isinstance(e.value, Unsupported)
    assert eng.InplaceUpdate(0, [], fallback=False) == ([], [])
    # none of them changed the handle
    assert _keys(eng.InplaceUpdate(0, upd, fallback=False)) == _keys(inplace_update_by_select(ora, 0, upd))
