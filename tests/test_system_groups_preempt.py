"""Multi-group system placement on a preempting stack (pe_system_place_groups_preempt).

The reference's default scheduler configuration enables preemption for system
jobs (nomad/config.go:448-455): a single-node Select whose plain BinPack fails
its fit goes into BinPack with evict (stack.go:267-278), and the option is
followed by Plan.AppendAlloc and Plan.AppendPreemptedAlloc of each preempted
alloc. The CPU part pins the per-Select reference loop on the oracle with a
hand-built cluster and the decoding of the preempted lists. The GPU part
compares the batched call with that loop on the oracle and with sequential
SystemPlace(g) calls on a second engine handle: outcomes, counts and the
preempted allocs equal, FinalScores bit-equal between the engine handles and
within 1e-12 relative of the oracle (README), and the same for
EvalEligibility, a further SystemPlace of a group that was not listed and one
per-Select Select with Preempt.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from nomad_amd import abi, synth
from nomad_amd.stack import (SelectOptions, preempted_from_csr, system_place_groups_by_select,
                             system_place_groups_preempt_by_select)
from nomad_amd.structs import (Allocation, Constraint, NetworkResource, RequestedDevice, SchedulerConfig, Task,
                               TaskGroup)
from oracle.oracle import OracleSystemStack

gpu = pytest.mark.gpu

PRE = SchedulerConfig(preempt_system=True)


def _tg(name, cpu, mem=64, net=None, devices=(), constraints=(), tg_net=None, cores=0):
    return TaskGroup(name=name, count=1, ephemeral_disk_mb=50, constraints=list(constraints), network=tg_net,
                     tasks=[Task(name=name, driver="exec", cpu=cpu, memory_mb=mem, network=net,
                                 devices=list(devices), cores=cores)])


def _sys_job(groups, constraints=()):
    job = synth.mock_system_job("sys-groups-pre")   # priority 100
    job.constraints = job.constraints + list(constraints)
    job.task_groups = list(groups)
    return job


def _setup(st, nodes, allocs, job, rows):
    st.SetState(nodes, allocs)
    st.SetJob(job)
    st.SetNodes(rows)
    return st


# ---- CPU: the per-Select loop on the oracle, the CSR decoding -----------------

def _hand_cluster():
    """evict_a: group a evicts x, b then fits in the freed room; evict_b: a
    fits, b evicts y; stuck: the blocking alloc z is priority 95 (less than 10
    below the job's 100), eviction cannot help; win: constraint-filtered."""
    ids = sorted(synth.uuids(4, 3))
    evict_a, evict_b, stuck, win = (synth.mock_node(i) for i in ids)
    evict_a.cpu_shares = evict_b.cpu_shares = 8000      # 7900 after the reserved 100
    win.attributes["kernel.name"] = "windows"
    for nd in (evict_a, evict_b, stuck, win):
        nd.compute_class()
    low = dict(job_id="low", task_group="tg", memory_mb=64, disk_mb=10, priority=20)
    allocs = [Allocation(node_id=evict_a.id, cpu_shares=6500, **low),    # x: a's 2000 does not fit beside it
              Allocation(node_id=evict_b.id, cpu_shares=3500, **low),    # y: a fits (5500), b's 2500 does not (8000)
              Allocation(node_id=stuck.id, job_id="high", task_group="tg", cpu_shares=3000, memory_mb=64,
                         disk_mb=10, priority=95)]                       # z: 3900 available, 900 free
    return [evict_a, evict_b, stuck, win], allocs


def test_by_select_helper_evicts_on_the_oracle():
    nodes, allocs = _hand_cluster()
    job = _sys_job([_tg("a", 2000), _tg("b", 2500)])
    o = _setup(OracleSystemStack(config=PRE), nodes, allocs, job, nodes)
    score, status, counts, placed, pre = system_place_groups_preempt_by_select(o, [0, 1])
    assert status.tolist() == [[0, 0], [0, 0], [2, 2], [1, 1]]
    assert counts.tolist() == [[2, 1, 1], [2, 1, 1]]
    assert placed == 4
    assert pre == {(0, 0): [0], (1, 1): [1]}
    assert np.array_equal(np.isnan(score), status != 0)
    # the same cluster without preemption: the evicting entries are exhausted, nothing is preempted
    o = _setup(OracleSystemStack(), nodes, allocs, job, nodes)
    _, status, _, placed, pre = system_place_groups_preempt_by_select(o, [0, 1])
    assert status.tolist() == [[2, 2], [0, 2], [2, 2], [1, 1]] and placed == 1 and pre == {}
    # the four-result helper is the same loop
    o = _setup(OracleSystemStack(config=PRE), nodes, allocs, job, nodes)
    assert system_place_groups_by_select(o, [0, 1])[1].tolist() == [[0, 0], [0, 0], [2, 2], [1, 1]]


def test_preempted_csr_decoding():
    assert preempted_from_csr([], [0], [], 3) == {}
    entries, off, allocs = np.array([1, 5, 6], np.uint32), np.array([0, 2, 3, 6], np.uint32), \
        np.array([7, 9, 4, 1, 2, 3], np.uint32)
    assert preempted_from_csr(entries, off, allocs, 3) == {(0, 1): [7, 9], (1, 2): [4], (2, 0): [1, 2, 3]}
    assert preempted_from_csr(entries, off, allocs, 1) == {(1, 0): [7, 9], (5, 0): [4], (6, 0): [1, 2, 3]}


# ---- GPU ----------------------------------------------------------------------

def _engine(**kw):
    from nomad_amd.stack import SystemStack
    return SystemStack(**kw)


def _sequential(st, tgs):
    """pe_system_place group after group, in SystemPlaceGroups' shape."""
    n, G = len(st._visit), len(tgs)
    score, status = np.full((n, G), np.nan), np.zeros((n, G), dtype=np.uint8)
    placed = 0
    for k, g in enumerate(tgs):
        sc, ss, p = st.SystemPlace(g)
        status[:, k] = ss
        score[:, k] = np.where(ss == 0, sc, np.nan)
        placed += p
    counts = np.stack([np.bincount(status[:, k], minlength=3)[:3] for k in range(G)]).astype(np.uint32) \
        if G else np.zeros((0, 3), np.uint32)
    return score, status, counts, placed


def _same_exact(a, b):
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[2], b[2])
    assert a[3] == b[3]
    assert np.array_equal(a[0].view(np.uint64)[a[1] == 0], b[0].view(np.uint64)[b[1] == 0])   # bit-equal
    assert np.isnan(a[0][a[1] != 0]).all() and np.isnan(b[0][b[1] != 0]).all()


def _same_oracle(a, o):
    assert np.array_equal(a[1], o[1])
    assert np.array_equal(a[2], o[2])
    assert a[3] == o[3]
    m = a[1] == 0
    print("max relative score difference to the oracle:",
          float(np.max(np.abs(a[0][m] - o[0][m]) / np.abs(o[0][m]))) if m.any() else 0.0)
    assert np.allclose(a[0][m], o[0][m], rtol=1e-12, atol=0.0)
    if len(a) > 4:
        assert a[4] == o[4]   # the preempted allocs of every evicting entry


def _after(st, rows, extra, tg, after_rows=None):
    """What the tests compare after the placements: the eligibility maps, a
    further SystemPlace of a group that was not listed (over `after_rows`,
    default the list), and one per-Select Select with Preempt of `tg` over the
    first rows of the list."""
    el = st.Eligibility()
    st.SetNodes(rows if after_rows is None else after_rows)
    sc, ss, p = st.SystemPlace(extra)
    st.SetNodes(rows[:16])
    r = st.SelectRaw(tg, SelectOptions(preempt=True))
    sel = (r.row, sorted(r.preempted), r.nodes_filtered, r.nodes_exhausted, r.final_score if r.row >= 0 else 0.0)
    return {"job": el["job"], "tgs": el["tgs"]}, (np.where(ss == 0, sc, np.nan).reshape(-1, 1), ss.reshape(-1, 1),
                                                  np.bincount(ss, minlength=3)[:3].reshape(1, 3), p), sel


def _same_select(a, b, rtol):
    assert a[:4] == b[:4]
    assert a[4] == b[4] if rtol == 0.0 else np.isclose(a[4], b[4], rtol=rtol, atol=0.0)


def _does_its_work(ro):
    """The oracle's result shows what the workload is for."""
    st, pre = ro[1], ro[4]
    cols = {k for (_, k) in pre}
    assert len(cols) >= 2                                  # evictions in at least two columns
    per_node = {}
    for (pos, _) in pre:
        per_node[pos] = per_node.get(pos, 0) + 1
    assert max(per_node.values()) >= 2                     # a node evicting in two groups
    assert (st == 2).any() and (st == 1).any()             # still exhausted entries, filtered entries
    assert all(st[pos, k] == 0 for (pos, k) in pre)


def _parity(nodes, allocs, job, rows, tgs, extra, oracle=None, cfg=PRE, staged=False, check=True, before=None,
            after_rows=None):
    """The batched call (a), the sequential calls (b) and the oracle loop (o),
    compared; returns the engine stacks and the results. `before`: run on
    each stack after its setup. `after_rows`: the list of the further
    SystemPlace (default: the call's)."""
    before = before or (lambda st: None)
    if oracle is None:
        o = _setup(OracleSystemStack(config=cfg), nodes, allocs, job, rows)
        before(o)
        ro = system_place_groups_preempt_by_select(o, tgs)
        eo, xo, so = _after(o, rows, extra, tgs[0], after_rows)
    else:
        ro, eo, xo, so = oracle
    if check:
        _does_its_work(ro)
    a = _setup(_engine(config=cfg), nodes, allocs, job, rows)
    b = _setup(_engine(config=cfg), nodes, allocs, job, rows)
    before(a)
    before(b)
    ra = a.SystemPlaceGroupsPreempt(tgs, fallback=False, staged=staged)
    rb = _sequential(b, tgs)
    _same_exact(ra, rb)
    _same_oracle(ra, ro)
    ea, xa, sa = _after(a, rows, extra, tgs[0], after_rows)
    eb, xb, sb = _after(b, rows, extra, tgs[0], after_rows)
    assert ea == eb == eo
    _same_exact(xa, xb)
    _same_oracle(xa, xo)
    _same_select(sa, sb, 0.0)
    _same_select(sa, so, 1e-12)
    return (a, b), ra, ro


GPU_TG, BIG, NET, EXTRA = 0, 1, 2, 3


def _groups():
    return [_tg("gpu", 500, mem=256, devices=[RequestedDevice("nvidia/gpu", 2)]),
            _tg("big", 7200, mem=14000),
            _tg("net", 1500, mem=2048, net=NetworkResource(mbits=50, dynamic_ports=1)),
            _tg("extra", 300, mem=128)]


@functools.lru_cache(maxsize=None)
def _c5(n, seed):
    nodes, allocs = synth.cluster_c5(n, seed=seed, busy=0.5)
    for a in allocs:
        a.max_parallel = 0   # no penalty that reads the plan's preemption counts
    return nodes, allocs, _sys_job(_groups())


@functools.lru_cache(maxsize=None)
def _c5_oracle(n, seed, list_seed, order, subset):
    """The oracle loop once per shape: results, eligibility, the further
    placement, the Select."""
    nodes, allocs, job = _c5(n, seed)
    rows = _c5_rows(n, list_seed, subset)
    o = _setup(OracleSystemStack(config=PRE), nodes, allocs, job, rows)
    ro = system_place_groups_preempt_by_select(o, list(order))
    return (ro,) + _after(o, rows, EXTRA, order[0])


def _c5_rows(n, list_seed, subset):
    perm = synth.shuffle(n, list_seed)
    return perm if subset is None else np.ascontiguousarray(perm[:subset])


SHAPES = {
    "300 gpu-big-net": (300, 9, 12, (GPU_TG, BIG, NET), [[175, 125, 0], [300, 0, 0], [210, 0, 90]], 250),
    "300 net-big-gpu": (300, 9, 12, (NET, BIG, GPU_TG), [[300, 0, 0], [247, 0, 53], [146, 125, 29]], 216),
    "600 gpu-big-net": (600, 4, 7, (GPU_TG, BIG, NET), [[348, 252, 0], [600, 0, 0], [436, 0, 164]], 483),
}


@gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_row_order_form(shape):
    """The full shuffled list (row-order kernel form)."""
    n, seed, list_seed, order, counts, evicting = SHAPES[shape]
    nodes, allocs, job = _c5(n, seed)
    ora = _c5_oracle(n, seed, list_seed, order, None)
    assert ora[0][2].tolist() == counts and len(ora[0][4]) == evicting
    _, ra, _ = _parity(nodes, allocs, job, _c5_rows(n, list_seed, None), list(order), EXTRA, oracle=ora)
    assert max(len(v) for v in ra[4].values()) >= 2


@gpu
def test_list_order_form():
    """60 rows of the 300: under a quarter of the snapshot, the list-order form."""
    nodes, allocs, job = _c5(300, 9)
    order = (GPU_TG, BIG, NET)
    _parity(nodes, allocs, job, _c5_rows(300, 12, 60), list(order), EXTRA, oracle=_c5_oracle(300, 9, 12, order, 60))


@gpu
def test_row_order_form_with_unlisted_rows():
    """150 of 300 rows listed: in the row-order form the unlisted rows are lanes
    without a node inside every wave of the stopping pass, which take part in
    the wave's ballots. The further SystemPlace runs over all 300 rows: the
    rows the call must not have touched are compared too."""
    nodes, allocs, job = _c5(300, 9)
    rows = _c5_rows(300, 12, 150)
    listed = np.zeros(300, dtype=bool)
    listed[rows] = True
    assert 4 * len(rows) >= 300   # the row-order form
    assert all(listed[w:w + 64].any() and not listed[w:w + 64].all() for w in range(0, 300, 64))
    _, _, ro = _parity(nodes, allocs, job, rows, [GPU_TG, BIG, NET], EXTRA, after_rows=np.arange(300, dtype=np.uint32))
    assert (ro[1] == 0).any() and (ro[1] == 2).any()   # placed and exhausted entries
    assert len(ro[4]) >= 1                             # and evicting ones


def _nine():
    nodes, allocs, _ = _c5(40, 6)
    g = _groups()
    small = [_tg("s%d" % k, 100 + 10 * k) for k in range(6)]
    # gpu first, six small groups, then net at index 7 and big at index 8, the first group of the second chunk
    job = _sys_job([g[GPU_TG]] + small + [g[NET], g[BIG], g[EXTRA]])
    return nodes, allocs, job


@gpu
def test_nine_groups_cross_a_chunk():
    """Evictions before and at group index 8: a node stopped in the first
    chunk of the stopping pass is skipped by the second, a node that walked
    through the first chunk may stop in the second."""
    nodes, allocs, job = _nine()
    rows = synth.shuffle(40, 2)
    _, ra, ro = _parity(nodes, allocs, job, rows, list(range(9)), 9)
    cols = {k for (_, k) in ro[4]}
    assert min(cols) < 8 and max(cols) >= 8
    first = {}
    for (pos, k) in ro[4]:
        first[pos] = min(first.get(pos, 99), k)
    assert 8 in first.values()   # a node whose first eviction is in the second chunk


def _wide():
    """Eight 8000-share nodes; node 3 holds 40 priority-20 allocs of 150
    shares, the others one of 6000 (node 6: priority 95, node 7: windows)."""
    ids = sorted(synth.uuids(8, 5))
    nodes = [synth.mock_node(i) for i in ids]
    for nd in nodes:
        nd.cpu_shares = 8000
    nodes[7].attributes["kernel.name"] = "windows"
    for nd in nodes:
        nd.compute_class()
    allocs = []
    for k, nd in enumerate(nodes):
        if k == 3:
            allocs += [Allocation(node_id=nd.id, job_id="many-%d" % (j % 5), task_group="tg", cpu_shares=150,
                                  memory_mb=32, disk_mb=10, priority=20) for j in range(40)]
        else:
            allocs.append(Allocation(node_id=nd.id, job_id="one", task_group="tg", cpu_shares=6000, memory_mb=64,
                                     disk_mb=10, priority=95 if k == 6 else 20))
    job = _sys_job([_tg("a", 3000), _tg("b", 2500), _tg("c", 2500), _tg("extra", 200)])
    return nodes, allocs, job


@gpu
def test_one_wide_node_takes_the_relaunch():
    """Node 3's 40 allocs are beyond the narrowest eviction width (32): the
    walk leaves it to a second launch at width 8; the other nodes' results
    come from the first."""
    nodes, allocs, job = _wide()
    rows = np.arange(8, dtype=np.uint32)
    _, ra, ro = _parity(nodes, allocs, job, rows, [0, 1, 2], 3)
    wide = [v for (pos, _), v in ro[4].items() if pos == 3]
    assert wide and sum(len(v) for v in wide) > 1        # the wide node evicts several of its allocs
    assert any(pos != 3 for (pos, _) in ro[4])
    # the relaunch itself, seen through the per-stage events: the fourth value is
    # the time from the first compaction to the end of the wider rounds, exactly 0
    # without one (the starting width covers all but an eighth of the snapshot's
    # nodes: here seven of eight)
    assert _wider_ms(nodes, allocs, job, rows, [0, 1, 2]) > 0.0
    nodes3, allocs3, job3 = _c5(300, 9)
    assert _wider_ms(nodes3, allocs3, job3, _c5_rows(300, 12, None), [GPU_TG, BIG, NET]) == 0.0


def _wider_ms(nodes, allocs, job, rows, tgs):
    st = _setup(_engine(config=PRE), nodes, allocs, job, rows)
    st._check(st._lib.pe_set_kernel_split(st._h, 1))
    st.SystemPlaceGroupsPreempt(tgs, fallback=False)
    ms4 = (C.c_double * 4)()
    st._check(st._lib.pe_last_kernel_split(st._h, C.cast(ms4, abi.f64p)))
    assert ms4[0] > 0.0 and ms4[1] > 0.0 and ms4[2] > 0.0
    return ms4[3]


@gpu
def test_a_long_plan_before_the_call():
    """More than 2048 placements in the plan before the call: the refusal of
    nodes beyond the widest eviction width then counts the plan's placements
    per node (none comes near the limit, the call goes ahead) and the
    eviction sees them as proposed allocs."""
    nodes, allocs = synth.cluster_c4(2999, seed=11)
    job = _sys_job([_tg("a", 300), _tg("big", 3500), _tg("b", 400), _tg("extra", 200), _tg("first", 50)])
    rows = synth.shuffle(2999, 5)
    placed = []

    def before(st):
        placed.append(st.SystemPlace(4)[2])

    _, ra, ro = _parity(nodes, allocs, job, rows, [0, 1, 2], 3, before=before, check=False)
    assert min(placed) > 2048 and len(set(placed)) == 1
    assert ro[4] and (ro[1] == 2).any() and (ro[1] == 1).any()


@gpu
def test_preemption_off_is_the_plain_call():
    nodes, allocs = synth.cluster_c4(2999, seed=11)
    web = synth.mock_system_job().task_groups[0]
    job = _sys_job([web, _tg("big", 3500), _tg("tiny", 150), _tg("extra", 300, mem=128)])
    rows = synth.shuffle(2999, 5)
    a = _setup(_engine(), nodes, allocs, job, rows)
    b = _setup(_engine(), nodes, allocs, job, rows)
    ra = a.SystemPlaceGroupsPreempt([0, 1, 2], fallback=False)
    rb = b.SystemPlaceGroups([0, 1, 2], fallback=False)
    _same_exact(ra, rb)
    assert ra[4] == {}
    ea, xa, sa = _after(a, rows, 3, 0)
    eb, xb, sb = _after(b, rows, 3, 0)
    assert ea == eb
    _same_exact(xa, xb)
    _same_select(sa, sb, 0.0)


@gpu
def test_edges():
    nodes, allocs, job = _c5(300, 9)
    rows = _c5_rows(300, 12, None)
    order = (GPU_TG, BIG, NET)
    # null arrays + pe_system_groups_results
    _parity(nodes, allocs, job, rows, list(order), EXTRA, oracle=_c5_oracle(300, 9, 12, order, None), staged=True)
    # one row (one that evicts), one group
    ro = _c5_oracle(300, 9, 12, order, None)[0]
    pos = sorted(ro[4])[0][0]
    _parity(nodes, allocs, job, rows[pos:pos + 1], list(order), EXTRA, check=False)
    _parity(nodes, allocs, job, rows, [BIG], EXTRA, check=False)
    # an empty list
    a = _setup(_engine(config=PRE), nodes, allocs, job, rows)
    a.SetNodes(np.zeros(0, dtype=np.uint32))
    sc, st, cn, p, pre = a.SystemPlaceGroupsPreempt([EXTRA], fallback=False)
    assert sc.shape == (0, 1) and st.shape == (0, 1) and cn.tolist() == [[0, 0, 0]] and p == 0 and pre == {}


@gpu
def test_reset_plan_then_again_equals_fresh():
    nodes, allocs, job = _c5(300, 9)
    rows = _c5_rows(300, 12, None)
    order = [GPU_TG, BIG, NET]
    a = _setup(_engine(config=PRE), nodes, allocs, job, rows)
    first = a.SystemPlaceGroupsPreempt(order, fallback=False)
    a.ResetPlan()
    a.SetJob(job)
    a.SetNodes(rows)
    again = a.SystemPlaceGroupsPreempt(order, fallback=False)
    _same_exact(first, again)
    assert first[4] == again[4]
    _same_oracle(again, _c5_oracle(300, 9, 12, tuple(order), None)[0])
    fresh = _setup(_engine(config=PRE), nodes, allocs, job, rows)
    _same_exact(again, fresh.SystemPlaceGroupsPreempt(order, fallback=False))
    ea, xa, sa = _after(a, rows, EXTRA, GPU_TG)
    ef, xf, sf = _after(fresh, rows, EXTRA, GPU_TG)
    assert ea == ef
    _same_exact(xa, xf)
    _same_select(sa, sf, 0.0)


@gpu
def test_stops_after_the_call():
    """StopAllocs / PopUpdate of snapshot allocs after the call, among them
    allocs the call preempted, then a further group: the batched handle, the
    sequential one and the oracle."""
    nodes, allocs, job = _c5(300, 9)
    rows = _c5_rows(300, 12, None)
    order = [GPU_TG, BIG, NET]
    out = []
    for kind in ("batched", "sequential", "oracle"):
        st = _setup(OracleSystemStack(config=PRE) if kind == "oracle" else _engine(config=PRE), nodes, allocs, job,
                    rows)
        if kind == "batched":
            r = st.SystemPlaceGroupsPreempt(order, fallback=False)
        elif kind == "sequential":
            r = _sequential(st, order)
        else:
            r = system_place_groups_preempt_by_select(st, order)
        pre = _c5_oracle(300, 9, 12, tuple(order), None)[0][4]
        taken = {a for v in pre.values() for a in v}
        stop = [i for i in range(len(allocs)) if i not in taken][:40]   # allocs the plan still holds
        st.StopAllocs(stop)
        st.PopUpdate(stop[-1])          # the last stop is taken back ...
        st.StopAllocs(stop[:1])         # ... and the first one repeated
        out.append((r, _after(st, rows, EXTRA, GPU_TG)))
    (ra, (ea, xa, sa)), (rb, (eb, xb, sb)), (ro, (eo, xo, so)) = out
    _same_exact(ra, rb)
    _same_oracle(ra, ro)
    assert ea == eb == eo
    _same_exact(xa, xb)
    _same_oracle(xa, xo)
    _same_select(sa, sb, 0.0)
    _same_select(sa, so, 1e-12)


def _refusal_cases():
    two_nic = NetworkResource(mode="host", device="eth1", cidr="10.9.9.9/32", ip="10.9.9.9", mbits=1000)
    dev = lambda c=1: [RequestedDevice("nvidia/gpu", c)]   # noqa: E731
    net = NetworkResource(mbits=10, dynamic_ports=1)
    static = NetworkResource(mode="host", reserved_ports=[8080], port_labels=["http"])
    dp = Constraint("${meta.database}", "", "distinct_property")
    return {
        "max_parallel candidate": dict(mp=True),
        "one device group twice in an alloc": dict(
            groups=[_tg("a", 100, devices=dev()), _tg("b", 3500)], alloc_devices=[(0, 1), (0, 1)]),
        "alloc device entries beyond the packed form": dict(alloc_devices=[(0, 300)]),
        # two task networks of 600 MBits on 1000-MBit nodes: the second needs PreemptForNetwork
        "several task networks": dict(groups=[TaskGroup(name="a", count=1, ephemeral_disk_mb=50, tasks=[
            Task(name="t1", driver="exec", cpu=50, memory_mb=32, network=NetworkResource(mbits=600, dynamic_ports=1)),
            Task(name="t2", driver="exec", cpu=50, memory_mb=32, network=NetworkResource(mbits=600, dynamic_ports=1))]),
            _tg("b", 3500)]),
        "duplicate rows": dict(rows=[0, 1, 1]),
        "job distinct_property": dict(job_cons=[dp]),
        "group distinct_property": dict(groups=[_tg("a", 100), _tg("b", 100, constraints=[dp])]),
        "reserved cores": dict(groups=[_tg("a", 100), _tg("b", 100, cores=1)]),
        "static ports": dict(groups=[_tg("a", 100, tg_net=static), _tg("b", 100)]),
        "multi-NIC task network": dict(groups=[_tg("a", 100, net=net), _tg("b", 100)], extra_net=two_nic),
        "devices in two groups": dict(groups=[_tg("a", 100, devices=dev()), _tg("b", 100, devices=dev())]),
        "metrics on": dict(metrics=True),
        "several devices": dict(devices=[0, 0]),
        "group unsupported": dict(groups=[_tg("a", 100), _tg("b", 100, devices=dev(300))]),
    }


SELECT_REFUSES = ("reserved cores", "one device group twice in an alloc",
                  "alloc device entries beyond the packed form", "several task networks")


@gpu
@pytest.mark.parametrize("case", sorted(_refusal_cases()))
def test_refusals_change_nothing(case):
    """Each refusal on a fresh pair of preempting handles: Unsupported without
    the fallback, a following per-group SystemPlace equal to a fresh
    handle's, and with the fallback the oracle loop's answer."""
    from nomad_amd.stack import Unsupported
    kw = _refusal_cases()[case]
    ids = sorted(synth.uuids(40, 17))
    nodes = [synth.nvidia_node(i) if k % 2 else synth.mock_node(i) for k, i in enumerate(ids)]
    if "extra_net" in kw:
        nodes[5].networks.append(kw["extra_net"])
        nodes[5].compute_class()
    # low-priority allocs that the second group (3500 of 3900) must evict
    allocs = [Allocation(node_id=nodes[k].id, job_id="low", task_group="tg", cpu_shares=1000, memory_mb=64, disk_mb=10,
                         priority=20) for k in range(0, 40, 3)]
    if kw.get("mp"):   # anywhere in the snapshot, on a node that is not even listed first
        allocs.append(Allocation(node_id=nodes[39].id, job_id="mp", task_group="tg", cpu_shares=10, memory_mb=8,
                                 disk_mb=1, priority=20, max_parallel=1))
    if "alloc_devices" in kw:   # on a GPU node (odd rows)
        allocs.append(Allocation(node_id=nodes[7].id, job_id="two-tasks", task_group="tg", cpu_shares=10, memory_mb=8,
                                 disk_mb=1, priority=20, devices=kw["alloc_devices"]))
    job = _sys_job(kw.get("groups", [_tg("a", 100), _tg("b", 3500)]), constraints=kw.get("job_cons", ()))
    rows = kw.get("rows", list(range(40)))

    def make(engine=True):
        if not engine:
            st = OracleSystemStack(config=PRE)
        elif "devices" in kw:
            st = _engine(config=PRE, devices=kw["devices"])
        else:
            st = _engine(config=PRE)
        _setup(st, nodes, allocs, job, rows)
        if kw.get("metrics"):
            st.EnableMetrics(True)
        return st

    def per_group(st):
        out = []
        for g in (0, 1):
            try:
                sc, ss, p = st.SystemPlace(g)
                out.append((sc.view(np.uint64)[ss == 0].tolist(), ss.tolist(), p))
            except Unsupported as e:   # the per-group call refuses the same job: also an answer
                out.append(("unsupported", e.code))
        return out

    a = make()
    with pytest.raises(Unsupported):
        a.SystemPlaceGroupsPreempt([0, 1], fallback=False)
    assert per_group(a) == per_group(make())   # nothing changed: a fresh handle gives the same
    if case in ("duplicate rows", "group unsupported"):
        return   # the per-Select loop over such a list / job is not this test's subject
    if case in SELECT_REFUSES:
        # the engine's own Select refuses this job or snapshot where it would evict, so the
        # wrapper's fallback, which is that Select in a loop, refuses too
        with pytest.raises(Unsupported):
            make().SystemPlaceGroupsPreempt([0, 1])
        return
    rf = make().SystemPlaceGroupsPreempt([0, 1])
    ro = system_place_groups_preempt_by_select(make(engine=False), [0, 1])
    _same_oracle(rf, ro)
    if case == "max_parallel candidate":
        assert ro[4]   # the fallback's answer carries the evictions


@gpu
def test_argument_errors():
    from nomad_amd.stack import EngineError, GenericStack
    nodes, allocs, job = _c5(300, 9)
    rows = np.arange(50, dtype=np.uint32)
    a = _setup(_engine(config=PRE), nodes, allocs, job, rows)
    en, of, al, ne = abi.u32p(), abi.u32p(), abi.u32p(), C.c_uint32(0)
    pre_args = (C.byref(en), C.byref(of), C.byref(al), C.byref(ne))
    assert a._lib.pe_system_groups_preempted(a._h, *pre_args) == abi.PE_ESTATE      # before any call
    fn = a._lib.pe_system_place_groups_preempt
    placed = C.c_uint32(7)
    t = np.array([0, 1], dtype=np.uint32)
    sc, st, cn = np.zeros(100), np.zeros(25, np.uint8), np.zeros(6, np.uint32)
    args = (sc.ctypes.data_as(abi.f64p), st.ctypes.data_as(abi.u8p), cn.ctypes.data_as(abi.u32p))
    tp = t.ctypes.data_as(abi.u32p)
    assert fn(a._h, tp, 0, *args, C.byref(placed)) == abi.PE_EINVAL                       # n_tg == 0
    assert fn(a._h, np.array([0, 4], np.uint32).ctypes.data_as(abi.u32p), 2, *args, C.byref(placed)) == abi.PE_EINVAL
    assert fn(a._h, np.array([1, 1], np.uint32).ctypes.data_as(abi.u32p), 2, *args, C.byref(placed)) == abi.PE_EINVAL
    assert fn(a._h, tp, 2, args[0], None, args[2], C.byref(placed)) == abi.PE_EINVAL      # mixed null / set
    assert fn(a._h, tp, 2, None, None, args[2], C.byref(placed)) == abi.PE_EINVAL
    assert a._lib.pe_system_groups_preempted(a._h, None, *pre_args[1:]) == abi.PE_EINVAL
    assert a._lib.pe_system_groups_preempted(a._h, *pre_args) == abi.PE_ESTATE      # the failed calls left none
    with pytest.raises(EngineError):
        a.SystemPlaceGroupsPreempt([0, 0], fallback=False)
    g = GenericStack()
    g.SetState(nodes, allocs)
    g.SetJob(job)
    g.SetNodes(rows)
    assert fn(g._h, tp, 2, *args, C.byref(placed)) == abi.PE_ESTATE                       # not a system stack
    # nothing changed on the system handle: the call now equals a fresh handle's
    fresh = _setup(_engine(config=PRE), nodes, allocs, job, rows)
    ra = a.SystemPlaceGroupsPreempt([0, 1], fallback=False)
    rf = fresh.SystemPlaceGroupsPreempt([0, 1], fallback=False)
    _same_exact(ra, rf)
    assert ra[4] == rf[4] and ra[4]
    # a pe_system_place since: the lists are gone
    a.SystemPlace(2)
    assert a._lib.pe_system_groups_preempted(a._h, *pre_args) == abi.PE_ESTATE
