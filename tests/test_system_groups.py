"""System jobs with several task groups in one pass (pe_system_place_groups).

SystemScheduler.computePlacements (scheduler_system.go:283-425) walks diff.place
node-major: for each node every required task group, in Go map order within
the node. The groups of one node are coupled (the first group's ask shrinks
what the second finds). The CPU part pins that coupling on the oracle with
the per-call helper; the GPU part compares the batched call with the helper on
the oracle (the node-major reference loop) and with sequential SystemPlace(g)
calls on a second engine handle: outcomes and counts equal, FinalScores
bit-equal between the engine handles and within 1e-12 relative of the oracle
(README), and the same for EvalEligibility and a further SystemPlace of a
group that was not listed.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from nomad_amd import abi, synth
from nomad_amd.stack import pack_status2, system_place_groups_by_select, unpack_status2
from nomad_amd.structs import (Allocation, Constraint, NetworkResource, RequestedDevice, SchedulerConfig, Task,
                               TaskGroup)
from oracle.oracle import OracleSystemStack

gpu = pytest.mark.gpu


# ---- CPU: the per-call helper on the oracle, and the packing ------------------

def _tg(name, cpu, mem=64, net=None, devices=(), constraints=(), tg_net=None, cores=0):
    return TaskGroup(name=name, count=1, ephemeral_disk_mb=50, constraints=list(constraints), network=tg_net,
                     tasks=[Task(name=name, driver="exec", cpu=cpu, memory_mb=mem, network=net,
                                 devices=list(devices), cores=cores)])


def _sys_job(groups, constraints=()):
    job = synth.mock_system_job("sys-groups")
    job.constraints = job.constraints + list(constraints)
    job.task_groups = list(groups)
    return job


def _hand_cluster():
    """both: fits a and b; first: a then b exhausted because of a; win:
    constraint-filtered; full: pre-filled."""
    ids = sorted(synth.uuids(4, 3))
    both, first, win, full = (synth.mock_node(i) for i in ids)
    both.cpu_shares = 8000
    win.attributes["kernel.name"] = "windows"
    for nd in (both, first, win, full):
        nd.compute_class()
    allocs = [Allocation(node_id=full.id, job_id="filler", task_group="tg", cpu_shares=3800, memory_mb=256,
                         disk_mb=100)]
    return [both, first, win, full], allocs


def _hand_run(order):
    nodes, allocs = _hand_cluster()
    job = _sys_job([_tg("a", 2000), _tg("b", 2500)])
    o = OracleSystemStack()
    o.SetState(nodes, allocs)
    o.SetJob(job)
    o.SetNodes(nodes)
    return system_place_groups_by_select(o, order)


def test_by_select_helper_on_the_oracle():
    score, status, counts, placed = _hand_run([0, 1])
    assert status.tolist() == [[0, 0], [0, 2], [1, 1], [2, 2]]
    assert counts.tolist() == [[2, 1, 1], [1, 1, 2]]
    assert placed == 3
    assert np.array_equal(np.isnan(score), status != 0)
    assert score.shape == (4, 2) and status.dtype == np.uint8


def test_group_order_matters():
    _, ab, _, _ = _hand_run([0, 1])
    _, ba, _, pb = _hand_run([1, 0])
    # columns follow the listed order: [1, 0] lists b first
    assert ba.tolist() == [[0, 0], [0, 2], [1, 1], [2, 2]]
    assert ab[1].tolist() == [0, 2] and ba[1, ::-1].tolist() == [2, 0]   # node `first`: (a, b) outcomes
    assert not np.array_equal(ab, ba[:, ::-1])
    assert pb == 3


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 8997])
def test_status2_round_trip(n):
    st = np.random.Generator(np.random.PCG64(n)).integers(0, 3, size=n).astype(np.uint8)
    packed = pack_status2(st)
    assert packed.dtype == np.uint8 and len(packed) == (n + 3) // 4
    assert np.array_equal(unpack_status2(packed, n), st)
    if n % 4:   # unused bits of the last byte are 0
        assert int(packed[-1]) >> (2 * (n % 4)) == 0


def test_status2_bit_positions():
    # entry e in byte e >> 2 at bits 2 * (e & 3)
    assert pack_status2([0, 1, 2, 0, 2]).tolist() == [(1 << 2) | (2 << 4), 2]
    assert unpack_status2(np.array([0b10_01_00_10, 0b01], dtype=np.uint8), 5).tolist() == [2, 0, 1, 2, 1]


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


def _setup(st, nodes, allocs, job, rows):
    st.SetState(nodes, allocs)
    st.SetJob(job)
    st.SetNodes(rows)
    return st


def _after(st, rows, extra):
    """What the tests compare after the placements: the eligibility maps and
    a further SystemPlace of a group that was not listed."""
    el = st.Eligibility()
    st.SetNodes(rows)
    sc, ss, p = st.SystemPlace(extra)
    return {"job": el["job"], "tgs": el["tgs"]}, (np.where(ss == 0, sc, np.nan).reshape(-1, 1), ss.reshape(-1, 1),
                                                  np.bincount(ss, minlength=3)[:3].reshape(1, 3), p)


def _parity(nodes, allocs, job, rows, tgs, extra, oracle=None, cfg=None, after_rows=None):
    """The batched call (a), the sequential calls (b) and the oracle loop (o),
    compared; returns the three stacks' results. `after_rows`: the list of the
    further SystemPlace (default: the call's)."""
    after_rows = rows if after_rows is None else after_rows
    a = _setup(_engine(config=cfg), nodes, allocs, job, rows)
    b = _setup(_engine(config=cfg), nodes, allocs, job, rows)
    ra = a.SystemPlaceGroups(tgs, fallback=False)
    rb = _sequential(b, tgs)
    if oracle is None:
        o = _setup(OracleSystemStack(config=cfg), nodes, allocs, job, rows)
        ro = system_place_groups_by_select(o, tgs)
        eo, xo = _after(o, after_rows, extra)
    else:
        ro, eo, xo = oracle
    _same_exact(ra, rb)
    _same_oracle(ra, ro)
    ea, xa = _after(a, after_rows, extra)
    eb, xb = _after(b, after_rows, extra)
    assert ea == eb == eo
    _same_exact(xa, xb)
    _same_oracle(xa, xo)
    return (a, b), ra, ro


N4 = 2999
WEB, BIG, TINY, EXTRA = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def _c4():
    nodes, allocs = synth.cluster_c4(N4, seed=11)
    web = synth.mock_system_job().task_groups[0]                    # task network: 50 MBits + 1 dynamic port
    # big fits an empty 4000-share node (3900 free) but not after web's 500; tiny
    # does not fit a pre-filled node (100 free)
    job = _sys_job([web, _tg("big", 3500), _tg("tiny", 150), _tg("extra", 300, mem=128)])
    return nodes, allocs, job


@functools.lru_cache(maxsize=None)
def _c4_oracle(order, subset):
    """The oracle loop once per (group order, list): results, eligibility, the
    further placement."""
    nodes, allocs, job = _c4()
    rows = _c4_rows(subset)
    o = _setup(OracleSystemStack(), nodes, allocs, job, rows)
    ro = system_place_groups_by_select(o, list(order))
    eo, xo = _after(o, rows, EXTRA)
    return ro, eo, xo


def _c4_rows(subset):
    perm = synth.shuffle(N4, 5)
    return perm if subset is None else np.ascontiguousarray(perm[:subset])


@gpu
def test_row_order_form():
    """The full shuffled list (row-order kernel form): 2999 x 3 = 8997 entries,
    no multiple of 4, 64 or 256."""
    nodes, allocs, job = _c4()
    order = (WEB, BIG, TINY)
    ora = _c4_oracle(order, None)
    st = ora[0][1]
    for k in range(3):   # every outcome in every group
        assert set(np.unique(st[:, k])) == {0, 1, 2}, k
    rows = _c4_rows(None)
    small = np.array([nodes[int(r)].cpu_shares == 4000 for r in rows])
    coupled = small & (st[:, 0] == 0) & (st[:, 1] == 2)
    assert coupled.any()   # big exhausted only because web was placed (3500 <= 3900 free)
    _parity(nodes, allocs, job, rows, list(order), EXTRA, oracle=ora)


@gpu
def test_list_order_form():
    """A 500-row subset: under a quarter of the snapshot, the list-order form."""
    nodes, allocs, job = _c4()
    order = (WEB, BIG, TINY)
    _parity(nodes, allocs, job, _c4_rows(500), list(order), EXTRA, oracle=_c4_oracle(order, 500))


def _half_listed(n, seed):
    """Half of an n-row snapshot, shuffled: 4 * len >= n takes the row-order
    form, and every wave of 64 rows holds rows that are not listed."""
    rows = np.ascontiguousarray(synth.shuffle(n, seed)[:n // 2])
    listed = np.zeros(n, dtype=bool)
    listed[rows] = True
    assert all(listed[w:w + 64].any() and not listed[w:w + 64].all() for w in range(0, n, 64))
    return rows


@gpu
def test_row_order_form_with_unlisted_rows():
    """150 of 300 rows listed: in the row-order form the unlisted rows are lanes
    without a node inside every wave, which take part in the wave's ballots.
    The further SystemPlace runs over all 300 rows: the rows the call must not
    have touched are compared too."""
    nodes, allocs = synth.cluster_c4(300, seed=11)
    job = _c4()[2]
    rows = _half_listed(300, 7)
    _, _, ro = _parity(nodes, allocs, job, rows, [WEB, BIG, TINY], EXTRA,
                       after_rows=np.arange(300, dtype=np.uint32))
    assert (ro[1] == 0).any() and (ro[1] == 2).any()   # placed and exhausted entries


@gpu
def test_group_order_changes_the_answer():
    nodes, allocs, job = _c4()
    first = _c4_oracle((WEB, BIG, TINY), None)[0][1]
    order = (BIG, WEB, TINY)
    ora = _c4_oracle(order, None)
    rows = _c4_rows(None)
    _, ra, _ = _parity(nodes, allocs, job, rows, list(order), EXTRA, oracle=ora)
    small = np.array([nodes[int(r)].cpu_shares == 4000 for r in rows])
    coupled = small & (first[:, 0] == 0) & (first[:, 1] == 2)
    # on those nodes big now comes first and is placed, and web no longer fits
    assert (ra[1][coupled, 0] == 0).all() and (ra[1][coupled, 1] == 2).all()


@gpu
def test_distinct_hosts_and_ineligible_class():
    """Job-level distinct_hosts on a system job, and a group constraint that
    makes one class ineligible. NewSystemStack (stack.go:207-283) has no
    DistinctHostsIterator: the reference places the second group beside the
    first, and so do all three runs here."""
    nodes, allocs = synth.cluster_c4(700, seed=3)
    for k, nd in enumerate(nodes):
        nd.meta["tier"] = "gold" if k % 3 == 0 else "plain"
        nd.compute_class()
    job = _sys_job([_tg("a", 400), _tg("b", 300, constraints=[Constraint("${meta.tier}", "gold", "=")]),
                    _tg("extra", 200)], constraints=[Constraint("", "", "distinct_hosts")])
    rows = synth.shuffle(700, 9)
    (a, _), ra, ro = _parity(nodes, allocs, job, rows, [0, 1], 2)
    both = (ro[1][:, 0] == 0) & (ro[1][:, 1] == 0)
    assert both.any()   # the reference's system stack does not filter the second group
    plain = np.array([nodes[int(r)].meta["tier"] == "plain" for r in rows])
    assert (ra[1][plain, 1] == 1).all()
    classes = a.GetClasses(a.Eligibility())
    assert True in classes.values() and False in classes.values()


@gpu
@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_devices_in_one_group(order):
    ids = sorted(synth.uuids(300, 21))
    nodes = [synth.nvidia_node(i, healthy=1 + k % 3) if k % 2 else synth.mock_node(i) for k, i in enumerate(ids)]
    allocs = [Allocation(node_id=nodes[k].id, job_id="held", task_group="tg", cpu_shares=200, memory_mb=64,
                         disk_mb=10, devices=[(0, 1)]) for k in range(1, 300, 8)]
    job = _sys_job([_tg("gpu", 300, devices=[RequestedDevice("nvidia/gpu", 2)]), _tg("plain", 3500),
                    _tg("extra", 100, devices=[RequestedDevice("nvidia/gpu", 1)])])
    _, ra, _ = _parity(nodes, allocs, job, synth.shuffle(300, 2), list(order), 2)
    k = order.index(0)
    assert {0, 2} <= set(np.unique(ra[1][:, k]))


@gpu
def test_dynamic_ports_and_bandwidth():
    """Three groups of 50 MBits on nodes whose bandwidth admits two."""
    nodes, allocs = synth.cluster_c4(400, seed=8)
    for k, nd in enumerate(nodes):
        nd.networks[0].mbits = 100 if k % 2 else 1000
    net = lambda: NetworkResource(mbits=50, dynamic_ports=1)   # noqa: E731
    job = _sys_job([_tg("n0", 20, net=net()), _tg("n1", 20, net=net()), _tg("n2", 20, net=net()),
                    _tg("extra", 20, net=net())])
    rows = synth.shuffle(400, 4)
    _, ra, _ = _parity(nodes, allocs, job, rows, [0, 1, 2], 3)
    narrow = np.array([nodes[int(r)].networks[0].mbits == 100 for r in rows]) & (ra[1][:, 0] == 0)
    assert narrow.any() and (ra[1][narrow, 1] == 0).all() and (ra[1][narrow, 2] == 2).all()


@gpu
def test_edges():
    nodes, allocs, job = _c4()
    rows = _c4_rows(None)
    # one row
    _parity(nodes, allocs, job, rows[:1], [WEB, BIG, TINY], EXTRA)
    # one group: SystemPlace, unpacked
    a = _setup(_engine(), nodes, allocs, job, rows)
    b = _setup(_engine(), nodes, allocs, job, rows)
    ra = a.SystemPlaceGroups([BIG], fallback=False)
    _same_exact(ra, _sequential(b, [BIG]))
    # null arrays + pe_system_groups_results, on the state the call above left
    rs = a.SystemPlaceGroups([WEB, TINY], fallback=False, staged=True)
    _same_exact(rs, _sequential(b, [WEB, TINY]))
    # an empty list
    a.SetNodes(np.zeros(0, dtype=np.uint32))
    sc, st, cn, p = a.SystemPlaceGroups([EXTRA], fallback=False)
    assert sc.shape == (0, 1) and st.shape == (0, 1) and cn.tolist() == [[0, 0, 0]] and p == 0


@gpu
def test_nine_groups_cross_a_chunk():
    nodes, allocs = synth.cluster_c4(600, seed=2)
    job = _sys_job([_tg("g%d" % k, 450 + 10 * k) for k in range(9)] + [_tg("extra", 100)])
    _, ra, _ = _parity(nodes, allocs, job, synth.shuffle(600, 1), list(range(9)), 9)
    assert {0, 2} <= set(np.unique(ra[1][:, 8]))   # 4000-share nodes run out before the ninth group


@gpu
def test_reset_plan_then_again_equals_fresh():
    nodes, allocs, job = _c4()
    rows = _c4_rows(500)
    a = _setup(_engine(), nodes, allocs, job, rows)
    first = a.SystemPlaceGroups([WEB, BIG, TINY], fallback=False)
    a.ResetPlan()
    a.SetJob(job)
    a.SetNodes(rows)
    again = a.SystemPlaceGroups([WEB, BIG, TINY], fallback=False)
    _same_exact(first, again)
    _same_oracle(again, _c4_oracle((WEB, BIG, TINY), 500)[0])
    fresh = _setup(_engine(), nodes, allocs, job, rows)
    _same_exact(again, fresh.SystemPlaceGroups([WEB, BIG, TINY], fallback=False))
    ea, xa = _after(a, rows, EXTRA)
    ef, xf = _after(fresh, rows, EXTRA)
    assert ea == ef
    _same_exact(xa, xf)


@gpu
def test_stops_after_the_call():
    """PopUpdate / StopAllocs of a snapshot alloc on a placed node, then a
    further group: the batched handle, the sequential one and the oracle."""
    nodes, allocs = synth.cluster_c4(500, seed=6)
    held = [k for k in range(0, 500, 7) if nodes[k].attributes["kernel.name"] == "linux"]
    base = len(allocs)
    allocs = allocs + [Allocation(node_id=nodes[k].id, job_id="old", task_group="tg", cpu_shares=3000, memory_mb=128,
                                  disk_mb=10) for k in held]
    job = _sys_job([_tg("a", 300), _tg("b", 400), _tg("extra", 2500)])
    rows = synth.shuffle(500, 3)
    out = []
    for kind in ("batched", "sequential", "oracle"):
        st = _setup(OracleSystemStack() if kind == "oracle" else _engine(), nodes, allocs, job, rows)
        if kind == "batched":
            r = st.SystemPlaceGroups([0, 1], fallback=False)
        elif kind == "sequential":
            r = _sequential(st, [0, 1])
        else:
            r = system_place_groups_by_select(st, [0, 1])
        stop = list(range(base, base + len(held)))
        st.StopAllocs(stop)
        st.PopUpdate(stop[-1])          # the last stop is taken back ...
        st.StopAllocs(stop[:1])         # ... and the first one repeated
        out.append((r, _after(st, rows, 2)))
    (ra, (ea, xa)), (rb, (eb, xb)), (ro, (eo, xo)) = out
    _same_exact(ra, rb)
    _same_oracle(ra, ro)
    assert ea == eb == eo
    _same_exact(xa, xb)
    _same_oracle(xa, xo)
    at = {int(r): i for i, r in enumerate(rows)}
    filled = {x.node_id for x in allocs[:base]}
    freed = [k for k in held[1:-1] if nodes[k].id not in filled]
    assert freed and all(xa[1][at[k], 0] == 0 for k in freed)   # extra (2500) fits where a stop freed 3000


def _sys_view(e):
    fn = e._lib.pe_system_view_get
    fn.restype = C.POINTER(abi.pe_system_view)
    fn.argtypes = [C.c_void_p]
    return fn(e._h).contents


@gpu
def test_call_with_a_served_view_log():
    """The caller serves SetNodes([row]) + Select + Commit triples of group 0
    from the system view and logs them (tests/test_system_dropin.py's
    protocol); the batched call then takes the log over and equals the
    sequence in which those triples crossed the ABI."""
    nodes, allocs, job = _c4()
    n_served = 400
    a = _setup(_engine(), nodes, allocs, job, np.arange(N4, dtype=np.uint32))
    b = _setup(_engine(), nodes, allocs, job, np.arange(N4, dtype=np.uint32))
    o = _setup(OracleSystemStack(), nodes, allocs, job, np.arange(N4, dtype=np.uint32))

    def triple(st, r):
        st.SetNodes([r])
        x = st.Select(WEB)
        if x is not None:
            st.Commit(WEB, x.row)
        return None if x is None else (x.row, x.final_score)

    v = _sys_view(a)
    got = [triple(a, r) for r in range(3)]   # the first starts the cache pass
    assert v.n_rows == N4 and v.tg_index == WEB
    for r in range(3, n_served):
        bits = v.outcome[r]
        nan = (bits & 0x7FF8000000000000) == 0x7FF8000000000000
        code = bits & 3 if nan else 0
        assert code != 3 and v.n_log < v.log_cap
        if code:
            v.log[v.n_log] = r | abi.PE_SYS_NIL
            got.append(None)
        else:
            v.log[v.n_log] = r | abi.PE_SYS_COMMITTED
            v.outcome[r] = abi.PE_SYS_STALE
            got.append((r, C.c_double.from_buffer_copy(C.c_uint64(bits)).value))
        v.n_log += 1
    assert v.n_log == n_served - 3   # the log is not empty when the call comes
    ra = a.SystemPlaceGroups([BIG, TINY], fallback=False)   # on the list the last triple left: its one row
    assert [triple(b, r) for r in range(n_served)] == got
    rb = _sequential(b, [BIG, TINY])
    want = [triple(o, r) for r in range(n_served)]
    assert [x and x[0] for x in want] == [x and x[0] for x in got]
    ro = system_place_groups_by_select(o, [BIG, TINY])
    assert ra[1].shape == (1, 2)
    _same_exact(ra, rb)
    _same_oracle(ra, ro)
    rows = synth.shuffle(N4, 5)
    (ea, xa), (eb, xb), (eo, xo) = (_after(st, rows, EXTRA) for st in (a, b, o))
    assert ea == eb == eo
    _same_exact(xa, xb)
    _same_oracle(xa, xo)


def _refusal_cases():
    two_nic = NetworkResource(mode="host", device="eth1", cidr="10.9.9.9/32", ip="10.9.9.9", mbits=1000)
    dev = lambda c=1: [RequestedDevice("nvidia/gpu", c)]   # noqa: E731
    net = NetworkResource(mbits=10, dynamic_ports=1)
    static = NetworkResource(mode="host", reserved_ports=[8080], port_labels=["http"])
    dp = Constraint("${meta.database}", "", "distinct_property")
    return {
        "duplicate rows": dict(rows=[0, 1, 1]),
        "preemption": dict(cfg=SchedulerConfig(preempt_system=True)),
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


@gpu
@pytest.mark.parametrize("case", sorted(_refusal_cases()))
def test_refusals_change_nothing(case):
    from nomad_amd.stack import Unsupported
    kw = _refusal_cases()[case]
    ids = sorted(synth.uuids(40, 17))
    nodes = [synth.nvidia_node(i) if k % 2 else synth.mock_node(i) for k, i in enumerate(ids)]
    if "extra_net" in kw:
        nodes[5].networks.append(kw["extra_net"])
        nodes[5].compute_class()
    job = _sys_job(kw.get("groups", [_tg("a", 100), _tg("b", 3500)]), constraints=kw.get("job_cons", ()))
    rows = kw.get("rows", list(range(40)))
    cfg = kw.get("cfg")

    def make(engine=True):
        if not engine:
            st = OracleSystemStack(config=cfg)
        elif "devices" in kw:
            st = _engine(config=cfg, devices=kw["devices"])
        else:
            st = _engine(config=cfg)
        _setup(st, nodes, [], job, rows)
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
        a.SystemPlaceGroups([0, 1], fallback=False)
    assert per_group(a) == per_group(make())   # nothing changed: a fresh handle gives the same
    if case in ("duplicate rows", "group unsupported"):
        return   # the per-Select loop over such a list / job is not this test's subject
    # fallback=True: the wrapper's answer is the per-Select loop, equal to the oracle's
    rf = make().SystemPlaceGroups([0, 1])
    ro = system_place_groups_by_select(make(engine=False), [0, 1])
    _same_oracle(rf, ro)


@gpu
def test_argument_errors():
    from nomad_amd.stack import EngineError, GenericStack
    nodes, allocs = synth.cluster_c4(50, seed=1)
    job = _sys_job([_tg("a", 100), _tg("b", 3500)])
    a = _setup(_engine(), nodes, allocs, job, np.arange(50, dtype=np.uint32))
    fn = a._lib.pe_system_place_groups
    placed = C.c_uint32(7)
    t = np.array([0, 1], dtype=np.uint32)
    sc, st, cn = np.zeros(100), np.zeros(25, np.uint8), np.zeros(6, np.uint32)
    args = (sc.ctypes.data_as(abi.f64p), st.ctypes.data_as(abi.u8p), cn.ctypes.data_as(abi.u32p))
    tp = t.ctypes.data_as(abi.u32p)
    assert fn(a._h, tp, 0, *args, C.byref(placed)) == abi.PE_EINVAL                       # n_tg == 0
    assert fn(a._h, np.array([0, 2], np.uint32).ctypes.data_as(abi.u32p), 2, *args, C.byref(placed)) == abi.PE_EINVAL
    assert fn(a._h, np.array([1, 1], np.uint32).ctypes.data_as(abi.u32p), 2, *args, C.byref(placed)) == abi.PE_EINVAL
    assert fn(a._h, tp, 2, args[0], None, args[2], C.byref(placed)) == abi.PE_EINVAL      # mixed null / set
    assert fn(a._h, tp, 2, None, None, args[2], C.byref(placed)) == abi.PE_EINVAL
    with pytest.raises(EngineError):
        a.SystemPlaceGroups([0, 0], fallback=False)
    g = GenericStack()
    g.SetState(nodes, allocs)
    g.SetJob(job)
    g.SetNodes(np.arange(50, dtype=np.uint32))
    assert fn(g._h, tp, 2, *args, C.byref(placed)) == abi.PE_ESTATE                       # not a system stack
    # nothing changed on the system handle: the call now equals a fresh handle's
    fresh = _setup(_engine(), nodes, allocs, job, np.arange(50, dtype=np.uint32))
    _same_exact(a.SystemPlaceGroups([0, 1], fallback=False), fresh.SystemPlaceGroups([0, 1], fallback=False))
