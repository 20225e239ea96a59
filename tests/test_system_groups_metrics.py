"""Multi-group system placement with AllocMetric on (pe_system_place_groups_metrics).

SystemScheduler.computePlacements (scheduler_system.go:283-425) keeps little of
each single-node Select's maps: the first exhausted Select of a task group whole
(failedTGAllocs), the later ones as a count, and the ScoreMetaData of a placed
one. The CPU part pins the per-Select reference loop that collects exactly that
(system_place_groups_metrics_by_select) on the oracle with hand-built nodes and
hand-derived answers. The GPU part compares the batched call (a) with that loop
on the oracle and (b) with that loop on a second engine handle with metrics on:
positions, dimension and node class strings, outcomes, counts and preempted
allocs equal; scores bit-equal between engine handles and within 1e-12 relative
of the oracle (README). Outcomes, FinalScores, counts and preempted allocs are
also bit-equal to SystemPlaceGroupsPreempt on a third handle with metrics off.
Every listed group is compared in every test (the `failed` maps are compared
whole, and a group without an item has no exhausted entry on any side).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from nomad_amd import abi, synth
from nomad_amd.stack import system_place_groups_metrics_by_select
from nomad_amd.structs import (Affinity, Allocation, Constraint, NetworkResource, RequestedDevice, SchedulerConfig,
                               Task, TaskGroup)
from oracle.oracle import OracleSystemStack

gpu = pytest.mark.gpu

PRE = SchedulerConfig(preempt_system=True)
PLAIN = SchedulerConfig()
BANDWIDTH = "network: bandwidth exceeded"
NO_MATCH = "devices: no devices match request"


def _tg(name, cpu, mem=64, net=None, devices=(), constraints=(), tg_net=None, cores=0, disk=50):
    return TaskGroup(name=name, count=1, ephemeral_disk_mb=disk, constraints=list(constraints), network=tg_net,
                     tasks=[Task(name=name, driver="exec", cpu=cpu, memory_mb=mem, network=net,
                                 devices=list(devices), cores=cores)])


def _net50():
    return NetworkResource(mbits=50, dynamic_ports=1)


def _sys_job(groups, constraints=()):
    job = synth.mock_system_job("sys-groups-metrics")   # priority 100
    job.constraints = job.constraints + list(constraints)
    job.task_groups = list(groups)
    return job


def _setup(st, nodes, allocs, job, rows, metrics=True):
    st.SetState(nodes, allocs)
    st.SetJob(job)
    st.SetNodes(rows)
    if metrics:
        st.EnableMetrics(True)
    return st


# ---- CPU: the per-Select loop on the oracle, hand-derived answers -------------

def _hand_plain():
    """n0: 3900 free shares, a (2000) fits and b (2500) then does not, c (500)
    does; n1: windows, constraint-filtered; n2: 15900 free shares but a 100-MBit
    NIC under three 50-MBit asks; n3: everything fits, no NodeClass."""
    ids = sorted(synth.uuids(4, 3))
    n0, n1, n2, n3 = (synth.mock_node(i) for i in ids)
    n1.attributes["kernel.name"] = "windows"
    n2.cpu_shares = n3.cpu_shares = 16000
    n2.networks[0].mbits = 100
    n2.node_class = "narrow"
    n3.node_class = ""
    for nd in (n0, n1, n2, n3):
        nd.compute_class()
    job = _sys_job([_tg("a", 2000, net=_net50()), _tg("b", 2500, net=_net50()), _tg("c", 500, net=_net50())])
    return [n0, n1, n2, n3], job


def test_by_select_helper_on_the_oracle_plain_stack():
    nodes, job = _hand_plain()
    o = _setup(OracleSystemStack(), nodes, [], job, nodes)
    score, status, counts, placed, pre, m = system_place_groups_metrics_by_select(o, [0, 1, 2])
    assert status.tolist() == [[0, 2, 0], [1, 1, 1], [0, 0, 2], [0, 0, 0]]
    assert counts.tolist() == [[3, 1, 0], [2, 1, 1], [2, 1, 1]] and placed == 7 and pre == {}
    # a never fails; b fails on n0 only because a was placed there (2000 + 2500 > 3900, b alone fits);
    # c's first failure is the third 50-MBit ask on the 100-MBit node; the filtered node reports nothing
    assert m["failed"] == {1: (0, "cpu", "linux-medium-pci"), 2: (2, BANDWIDTH, "narrow")}
    assert set(m["scores"]) == {(p, k) for p in range(4) for k in range(3) if status[p, k] == 0}
    for (p, k), named in m["scores"].items():
        assert named == {"binpack": score[p, k]}   # the SystemStack ranks with BinPack alone
    # b alone fits on n0
    o = _setup(OracleSystemStack(), nodes, [], job, nodes)
    assert system_place_groups_metrics_by_select(o, [1])[1][0, 0] == 0
    # the other group order: c and b fit on n0 and a (listed third) does not; on n2 a is the third ask
    o = _setup(OracleSystemStack(), nodes, [], job, nodes)
    _, status, counts, _, _, m = system_place_groups_metrics_by_select(o, [2, 1, 0])
    assert status.tolist() == [[0, 0, 2], [1, 1, 1], [0, 0, 2], [0, 0, 0]]
    assert m["failed"] == {2: (0, "cpu", "linux-medium-pci")} and counts[2].tolist() == [1, 1, 2]
    # a node without a NodeClass reports no ClassExhausted key
    o = _setup(OracleSystemStack(), nodes, [], _sys_job([_tg("huge", 15950)]), nodes[3:])
    assert system_place_groups_metrics_by_select(o, [0])[5]["failed"] == {0: (0, "cpu", None)}


def _hand_preempting():
    """evict: a's 1000 does not fit beside x (7000 of 7900) and evicts it;
    stuck: the only alloc is priority 95 (less than 10 below the job's 100),
    eviction cannot help and both groups stay exhausted; free: everything fits."""
    ids = sorted(synth.uuids(3, 3))
    evict, stuck, free = (synth.mock_node(i) for i in ids)
    evict.cpu_shares = 8000
    stuck.node_class = "held"
    for nd in (evict, stuck, free):
        nd.compute_class()
    allocs = [Allocation(node_id=evict.id, job_id="low", task_group="tg", cpu_shares=7000, memory_mb=64, disk_mb=10,
                         priority=20),
              Allocation(node_id=stuck.id, job_id="high", task_group="tg", cpu_shares=3000, memory_mb=7000,
                         disk_mb=10, priority=95)]   # 900 shares and 936 MB free
    return [free, evict, stuck], allocs, _sys_job([_tg("a", 1000, mem=500), _tg("b", 500, mem=1000)])


def test_by_select_helper_on_the_oracle_preempting_stack():
    nodes, allocs, job = _hand_preempting()
    o = _setup(OracleSystemStack(config=PRE), nodes, allocs, job, nodes)
    score, status, counts, placed, pre, m = system_place_groups_metrics_by_select(o, [0, 1])
    assert status.tolist() == [[0, 0], [0, 0], [2, 2]] and placed == 4
    assert pre == {(1, 0): [0]}
    # after evict: a's 1000 shares do not fit in 900; b's 500 do but its 1000 MB do not fit in 936
    assert m["failed"] == {0: (2, "cpu", "held"), 1: (2, "memory", "held")}
    assert m["scores"][(1, 0)] == {"binpack": score[1, 0]}   # the entry placed by eviction
    # the other order on the stuck node: b still fails on memory, a on cpu
    o = _setup(OracleSystemStack(config=PRE), nodes, allocs, job, nodes)
    assert system_place_groups_metrics_by_select(o, [1, 0])[5]["failed"] == {0: (2, "memory", "held"),
                                                                             1: (2, "cpu", "held")}
    # without preemption the evicting entry is a's first failure instead
    o = _setup(OracleSystemStack(), nodes, allocs, job, nodes)
    _, status, _, _, pre, m = system_place_groups_metrics_by_select(o, [0, 1])
    assert status.tolist() == [[0, 0], [2, 0], [2, 2]] and pre == {}
    assert m["failed"] == {0: (1, "cpu", "linux-medium-pci"), 1: (2, "memory", "held")}


# ---- GPU ----------------------------------------------------------------------

def _engine(**kw):
    from nomad_amd.stack import SystemStack
    return SystemStack(**kw)


def _same_exact(a, b):
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[2], b[2])
    assert a[3] == b[3]
    assert np.array_equal(a[0].view(np.uint64)[a[1] == 0], b[0].view(np.uint64)[b[1] == 0])   # bit-equal
    assert np.isnan(a[0][a[1] != 0]).all() and np.isnan(b[0][b[1] != 0]).all()
    assert a[4] == b[4]   # the preempted allocs of every evicting entry


def _same_oracle(a, o):
    assert np.array_equal(a[1], o[1])
    assert np.array_equal(a[2], o[2])
    assert a[3] == o[3]
    m = a[1] == 0
    assert np.allclose(a[0][m], o[0][m], rtol=1e-12, atol=0.0)
    assert a[4] == o[4]


def _same_metrics(ra, rb, ro, dev_k):
    """The batched call's maps against the helper's on the engine (exact) and on
    the oracle (strings and positions equal, scores within 1e-12)."""
    ma, mb, mo = ra[5], rb[5], ro[5]
    assert ma["failed"] == mb["failed"] == mo["failed"]
    for k, (pos, _, _) in ma["failed"].items():   # the first exhausted entry of the final outcome
        assert pos == int(np.flatnonzero(ra[1][:, k] == 2)[0])
    assert set(ma["failed"]) == {k for k in range(ra[1].shape[1]) if (ra[1][:, k] == 2).any()}
    want = set() if dev_k is None else {(int(p), dev_k) for p in np.flatnonzero(ra[1][:, dev_k] == 0)}
    assert set(ma["scores"]) == want
    for key, named in ma["scores"].items():
        assert set(named) == {"binpack", "devices"} == set(mb["scores"][key]) == set(mo["scores"][key])
        for name in named:
            assert np.float64(named[name]).view(np.uint64) == np.float64(mb["scores"][key][name]).view(np.uint64)
            assert np.isclose(named[name], mo["scores"][key][name], rtol=1e-12, atol=0.0)
        if key not in ra[4]:   # the NormScore of the two is the FinalScore (an eviction's may hold the preemption score)
            assert (named["binpack"] + named["devices"]) / 2.0 == ra[0][key]
    # the other groups' only score is binpack = FinalScore, on the helper's side too
    for key, named in mb["scores"].items():
        if key[1] != dev_k:
            assert named == {"binpack": rb[0][key]}


def _after(st, rows, extra):
    """Later observable state: the eligibility maps and a further SystemPlace
    of a group that was not listed."""
    el = st.Eligibility()
    st.SetNodes(rows)
    sc, ss, p = st.SystemPlace(extra)
    return {"job": el["job"], "tgs": el["tgs"]}, (np.where(ss == 0, sc, np.nan).reshape(-1, 1), ss.reshape(-1, 1),
                                                  np.bincount(ss, minlength=3)[:3].reshape(1, 3), p, {})


def _oracle_run(nodes, allocs, job, rows, tgs, cfg, extra, after_rows=None):
    o = _setup(OracleSystemStack(config=cfg), nodes, allocs, job, rows)
    ro = system_place_groups_metrics_by_select(o, list(tgs))
    after_rows = rows if after_rows is None else after_rows
    return (ro,) + (_after(o, after_rows, extra) if extra is not None else (None, None))


def _parity(nodes, allocs, job, rows, tgs, cfg=PLAIN, dev_k=None, extra=None, oracle=None, staged=False,
            after_rows=None):
    """The batched call with metrics on (a), the helper on a second engine
    handle with metrics on (b) and on the oracle (o), SystemPlaceGroupsPreempt
    on a third handle with metrics off (c). `after_rows`: the list of the
    further SystemPlace (default: the call's)."""
    tgs = list(tgs)
    after_rows = rows if after_rows is None else after_rows
    ro, eo, xo = oracle if oracle is not None else _oracle_run(nodes, allocs, job, rows, tgs, cfg, extra, after_rows)
    a = _setup(_engine(config=cfg), nodes, allocs, job, rows)
    b = _setup(_engine(config=cfg), nodes, allocs, job, rows)
    c = _setup(_engine(config=cfg), nodes, allocs, job, rows, metrics=False)
    ra = a.SystemPlaceGroupsMetrics(tgs, fallback=False, staged=staged)
    rb = system_place_groups_metrics_by_select(b, tgs)
    rc = c.SystemPlaceGroupsPreempt(tgs, fallback=False)
    _same_exact(ra, rb)
    _same_exact(ra, rc)
    _same_oracle(ra, ro)
    _same_metrics(ra, rb, ro, dev_k)
    with pytest.raises(Exception) as e:   # no "last Select" after the batched call
        a.LastMetrics()
    assert getattr(e.value, "code", None) == abi.PE_ESTATE
    if extra is not None:
        ea, xa = _after(a, after_rows, extra)
        eb, xb = _after(b, after_rows, extra)
        assert ea == eb == eo
        _same_exact(xa, xb)
        _same_oracle(xa, xo)
    return (a, b, c), ra, ro


# -- cluster_c4(777): the row-order and the list-order form, row index against position

N4, LIST_SEED = 777, 5


@functools.lru_cache(maxsize=None)
def _c4():
    nodes, allocs = synth.cluster_c4(N4, seed=11)
    web = synth.mock_system_job().task_groups[0]                    # task network: 50 MBits + 1 dynamic port
    # big fits an empty 4000-share node (3900 free) but not after web's 500
    job = _sys_job([web, _tg("big", 3500), _tg("mid", 3300, mem=3000), _tg("extra", 300, mem=128)])
    return nodes, allocs, job


@functools.lru_cache(maxsize=None)
def _c4_oracle(order, subset):
    nodes, allocs, job = _c4()
    rows = synth.shuffle(N4, LIST_SEED)
    rows = rows if subset is None else np.ascontiguousarray(rows[:subset])
    return _oracle_run(nodes, allocs, job, rows, order, PLAIN, 3)


@gpu
def test_row_order_form_and_row_index_against_position():
    """2331 entries over the full shuffled list: four workgroups of the
    row-order form, a partial last wave and tile, a packed-byte tail. The list
    is chosen so that for at least two groups the exhausted entry with the
    smallest snapshot row is not the one at the smallest position: a word
    keyed by the lane's index instead of rank_of[i] gives another answer."""
    nodes, allocs, job = _c4()
    rows = synth.shuffle(N4, LIST_SEED)
    ora = _c4_oracle((0, 1, 2), None)
    status, failed = ora[0][1], ora[0][5]["failed"]
    assert N4 * 3 == 2331 and len(failed) == 3
    trapped = 0
    for k in range(3):
        ex = np.flatnonzero(status[:, k] == 2)
        by_row = ex[np.argmin(np.asarray(rows)[ex])]
        trapped += int(by_row != ex[0])
    assert trapped >= 2
    _parity(nodes, allocs, job, rows, (0, 1, 2), extra=3, oracle=ora)


@gpu
def test_list_order_form_and_the_other_group_order():
    """60 rows, under a quarter of the snapshot: the list-order form; the groups
    in another order give other first failures."""
    nodes, allocs, job = _c4()
    rows = np.ascontiguousarray(synth.shuffle(N4, LIST_SEED)[:60])
    _, ra, _ = _parity(nodes, allocs, job, rows, (0, 1, 2), extra=3, oracle=_c4_oracle((0, 1, 2), 60))
    # big first: it is placed where it failed behind web's 500 shares, and web then fails there
    other = (1, 0, 2)
    _, rr, _ = _parity(nodes, allocs, job, rows, other, extra=3, oracle=_c4_oracle(other, 60))
    by_group = {other[k]: v for k, v in rr[5]["failed"].items()}
    assert set(by_group) == set(ra[5]["failed"]) == {0, 1, 2}
    assert by_group[0][0] < ra[5]["failed"][0][0] and by_group[1][0] > ra[5]["failed"][1][0]


# -- every dimension

def _dimensions():
    """40 nodes, every fifth with a 100-MBit NIC; three 50-MBit groups, then a
    group sized to fail on cpu, one on memory, one on disk (mock node: 3900
    shares, 7936 MB, 96 GiB free)."""
    ids = sorted(synth.uuids(40, 23))
    nodes = [synth.mock_node(i) for i in ids]
    for k, nd in enumerate(nodes):
        if k % 5 == 2:
            nd.networks[0].mbits = 100
            nd.node_class = "narrow"
            nd.compute_class()
    job = _sys_job([_tg("n0", 100, net=_net50()), _tg("n1", 100, net=_net50()), _tg("n2", 100, net=_net50()),
                    _tg("cpu", 3700), _tg("mem", 50, mem=7800), _tg("disk", 50, disk=97 * 1024),
                    _tg("extra", 10)])
    return nodes, [], job


@gpu
def test_every_dimension_is_some_groups_first():
    nodes, allocs, job = _dimensions()
    rows = synth.shuffle(40, 4)
    _, ra, _ = _parity(nodes, allocs, job, rows, range(6), extra=6)
    dims = {k: v[1] for k, v in ra[5]["failed"].items()}
    assert dims == {2: BANDWIDTH, 3: "cpu", 4: "memory", 5: "disk"}
    assert len(set(dims.values())) >= 3 and any(d.startswith("network:") for d in dims.values())
    assert ra[5]["failed"][2][2] == "narrow"


# -- devices: cluster_c5(300, busy=0.5)

GPU_TG, BIG, NET, EXTRA, GPU_PLAIN = 0, 1, 2, 3, 4


def _dev_groups():
    aff = [Affinity("${device.attr.cuda_cores}", "6000", ">", 60), Affinity("${device.attr.memory}", "40 GiB", ">", 30)]
    return [_tg("gpu", 500, mem=256, devices=[RequestedDevice("nvidia/gpu", 2, affinities=aff)]),
            _tg("big", 7200, mem=14000),
            _tg("net", 1500, mem=2048, net=_net50()),
            _tg("extra", 300, mem=128),
            _tg("gpu-plain", 500, mem=256, devices=[RequestedDevice("nvidia/gpu", 2)])]


@functools.lru_cache(maxsize=None)
def _c5():
    nodes, allocs = synth.cluster_c5(300, seed=9, busy=0.5)
    for a in allocs:
        a.max_parallel = 0   # no penalty that reads the plan's preemption counts
    return nodes, allocs, _sys_job(_dev_groups())


@functools.lru_cache(maxsize=None)
def _c5_oracle(order, preempting):
    nodes, allocs, job = _c5()
    return _oracle_run(nodes, allocs, job, synth.shuffle(300, 12), order, PRE if preempting else PLAIN, EXTRA)


@gpu
@pytest.mark.parametrize("order", [(GPU_TG, BIG, NET), (NET, BIG, GPU_TG)])
def test_device_scores_and_device_dimension(order):
    """A device ask with affinities on a plain stack: `scores` of every placed
    entry of that group are the helper's binpack and devices; on a node whose
    instances are all held the group's Select is exhausted by the devices."""
    nodes, allocs, job = _c5()
    ora = _c5_oracle(order, False)
    k = order.index(GPU_TG)
    assert ora[0][5]["failed"][k][1] == NO_MATCH
    _, ra, _ = _parity(nodes, allocs, job, synth.shuffle(300, 12), order, dev_k=k, extra=EXTRA, oracle=ora)
    assert len(ra[5]["scores"]) > 50 and len({v["devices"] for v in ra[5]["scores"].values()}) > 1


@gpu
def test_device_ask_without_affinities_scores_nothing():
    nodes, allocs, job = _c5()
    st, ra, _ = _parity(nodes, allocs, job, synth.shuffle(300, 12), (GPU_PLAIN, BIG, NET), dev_k=None, extra=EXTRA)
    assert ra[5]["failed"][0][1] == NO_MATCH and ra[5]["scores"] == {}
    fl, dg = C.POINTER(abi.pe_sysg_failure)(), C.c_int32(7)
    bp, dv, nn = abi.f64p(), abi.f64p(), C.c_uint32(0)
    a = _setup(_engine(), nodes, allocs, job, synth.shuffle(300, 12))
    a.SystemPlaceGroupsMetrics([GPU_PLAIN, BIG, NET], fallback=False)
    assert a._lib.pe_system_groups_metrics(a._h, C.byref(fl), C.byref(dg), C.byref(bp), C.byref(dv),
                                           C.byref(nn)) == abi.PE_OK
    assert dg.value == -1 and not bp and not dv and nn.value == 300


@gpu
@pytest.mark.parametrize("order", [(GPU_TG, BIG, NET), (NET, BIG, GPU_TG)])
def test_preempting_stack(order):
    """The groups of test_system_groups_preempt.py on a preempting stack: first
    failures are entries that stayed exhausted after evict, and the device
    group's entries placed by eviction carry their named scores."""
    nodes, allocs, job = _c5()
    ora = _c5_oracle(order, True)
    k = order.index(GPU_TG)
    _, ra, ro = _parity(nodes, allocs, job, synth.shuffle(300, 12), order, cfg=PRE, dev_k=k, extra=EXTRA, oracle=ora)
    assert ra[5]["failed"]                                             # stayed exhausted after evict
    assert any(key in ra[4] for key in ra[5]["scores"])                # a device entry placed by eviction
    assert any(key not in ra[4] for key in ra[5]["scores"])            # and plainly placed ones
    assert len({key[1] for key in ra[4]}) >= 2


@gpu
@pytest.mark.parametrize("cfg", [PLAIN, PRE], ids=["plain", "preempting"])
def test_row_order_form_with_unlisted_rows(cfg):
    """150 of 300 rows listed: in the row-order form the unlisted rows are lanes
    without a node inside every wave, which take part in the wave's ballots and
    reductions; the first-failure positions and the device group's named scores
    are by list position, not by row. The further SystemPlace runs over all 300
    rows: the rows the call must not have touched are compared too."""
    nodes, allocs, job = _c5()
    rows = np.ascontiguousarray(synth.shuffle(300, 12)[:150])
    listed = np.zeros(300, dtype=bool)
    listed[rows] = True
    assert 4 * len(rows) >= 300   # the row-order form
    assert all(listed[w:w + 64].any() and not listed[w:w + 64].all() for w in range(0, 300, 64))
    _, _, ro = _parity(nodes, allocs, job, rows, (GPU_TG, BIG, NET), cfg=cfg, dev_k=0, extra=EXTRA,
                       after_rows=np.arange(300, dtype=np.uint32))
    assert (ro[1] == 0).any() and (ro[1] == 2).any()   # placed and exhausted entries
    assert ro[5]["failed"] and ro[5]["scores"]
    assert (len(ro[4]) >= 1) == (cfg is PRE)           # evicting entries on the preempting stack


# -- nine groups on 40 nodes: across the 8-group chunk

@gpu
@pytest.mark.parametrize("cfg", [PLAIN, PRE], ids=["plain", "preempting"])
def test_nine_groups_cross_a_chunk(cfg):
    nodes, allocs = synth.cluster_c5(40, seed=6, busy=0.5)
    for a in allocs:
        a.max_parallel = 0
    g = _dev_groups()
    small = [_tg("s%d" % k, 100 + 10 * k) for k in range(6)]
    # gpu first, six small groups, then net at index 7 and big at index 8, the first group of the second chunk
    job = _sys_job([g[GPU_TG]] + small + [g[NET], g[BIG], g[EXTRA]])
    _, ra, _ = _parity(nodes, allocs, job, synth.shuffle(40, 2), range(9), cfg=cfg, dev_k=0, extra=9)
    failed = ra[5]["failed"]
    assert 8 in failed   # a first failure from the second chunk
    if cfg is PLAIN:     # ... at a smaller position than one of the first chunk (eviction places that one)
        assert any(k < 8 and failed[k][0] > failed[8][0] for k in failed)


# -- one 40-alloc node among eight: the relaunch at width 8

def _wide():
    """Eight nodes. Node 3 (8000 shares, 7900 free) holds 40 priority-20 allocs
    of 50 shares and one priority-95 alloc of 5600: a (1000) and b (1500) evict
    there, c's 2500 do not fit in the 2300 that no eviction can take. Node 6
    (8000 shares) holds one priority-95 alloc of 6000: a fits, b and c do not
    and nothing can be evicted. The others (12000 shares) hold one priority-20
    alloc of 6000 and take all three."""
    ids = sorted(synth.uuids(8, 5))
    nodes = [synth.mock_node(i) for i in ids]
    for k, nd in enumerate(nodes):
        nd.cpu_shares = 8000 if k in (3, 6) else 12000
    nodes[3].node_class = "wide"
    for nd in nodes:
        nd.compute_class()
    allocs = []
    for k, nd in enumerate(nodes):
        if k == 3:
            allocs += [Allocation(node_id=nd.id, job_id="many-%d" % (j % 5), task_group="tg", cpu_shares=50,
                                  memory_mb=32, disk_mb=10, priority=20) for j in range(40)]
            allocs.append(Allocation(node_id=nd.id, job_id="keep", task_group="tg", cpu_shares=5600, memory_mb=32,
                                     disk_mb=10, priority=95))
        else:
            allocs.append(Allocation(node_id=nd.id, job_id="one", task_group="tg", cpu_shares=6000, memory_mb=64,
                                     disk_mb=10, priority=95 if k == 6 else 20))
    job = _sys_job([_tg("a", 1000), _tg("b", 1500), _tg("c", 2500), _tg("extra", 200)])
    return nodes, allocs, job


@gpu
def test_first_failures_survive_the_wider_round():
    """c's first failure is on the wide node, written by the relaunch at width
    8; b's is on a narrow node at a later position, written by the first
    launch (which also offered c that later position); a never fails."""
    nodes, allocs, job = _wide()
    rows = np.arange(8, dtype=np.uint32)
    (a, _, _), ra, ro = _parity(nodes, allocs, job, rows, [0, 1, 2], cfg=PRE, extra=3)
    assert ra[5]["failed"] == {1: (6, "cpu", "linux-medium-pci"), 2: (3, "cpu", "wide")}
    assert ra[1][6].tolist() == [0, 2, 2] and ra[1][3].tolist() == [0, 0, 2]
    assert sum(len(v) for (pos, _), v in ra[4].items() if pos == 3) > 1
    st = _setup(_engine(config=PRE), nodes, allocs, job, rows)
    st._check(st._lib.pe_set_kernel_split(st._h, 1))
    st.SystemPlaceGroupsMetrics([0, 1, 2], fallback=False)
    ms4 = (C.c_double * 4)()
    st._check(st._lib.pe_last_kernel_split(st._h, C.cast(ms4, abi.f64p)))
    assert ms4[0] > 0.0 and ms4[1] > 0.0 and ms4[2] > 0.0 and ms4[3] > 0.0   # the fourth: a wider round ran


# -- the reference memo

@gpu
def test_reference_memo_advances_as_the_selects_would():
    """A group constraint makes the rack-r2 class ineligible. A later Select on
    a node of that class that was not in the list reads "computed class
    ineligible" from the memo: after the batched call as after the loop."""
    ids = sorted(synth.uuids(12, 31))
    nodes = [synth.mock_node(i) for i in ids]
    for k, nd in enumerate(nodes):
        nd.meta["rack"] = "r2" if k % 3 == 0 else "r1"
        nd.compute_class()
    job = _sys_job([_tg("a", 300), _tg("b", 300, constraints=[Constraint("${meta.rack}", "r2", "!=")]),
                    _tg("c", 3500), _tg("extra", 100)])
    rows = np.arange(1, 12, dtype=np.uint32)       # node 0 (rack r2) is not listed
    (a, b, _), ra, _ = _parity(nodes, [], job, rows, [0, 1, 2])
    o = _setup(OracleSystemStack(), nodes, [], job, rows)
    system_place_groups_metrics_by_select(o, [0, 1, 2])
    assert (ra[1][:, 1] == 1).any() and (ra[1][:, 1] == 0).any()
    seen = []
    for st in (a, b, o):
        st.SetNodes(np.zeros(1, dtype=np.uint32))
        r = st.SelectRaw(1)
        assert r.row < 0 and r.nodes_filtered == 1
        assert st.LastMetrics()["ConstraintFiltered"] == {"computed class ineligible": 1}
        el = st.Eligibility()
        seen.append({"job": el["job"], "tgs": el["tgs"]})
    assert seen[0] == seen[1] == seen[2]


# -- metrics off, other forms, follow-ups

def _accessor(st):
    fl, dg = C.POINTER(abi.pe_sysg_failure)(), C.c_int32(0)
    bp, dv, nn = abi.f64p(), abi.f64p(), C.c_uint32(0)
    return st._lib.pe_system_groups_metrics(st._h, C.byref(fl), C.byref(dg), C.byref(bp), C.byref(dv), C.byref(nn))


@gpu
@pytest.mark.parametrize("cfg", [PLAIN, PRE], ids=["plain", "preempting"])
def test_metrics_off_is_the_preempt_call(cfg):
    from nomad_amd.stack import EngineError
    nodes, allocs, job = _c5()
    rows = synth.shuffle(300, 12)
    order = [GPU_TG, BIG, NET]
    a = _setup(_engine(config=cfg), nodes, allocs, job, rows, metrics=False)
    c = _setup(_engine(config=cfg), nodes, allocs, job, rows, metrics=False)
    assert _accessor(a) == abi.PE_ESTATE                       # before any call
    ra = a.SystemPlaceGroupsMetrics(order, fallback=False)
    _same_exact(ra, c.SystemPlaceGroupsPreempt(order, fallback=False))
    assert ra[5] == {"failed": {}, "scores": {}}
    assert _accessor(a) == abi.PE_ESTATE
    with pytest.raises(EngineError):
        a.SystemGroupsMetrics(3)
    ea, xa = _after(a, rows, EXTRA)
    ec, xc = _after(c, rows, EXTRA)
    assert ea == ec
    _same_exact(xa, xc)


@gpu
def test_other_forms_and_follow_ups():
    nodes, allocs, job = _c5()
    rows = synth.shuffle(300, 12)
    order = (GPU_TG, BIG, NET)
    ora = _c5_oracle(order, True)
    # null arrays + pe_system_groups_results
    (a, _, _), first, _ = _parity(nodes, allocs, job, rows, order, cfg=PRE, dev_k=0, extra=None, oracle=ora,
                                  staged=True)
    # the accessor again gives the same; a pe_system_place* call in between invalidates it
    assert a.SystemGroupsMetrics(3) == first[5]
    a.SystemPlace(EXTRA)
    assert _accessor(a) == abi.PE_ESTATE
    # ResetPlan and again: equal to the first call and to a fresh handle
    a.ResetPlan()
    a.SetJob(job)
    a.SetNodes(rows)
    again = a.SystemPlaceGroupsMetrics(list(order), fallback=False)
    _same_exact(first, again)
    assert first[5] == again[5]
    # one row (one whose gpu entry stays exhausted), one group, an empty list
    pos = min(v[0] for v in first[5]["failed"].values())
    _parity(nodes, allocs, job, rows[pos:pos + 1], order, cfg=PRE, dev_k=0, extra=EXTRA)
    _parity(nodes, allocs, job, rows, [BIG], cfg=PRE, extra=EXTRA)
    _parity(nodes, allocs, job, rows, [GPU_TG], cfg=PLAIN, dev_k=0, extra=EXTRA)
    e = _setup(_engine(config=PRE), nodes, allocs, job, rows)
    e.SetNodes(np.zeros(0, dtype=np.uint32))
    sc, st, cn, p, pre, m = e.SystemPlaceGroupsMetrics([GPU_TG, EXTRA], fallback=False)
    assert sc.shape == (0, 2) and st.shape == (0, 2) and cn.tolist() == [[0, 0, 0]] * 2 and p == 0 and pre == {}
    assert m == {"failed": {}, "scores": {}}


# -- refusals and argument errors: pe_system_place_groups_preempt's, minus metrics

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
        "several devices": dict(devices=[0, 0]),
        "group unsupported": dict(groups=[_tg("a", 100), _tg("b", 100, devices=dev(300))]),
    }


@gpu
@pytest.mark.parametrize("case", sorted(_refusal_cases()))
def test_refusals_change_nothing(case):
    """Each refusal of the preempt call, with metrics on, on a fresh preempting
    handle: Unsupported without the fallback, and a following per-group
    SystemPlace equal to a fresh handle's."""
    from nomad_amd.stack import Unsupported
    kw = _refusal_cases()[case]
    ids = sorted(synth.uuids(40, 17))
    nodes = [synth.nvidia_node(i) if k % 2 else synth.mock_node(i) for k, i in enumerate(ids)]
    if "extra_net" in kw:
        nodes[5].networks.append(kw["extra_net"])
        nodes[5].compute_class()
    allocs = [Allocation(node_id=nodes[k].id, job_id="low", task_group="tg", cpu_shares=1000, memory_mb=64, disk_mb=10,
                         priority=20) for k in range(0, 40, 3)]
    if kw.get("mp"):
        allocs.append(Allocation(node_id=nodes[39].id, job_id="mp", task_group="tg", cpu_shares=10, memory_mb=8,
                                 disk_mb=1, priority=20, max_parallel=1))
    if "alloc_devices" in kw:
        allocs.append(Allocation(node_id=nodes[7].id, job_id="two-tasks", task_group="tg", cpu_shares=10, memory_mb=8,
                                 disk_mb=1, priority=20, devices=kw["alloc_devices"]))
    job = _sys_job(kw.get("groups", [_tg("a", 100), _tg("b", 3500)]), constraints=kw.get("job_cons", ()))
    rows = kw.get("rows", list(range(40)))

    def make():
        st = _engine(config=PRE, devices=kw["devices"]) if "devices" in kw else _engine(config=PRE)
        return _setup(st, nodes, allocs, job, rows)

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
        a.SystemPlaceGroupsMetrics([0, 1], fallback=False)
    assert _accessor(a) == abi.PE_ESTATE
    assert per_group(a) == per_group(make())   # nothing changed: a fresh handle gives the same


@gpu
def test_argument_errors():
    from nomad_amd.stack import EngineError, GenericStack
    nodes, allocs, job = _c5()
    rows = np.arange(50, dtype=np.uint32)
    a = _setup(_engine(config=PRE), nodes, allocs, job, rows)
    fn = a._lib.pe_system_place_groups_metrics
    placed = C.c_uint32(7)
    t = np.array([0, 1], dtype=np.uint32)
    sc, st, cn = np.zeros(100), np.zeros(25, np.uint8), np.zeros(6, np.uint32)
    args = (sc.ctypes.data_as(abi.f64p), st.ctypes.data_as(abi.u8p), cn.ctypes.data_as(abi.u32p))
    tp = t.ctypes.data_as(abi.u32p)
    assert fn(a._h, tp, 0, *args, C.byref(placed)) == abi.PE_EINVAL                       # n_tg == 0
    assert fn(a._h, np.array([0, 9], np.uint32).ctypes.data_as(abi.u32p), 2, *args, C.byref(placed)) == abi.PE_EINVAL
    assert fn(a._h, np.array([1, 1], np.uint32).ctypes.data_as(abi.u32p), 2, *args, C.byref(placed)) == abi.PE_EINVAL
    assert fn(a._h, tp, 2, args[0], None, args[2], C.byref(placed)) == abi.PE_EINVAL      # mixed null / set
    assert fn(a._h, tp, 2, None, None, args[2], C.byref(placed)) == abi.PE_EINVAL
    assert _accessor(a) == abi.PE_ESTATE                                                  # the failed calls left none
    assert a._lib.pe_system_groups_metrics(a._h, None, None, None, None, None) == abi.PE_EINVAL
    with pytest.raises(EngineError):
        a.SystemPlaceGroupsMetrics([0, 0], fallback=False)
    g = GenericStack()
    g.SetState(nodes, allocs)
    g.SetJob(job)
    g.SetNodes(rows)
    g.EnableMetrics(True)
    assert fn(g._h, tp, 2, *args, C.byref(placed)) == abi.PE_ESTATE                       # not a system stack
    # nothing changed on the system handle: the call now equals a fresh handle's
    fresh = _setup(_engine(config=PRE), nodes, allocs, job, rows)
    ra = a.SystemPlaceGroupsMetrics([0, 1], fallback=False)
    rf = fresh.SystemPlaceGroupsMetrics([0, 1], fallback=False)
    _same_exact(ra, rf)
    assert ra[5] == rf[5] and ra[5]["scores"]
