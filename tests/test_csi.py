"""Task groups with CSI volumes on the device path (pe_set_csi, pe_set_csi_requests,
pe_csi_alloc_index, pe_csi_check, k_csi_avail) and the Select rule that goes
with an availability checker.

References (the oracle has no CSI):
  - `csi_code`, a restatement of CSIVolumeChecker.isFeasible
    (scheduler/feasible.go:261-337) that returns the engine's code instead of
    the reason text: 0, or request index << 3 | reason, the reason numbered in
    the order the checks run. The requests' list order stands in for the
    reference's map order.
  - the oracle's Select of the same job without CSI over the node list that
    FeasibilityWrapper.Next (feasible.go:1061-1153) would have let through:
    unavailable nodes of a class not yet memoised are skipped, the first
    unavailable node of a class already memoised eligible ends the list.
"""
import copy
import math

import numpy as np
import pytest

from nomad_amd import abi, synth
from nomad_amd.encode import EncodedCSI, Interner
from nomad_amd.structs import (Affinity, Allocation, CSINodePlugin, CSIVolume, CSIVolumeRequest, Constraint, DriverInfo, SchedulerConfig,
                               Task, TaskGroup)

NS = "default"


def csi_code(node, reqs, suffix, volumes, node_volumes, namespace, job_id):
    """isFeasible for one node: `reqs` in list order, `suffix` AllocSuffix(allocName)."""
    if not reqs:
        return 0
    by_id = {(v.namespace, v.id): v for v in volumes}
    any_ns = {v.id: v for v in volumes}
    plugin_count = {}
    for vid in node_volumes.get(node.id, ()):                 # CSIVolumesByNodeID
        pid = any_ns[vid].plugin_id
        plugin_count[pid] = plugin_count.get(pid, 0) + 1
    for q, r in enumerate(reqs):
        def code(reason):
            return q << 3 | reason
        vol = by_id.get((namespace, r.source + (suffix if r.per_alloc else "")))
        if vol is None:
            return code(abi.PE_CSI_NOT_FOUND)
        plugin = node.csi_node_plugins.get(vol.plugin_id)
        if plugin is None:
            return code(abi.PE_CSI_NO_PLUGIN)
        if not plugin.healthy:
            return code(abi.PE_CSI_UNHEALTHY)
        if plugin_count.get(vol.plugin_id, 0) >= plugin.max_volumes:
            return code(abi.PE_CSI_MAX_VOLUMES)
        if r.read_only:
            if not vol.read_schedulable:
                return code(abi.PE_CSI_NO_READ)
        else:
            if not vol.write_schedulable:
                return code(abi.PE_CSI_NO_WRITE)
            if not vol.write_free_claims:
                for holder in vol.write_allocs:
                    if holder is None or holder != (namespace, job_id):
                        return code(abi.PE_CSI_IN_USE)
    return 0


# ---- TestCSIVolumeChecker (scheduler/feasible_test.go:234-403) as data ----------

def kat():
    nodes = [synth.mock_node("kat-node-%d" % i) for i in range(5)]
    nodes[0].csi_node_plugins = {"foo": CSINodePlugin(True, 1)}
    nodes[1].csi_node_plugins = {"foo": CSINodePlugin(False, 1)}
    nodes[2].csi_node_plugins = {"bar": CSINodePlugin(True, 1)}
    nodes[4].csi_node_plugins = {"foo": CSINodePlugin(True, 1)}
    volumes = [CSIVolume("volume-id", NS, "foo"), CSIVolume("vid2-in-use", NS, "foo"),
               CSIVolume("volume-id[0]", NS, "foo")]
    node_volumes = {nodes[4].id: ["vid2-in-use"]}   # the alloc on nodes[4] mounts vid2
    return nodes, volumes, node_volumes


# the test's alloc has no Name, so AllocSuffix is "" and "unique" names volume-id[0] itself
KAT_REQS = [CSIVolumeRequest("volume-id"), CSIVolumeRequest("volume-id[0]", per_alloc=True)]
KAT_CASES = [(0, True, True), (1, True, False), (2, True, False), (3, False, True), (0, False, True),
             (3, True, False), (4, True, False)]    # (node, volumes requested, Result)
KAT_CODES = [0, abi.PE_CSI_UNHEALTHY, abi.PE_CSI_NO_PLUGIN, abi.PE_CSI_NO_PLUGIN, abi.PE_CSI_MAX_VOLUMES]


def test_csi_volume_checker_kat():
    nodes, volumes, node_volumes = kat()
    got = [csi_code(nodes[i], KAT_REQS if req else [], "", volumes, node_volumes, NS, "job") == 0
           for i, req, _ in KAT_CASES]
    assert got == [True, False, False, True, True, False, False]
    assert got == [want for _, _, want in KAT_CASES]
    assert [csi_code(nd, KAT_REQS, "", volumes, node_volumes, NS, "job") for nd in nodes] == KAT_CODES
    # "add a missing volume" (feasible_test.go:412-424): the request that is not found names the code
    reqs = KAT_REQS + [CSIVolumeRequest("does-not-exist")]
    assert csi_code(nodes[0], reqs, "", volumes, node_volumes, NS, "job") == 2 << 3 | abi.PE_CSI_NOT_FOUND


def test_csi_encoder_round_trip():
    nodes, volumes, node_volumes = kat()
    volumes[1].write_free_claims = False
    volumes[1].write_allocs = [(NS, "some-job"), None]
    volumes[2].read_schedulable = False
    enc = EncodedCSI(nodes, volumes, node_volumes, Interner())
    assert enc.table.n_nodes == 5 and enc.table.n_volumes == 3
    plugins, vols, node_vols = enc.decode()
    assert plugins == [nd.csi_node_plugins for nd in nodes]
    assert vols == volumes
    assert node_vols == [[], [], [], [], [1]]
    for off in ("plug_off", "node_vol_off"):
        assert len(enc.cols[off]) == 6 and enc.cols[off][0] == 0
    assert list(enc.cols["claim_off"]) == [0, 0, 2, 2]
    assert enc.cols["claim_ns"][1] == abi.PE_NONE and enc.cols["claim_job"][1] == abi.PE_NONE


# ---- the engine ------------------------------------------------------------------

def engine_generic(**kw):
    from nomad_amd.stack import GenericStack
    return GenericStack(**kw)


def engine_system(**kw):
    from nomad_amd.stack import SystemStack
    return SystemStack(**kw)


def csi_job(reqs, count=1, job_id="csi-job", extra_group=False, constraints=()):
    job = synth.mock_job(job_id, count)
    job.task_groups[0].csi_volumes = list(reqs)
    job.constraints = job.constraints + list(constraints)
    if extra_group:
        job.task_groups.append(TaskGroup(name="plain", count=1, tasks=[Task(name="plain", cpu=300, memory_mb=128)]))
    return job


def plain(job):
    """The same job without its CSI requests (what the oracle can run)."""
    j = copy.deepcopy(job)
    for g in j.task_groups:
        g.csi_volumes = []
    return j


def engine_with(nodes, volumes, node_volumes, job, perm=None, allocs=(), stack=engine_generic, csi=True, **kw):
    e = stack(**kw)
    e.SetState(nodes, list(allocs))
    if csi:
        e.SetCSI(volumes, node_volumes)
    e.SetJob(job)
    e.SetNodes(list(perm if perm is not None else range(len(nodes))))
    return e


@pytest.mark.gpu
def test_csi_check_kat_nodes():
    nodes, volumes, node_volumes = kat()
    # the engine's per_alloc source is source + "[idx]": "volume-id" at index 0 is the KAT's volume-id[0]
    reqs = [CSIVolumeRequest("volume-id"), CSIVolumeRequest("volume-id", per_alloc=True)]
    job = csi_job(reqs)
    e = engine_with(nodes, volumes, node_volumes, job)
    want = [csi_code(nd, reqs, "[0]", volumes, node_volumes, NS, job.id) for nd in nodes]
    assert want == KAT_CODES
    got = e.CSICheck(0)
    assert got.dtype == np.uint16 and list(got) == want
    e.CSIAllocIndex(0, 1)   # volume-id[1] does not exist: request 1 is not found wherever request 0 passes
    want1 = [csi_code(nd, reqs, "[1]", volumes, node_volumes, NS, job.id) for nd in nodes]
    assert want1[0] == 1 << 3 | abi.PE_CSI_NOT_FOUND
    assert list(e.CSICheck(0)) == want1


RANDOM_REQS = [CSIVolumeRequest("va"), CSIVolumeRequest("vb", per_alloc=True), CSIVolumeRequest("vc", read_only=True, per_alloc=True)]
RANDOM_INDICES = [0, 1, 2, 3, 4, 5]


def random_cluster(n, seed):
    """0 to 3 plugins per node (healthy or not, MaxVolumes 1, 2 or unbounded), 0
    to 4 volumes in use. Request 0 passes at the volume level (its write claims
    are all held by the placing job); request 1 is per_alloc: index 0 passes,
    1 has no write claims, 2 and 4 are held by another job / a lost alloc, 3 does
    not exist; request 2 (read only, per_alloc) has no read claims at index 0.
    At index 5 every request passes at the volume level."""
    rng = np.random.Generator(np.random.PCG64(seed))
    nodes = [synth.mock_node("csi-%04d-%05d" % (seed, i)) for i in range(n)]
    job_id = "csi-job"
    volumes = [
        CSIVolume("va", NS, "p0", write_free_claims=False, write_allocs=[(NS, job_id), (NS, job_id)]),
        CSIVolume("vb[0]", NS, "p1"),
        CSIVolume("vb[1]", NS, "p1", write_schedulable=False),
        CSIVolume("vb[2]", NS, "p1", write_free_claims=False, write_allocs=[(NS, job_id), ("other", job_id)]),
        CSIVolume("vb[4]", NS, "p1", write_free_claims=False, write_allocs=[None]),
        CSIVolume("vb[5]", NS, "p1"),
        CSIVolume("vc[0]", NS, "p2", read_schedulable=False),
        CSIVolume("vc[5]", NS, "p2", write_schedulable=False),
        CSIVolume("vb[3]", "other", "p0"),       # another namespace's volume of that id
        CSIVolume("filler-0", NS, "p0"), CSIVolume("filler-1", NS, "p1"), CSIVolume("filler-2", NS, "p2"),
    ]
    in_use = ["filler-0", "filler-1", "filler-2", "va", "vb[0]"]
    node_volumes = {}
    for nd in nodes:
        k = int(rng.integers(0, 4))
        for p in rng.permutation(3)[:k]:
            nd.csi_node_plugins["p%d" % p] = CSINodePlugin(bool(rng.random() < 0.8),
                                                           [1, 2, (1 << 63) - 1][int(rng.integers(0, 3))])
        m = int(rng.integers(0, 5))
        if m:
            node_volumes[nd.id] = [in_use[int(i)] for i in rng.integers(0, len(in_use), m)]
    return nodes, volumes, node_volumes, job_id


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_csi_check_random_clusters(n):
    nodes, volumes, node_volumes, job_id = random_cluster(n, seed=100 + n)
    job = csi_job(RANDOM_REQS, job_id=job_id)
    e = engine_with(nodes, volumes, node_volumes, job)
    for idx in RANDOM_INDICES:
        e.CSIAllocIndex(0, idx)
        want = [csi_code(nd, RANDOM_REQS, "[%d]" % idx, volumes, node_volumes, NS, job_id) for nd in nodes]
        assert list(e.CSICheck(0)) == want, idx


def test_csi_random_clusters_reach_every_reason():
    """The cases of test_csi_check_random_clusters, by the restatement alone:
    together they hold every reason 1 to 7 and available nodes."""
    seen = set()
    for n in (1, 63, 65, 257):
        nodes, volumes, node_volumes, job_id = random_cluster(n, seed=100 + n)
        for idx in RANDOM_INDICES:
            seen |= {csi_code(nd, RANDOM_REQS, "[%d]" % idx, volumes, node_volumes, NS, job_id) for nd in nodes}
    assert {c & 7 for c in seen if c} == {1, 2, 3, 4, 5, 6, 7}
    assert 0 in seen and {c >> 3 for c in seen if c} == {0, 1, 2}


# ---- the Select rule ---------------------------------------------------------------

STOP_REQS = [CSIVolumeRequest("vol")]


def stop_cluster(unavailable=(0, 5), meta_on_plugin_nodes=False, seed=9):
    """64 mock nodes of one computed class in a shuffled visit order; the nodes
    at the visit positions `unavailable` run no plugin."""
    nodes, _ = synth.cluster_c1(64, seed=seed)
    perm = [int(x) for x in synth.shuffle(64, seed + 1)]
    lacking = {perm[p] for p in unavailable}
    for r, nd in enumerate(nodes):
        if r not in lacking:
            nd.csi_node_plugins = {"foo": CSINodePlugin(True)}
            if meta_on_plugin_nodes:
                nd.meta["csi"] = "yes"
                nd.compute_class()
    return nodes, perm, [CSIVolume("vol", NS, "foo")], {}


def wrapper_walk(perm, cursor, limit, unavailable_rows, eligible):
    """FeasibilityWrapper.Next + LimitIterator over a ring of nodes of one class
    that all pass every check and all fit with a positive score: the rows that
    come through as options, the AllocMetric counts, the cursor afterwards and
    the class's memo. An unavailable node is skipped while the class is not
    memoised (its checks pass, so it memoises the class), and ends the stream
    once it is."""
    n = len(perm)
    rows, evaluated, filtered = [], 0, 0
    for k in range(n):
        row = perm[(cursor + k) % n]
        evaluated += 1
        if row in unavailable_rows:
            filtered += 1
            if eligible:
                break
            eligible = True
            continue
        eligible = True
        rows.append(row)
        if len(rows) == limit:
            break
    return rows, evaluated, filtered, (cursor + evaluated) % n, eligible


def oracle_on(o, tg, rows, limit):
    o.SetNodes(rows)
    o.SetCursor(0, limit)
    return o.SelectRaw(tg)


def same_option(got, want):
    assert got.row == want.row
    if want.row >= 0:
        assert got.final_score == want.final_score and got.scores == want.scores


@pytest.mark.gpu
def test_select_stops_at_unavailable_node_of_eligible_class():
    from oracle.oracle import OracleGenericStack
    nodes, perm, volumes, node_volumes = stop_cluster()
    job = csi_job(STOP_REQS)
    e = engine_with(nodes, volumes, node_volumes, job, perm)
    limit = e.limit
    assert 2 <= limit < 58   # the walk is windowed
    o = OracleGenericStack()
    o.SetState(nodes, [])
    o.SetJob(plain(job))
    lacking = {perm[0], perm[5]}
    assert [int(c) for c in e.CSICheck(0)] == [abi.PE_CSI_NO_PLUGIN if r in lacking else 0 for r in range(64)]

    rows, evaluated, filtered, cursor, eligible = wrapper_walk(perm, 0, limit, lacking, False)
    assert rows == perm[1:5] and (evaluated, filtered, cursor) == (6, 2, 6)
    got = e.SelectRaw(0)
    want = oracle_on(o, 0, rows, limit)
    assert want.nodes_evaluated == 4
    same_option(got, want)
    assert (got.nodes_evaluated, got.nodes_filtered, got.nodes_exhausted, got.new_offset) == (6, 2, 0, 6)
    assert e.GetCursor() == (6, limit)
    assert e.GetClasses(e.Eligibility()) == {nodes[0].computed_class: True}
    e.Commit(0, got.row)
    o.Commit(0, want.row)

    for _ in range(10):
        cur = e.GetCursor()[0]
        assert cur == cursor
        rows, evaluated, filtered, cursor, eligible = wrapper_walk(perm, cur, limit, lacking, eligible)
        got = e.SelectRaw(0)
        want = oracle_on(o, 0, rows, limit)
        assert want.nodes_evaluated == len(rows) and want.nodes_filtered == 0
        same_option(got, want)
        assert (got.nodes_evaluated, got.nodes_filtered, got.nodes_exhausted, got.new_offset) == \
            (evaluated, filtered, 0, cursor)
        if got.row < 0:
            continue
        e.Commit(0, got.row)
        o.Commit(0, want.row)
    assert cursor < 6   # the rounds went once round the ring and met position 0 again, memoised this time


@pytest.mark.gpu
def test_no_stop_when_unavailable_classes_are_ineligible():
    from oracle.oracle import OracleGenericStack
    nodes, perm, volumes, node_volumes = stop_cluster(meta_on_plugin_nodes=True)
    job = csi_job(STOP_REQS, constraints=[Constraint("${meta.csi}", "yes", "=")])
    e = engine_with(nodes, volumes, node_volumes, job, perm)
    o = OracleGenericStack()
    o.SetState(nodes, [])
    o.SetJob(plain(job))
    o.SetNodes(perm)
    for k in range(20):
        got, want = e.SelectRaw(0), o.SelectRaw(0)
        same_option(got, want)
        assert (got.nodes_evaluated, got.nodes_filtered, got.nodes_exhausted, got.new_offset) == \
            (want.nodes_evaluated, want.nodes_filtered, want.nodes_exhausted, want.new_offset), k
        assert got.row >= 0
        e.Commit(0, got.row)
        o.Commit(0, want.row)
    ee, oe = e.Eligibility(), o.Eligibility()
    assert ee["job"] == oe["job"] and ee["tgs"] == oe["tgs"]
    assert False in ee["job"].values()


@pytest.mark.gpu
def test_resume_corner_is_refused_untouched():
    from nomad_amd.stack import SelectOptions, Unsupported
    nodes, perm, volumes, node_volumes = stop_cluster()
    job = csi_job(STOP_REQS, extra_group=True)
    e = engine_with(nodes, volumes, node_volumes, job, perm)
    fresh = engine_with(nodes, volumes, node_volumes, job, perm)
    cursor, elig = e.GetCursor(), e.Eligibility()
    # a reschedule penalty on position 2 makes that option's score (binpack - 1) / 2 <= 0: LimitIterator
    # sets it aside and, when the stream ends at position 5, asks the source again
    opts = SelectOptions(penalty_node_ids=[nodes[perm[2]].id])
    with pytest.raises(Unsupported):
        e.Select(0, opts)
    assert e.GetCursor() == cursor
    assert e.Eligibility() == elig
    got, want = e.SelectRaw(1), fresh.SelectRaw(1)
    same_option(got, want)
    assert (got.nodes_evaluated, got.nodes_filtered, got.new_offset) == \
        (want.nodes_evaluated, want.nodes_filtered, want.new_offset)
    # without the penalty the same Select is answered (the stop alone is on the device path)
    assert e.SetNodes(perm) == fresh.SetNodes(perm)
    assert e.SelectRaw(0).nodes_evaluated == 6


@pytest.mark.gpu
def test_system_stack_filters_unavailable_nodes():
    from oracle.oracle import OracleSystemStack
    nodes, _ = synth.cluster_c1(300, seed=21)
    for r, nd in enumerate(nodes):
        if r % 3:
            nd.csi_node_plugins = {"foo": CSINodePlugin(True)}
    volumes = [CSIVolume("vol", NS, "foo")]
    job = synth.mock_system_job("csi-system")
    job.task_groups[0].csi_volumes = list(STOP_REQS)
    order = [int(x) for x in synth.shuffle(300, 22)]
    avail = [r for r in order if r % 3]

    o = OracleSystemStack()
    o.SetState(nodes, [])
    o.SetJob(plain(job))
    o.SetNodes(avail)
    o_score, o_status, o_placed = o.SystemPlace(0)
    by_row = {r: (float(o_score[k]), int(o_status[k])) for k, r in enumerate(avail)}

    e = engine_with(nodes, volumes, {}, job, order, stack=engine_system)
    score, status, placed = e.SystemPlace(0)
    assert placed == o_placed == 200
    for k, r in enumerate(order):
        if r % 3 == 0:
            assert status[k] == 1 and math.isnan(score[k])
        else:
            assert (float(score[k]), int(status[k])) == by_row[r]

    # the same through per-node Selects (SystemScheduler.computePlacements' loop)
    e2 = engine_with(nodes, volumes, {}, job, order, stack=engine_system)
    for r in order:
        e2.SetNodes([r])
        got = e2.SelectRaw(0)
        assert got.nodes_evaluated == 1
        if r % 3 == 0:
            assert got.row < 0 and got.nodes_filtered == 1
        else:
            assert got.row == r and (got.final_score, 0) == by_row[r]
            e2.Commit(0, r)


@pytest.mark.gpu
def test_refusals_leave_the_handle_unchanged():
    from nomad_amd.stack import SelectOptions, Unsupported
    nodes, perm, volumes, node_volumes = stop_cluster()
    job = csi_job(STOP_REQS, count=3)
    allocs = [Allocation(nodes[perm[7]].id, job.id, "web", cpu_shares=500, memory_mb=256)]
    e = engine_with(nodes, volumes, node_volumes, job, perm, allocs=allocs)
    fresh = engine_with(nodes, volumes, node_volumes, job, perm, allocs=allocs)
    cursor, elig = e.GetCursor(), e.Eligibility()

    refused = {
        "preempt": lambda: e.Select(0, SelectOptions(preempt=True)),
        "preferred": lambda: e.Select(0, SelectOptions(preferred_nodes=[nodes[perm[1]].id])),
        "place": lambda: e.Place(0, 3),
        "batch": lambda: (e.StageOrders(np.asarray([perm], dtype=np.uint32)), e.PlaceBatch(0, 1)),
        "inplace": lambda: e.InplaceUpdate(0, [0], fallback=False),
        "inplace_metrics": lambda: e.InplaceUpdateMetrics(0, [0], fallback=False),
        "inplace_spread": lambda: e.InplaceUpdateSpread(0, [0], fallback=False),
    }
    for name, call in refused.items():
        with pytest.raises(Unsupported):
            call()
        assert e.GetCursor() == cursor, name
        assert e.Eligibility() == elig, name
    e.EnableMetrics(True)
    with pytest.raises(Unsupported):
        e.SelectRaw(0)
    e.EnableMetrics(False)
    assert e.GetCursor() == cursor and e.Eligibility() == elig
    e.SetNodes(perm)       # (pe_stage_orders and the in-place calls leave the list to the caller)
    got, want = e.SelectRaw(0), fresh.SelectRaw(0)
    same_option(got, want)
    assert (got.nodes_evaluated, got.nodes_filtered, got.new_offset) == (6, 2, 6) == \
        (want.nodes_evaluated, want.nodes_filtered, want.new_offset)


@pytest.mark.gpu
def test_system_group_calls_refuse_csi_groups():
    from nomad_amd.stack import Unsupported
    nodes, _ = synth.cluster_c1(40, seed=23)
    for nd in nodes[1:]:
        nd.csi_node_plugins = {"foo": CSINodePlugin(True)}
    job = synth.mock_system_job("csi-system")
    job.task_groups[0].csi_volumes = list(STOP_REQS)
    job.task_groups.append(TaskGroup(name="plain", count=1, tasks=[Task(name="plain", cpu=300, memory_mb=128)]))
    e = engine_with(nodes, [CSIVolume("vol", NS, "foo")], {}, job, stack=engine_system)
    for call in (e.SystemPlaceGroups, e.SystemPlaceGroupsPreempt, e.SystemPlaceGroupsMetrics):
        with pytest.raises(Unsupported):
            call([0, 1], fallback=False)
    score, status, placed = e.SystemPlace(0)   # the handle still answers, with node 0 filtered
    assert placed == 39 and status[0] == 1 and not status[1:].any()


@pytest.mark.gpu
def test_group_without_table_or_requests_is_refused_and_set_state_drops_the_table():
    from nomad_amd.stack import Unsupported
    nodes, perm, volumes, node_volumes = stop_cluster()
    job = csi_job(STOP_REQS)
    e = engine_with(nodes, volumes, node_volumes, job, perm, csi=False)
    with pytest.raises(Unsupported, match="CSI volumes"):
        e.SelectRaw(0)
    with pytest.raises(Unsupported, match="CSI volumes"):
        e.CSICheck(0)
    e.SetCSI(volumes, node_volumes)          # the table after the job: the group is placed from here on
    assert e.SelectRaw(0).nodes_evaluated == 6
    e.SetState(nodes, [])                    # a new snapshot drops the table
    e.SetJob(job)
    e.SetNodes(perm)
    with pytest.raises(Unsupported, match="CSI volumes"):
        e.SelectRaw(0)
    e.SetCSI(volumes, node_volumes)
    e.SetCSI(None)                           # and so does an explicit drop
    with pytest.raises(Unsupported, match="CSI volumes"):
        e.SelectRaw(0)


def assert_untouched_then_same(e, fresh, cursor, elig, tg=0):
    """After a refusal: cursor, limit and memo as before, and the next Select of a
    group the engine answers equals a fresh handle's."""
    assert e.GetCursor() == cursor
    assert e.Eligibility() == elig
    got, want = e.SelectRaw(tg), fresh.SelectRaw(tg)
    same_option(got, want)
    assert (got.nodes_evaluated, got.nodes_filtered, got.nodes_exhausted, got.new_offset) == \
        (want.nodes_evaluated, want.nodes_filtered, want.nodes_exhausted, want.new_offset)


@pytest.mark.gpu
def test_non_uniform_class_is_refused_untouched():
    """Drivers are not hashed into the computed class: a node whose exec driver
    is unhealthy makes its class non-uniform for the group's checks, and the memo
    shadow's deciding node then depends on the visit order ahead of the Select."""
    from nomad_amd.stack import Unsupported
    nodes, perm, volumes, node_volumes = stop_cluster()
    cls = nodes[perm[10]].computed_class
    nodes[perm[10]].drivers = dict(nodes[perm[10]].drivers, exec=DriverInfo(detected=True, healthy=False))
    assert nodes[perm[10]].computed_class == cls == nodes[perm[11]].computed_class
    job = csi_job(STOP_REQS, extra_group=True)
    job.task_groups[1].tasks[0].driver = "mock_driver"    # the plain group's class stays uniform
    e = engine_with(nodes, volumes, node_volumes, job, perm)
    fresh = engine_with(nodes, volumes, node_volumes, job, perm)
    cursor, elig = e.GetCursor(), e.Eligibility()
    with pytest.raises(Unsupported, match="CSI volumes with computed classes"):
        e.SelectRaw(0)
    assert_untouched_then_same(e, fresh, cursor, elig, tg=1)


def affinity_csi_job():
    job = csi_job(STOP_REQS)
    job.task_groups[0].affinities = [Affinity("${meta.database}", "mysql", "=", 50)]
    return job


@pytest.mark.gpu
def test_full_pass_group_no_stop_and_refused_stop():
    """A group with an affinity runs full passes (limit MaxInt32). Without a stop
    the Select is the oracle's over the available nodes plus the filtered ones;
    a full pass that ends at an unavailable node is handed back untouched."""
    from nomad_amd.stack import Unsupported
    from oracle.oracle import OracleGenericStack
    nodes, perm, volumes, node_volumes = stop_cluster()
    job = affinity_csi_job()
    lacking = {perm[0], perm[5]}
    # the group escapes its class (a unique attribute in a constraint): no memo entry, so never a stop
    esc = copy.deepcopy(job)
    esc.task_groups[0].constraints = [Constraint("${node.unique.id}", "no-such-node", "!=")]
    e = engine_with(nodes, volumes, node_volumes, esc, perm)
    o = OracleGenericStack()
    o.SetState(nodes, [])
    o.SetJob(plain(esc))
    o.SetNodes([r for r in perm if r not in lacking])
    got, want = e.SelectRaw(0), o.SelectRaw(0)
    same_option(got, want)
    assert (got.nodes_evaluated, got.nodes_filtered) == (64, 2) and want.nodes_evaluated == 62
    # memoised: position 0 is skipped and memoises the class, position 5 ends the stream
    e = engine_with(nodes, volumes, node_volumes, job, perm)
    cursor, elig = e.GetCursor(), e.Eligibility()
    with pytest.raises(Unsupported, match="full-pass Select"):
        e.SelectRaw(0)
    assert e.GetCursor() == cursor and e.Eligibility() == elig


@pytest.mark.gpu
def test_sharded_select_and_multi_device_handle_refuse_csi_groups():
    from nomad_amd.stack import Unsupported
    nodes, perm, volumes, node_volumes = stop_cluster()
    job = affinity_csi_job()    # a full pass, which the sharded Select takes when the group has no CSI
    e = engine_with(nodes, volumes, node_volumes, job, perm)
    cursor, elig = e.GetCursor(), e.Eligibility()
    with pytest.raises(Unsupported, match="CSI volumes"):
        e.SelectShard(0, 0, 64)
    assert e.GetCursor() == cursor and e.Eligibility() == elig
    no_csi = plain(job)
    no_csi.version = job.version + 1   # (SetJob keeps the stack's job when the version is the same)
    e.SetJob(no_csi)
    e.SetNodes(perm)
    assert len(e.SelectShard(0, 0, 64)) == 80   # the same call without the requests is answered

    m = engine_with(nodes, volumes, node_volumes, csi_job(STOP_REQS), perm, devices=[0, 0])
    cursor, elig = m.GetCursor(), m.Eligibility()
    with pytest.raises(Unsupported, match="CSI volumes on a handle over several devices"):
        m.SelectRaw(0)
    assert m.GetCursor() == cursor and m.Eligibility() == elig
