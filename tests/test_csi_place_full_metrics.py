"""pe_place_csi_full_metrics / pe_place_csi_maps: the count loop of a CSI task
group that runs full passes (node affinities, spreads, a latched limit) with
AllocMetric kept: k_csi_full's metrics form writes k_csi_loop<true>'s trace log,
the host walks windows of any length against the reference memo shadow, and one
batched trace against the checkpoint gives every record's maps with its own
spread tables.

Reference for the records: `test_csi_place.Ref` at limit 2**31 - 1, as
test_csi_place_full uses it.

Reference for record k's maps: test_csi_place_metrics.reference's method at that
limit. A second oracle stack with metrics on and the same commits runs a Select
(`SetCursor(0, 0x7FFFFFFF)`) over record k's consumed window without the rows
that reach the CSI checker and fail it; each removed row adds the restated
FilterNode: ClassFiltered[NodeClass] where the node has a class, and
ConstraintFiltered[text]. The oracle's own Select over the reduced window may
pick another row than `Ref` does (LimitIterator sets options aside and pops
them later, so ties resolve differently); the maps do not depend on that, since
ScoreNode is recorded upstream of LimitIterator in source order. `Ref`'s row is
what gets committed, and the oracle's row is not asserted.
"""
import ctypes as C
import os

import pytest

from nomad_amd import abi, synth
from nomad_amd.structs import (Allocation, CSINodePlugin, CSIVolume, Constraint, NetworkResource, Spread, Task,
                               TaskGroup)

from test_csi import NS, RANDOM_INDICES, RANDOM_REQS, STOP_REQS, csi_job, engine_with, plain, random_cluster
from test_csi_place import (LIB, PER_ALLOC_REQS, ROOT, Ref, assert_records, assert_untouched, class_elig, job_allocs,
                            same_record)
from test_csi_place_full import (AGAINST, EVEN, SPREAD_CASES, TARGET, UNBOUNDED, block, dc_cluster, full_job,
                                 memoised)
from test_csi_place_metrics import Case, NeverKnown, csi_keys, mixed_node_class, passes_checks

HEADER = os.path.join(ROOT, "include", "nomad_pe.h")


# ---- the cases --------------------------------------------------------------------------------

class FullCase(Case):
    """test_csi_place_metrics.Case for PlaceCSIFullMetrics. `sibling_first`: a
    Select of the plain sibling group, whose affinity latches the limit, comes
    before the call (and before the reference's cursor)."""

    def __init__(self, *a, sibling_first=False, check_plan=True, **kw):
        super().__init__(*a, **kw)
        self.sibling_first, self.check_plan = sibling_first, check_plan

    def engine(self, metrics):
        e = super().engine(metrics)
        if self.sibling_first:
            r = e.SelectRaw(1)
            assert e.GetCursor()[1] == UNBOUNDED and r.nodes_evaluated == len(self.perm)
            assert e.GetCursor()[0] == self.cursor_after_sibling
        return e


def spread_case(k, which):
    P, U = SPREAD_CASES[k]
    nodes, perm, volumes, node_volumes = dc_cluster(48, unavailable=U)
    job = full_job(5, spreads=TARGET) if which == "target" else full_job(5, spreads=EVEN, job_level=True)
    return FullCase("spread%d_%s" % (k, which), nodes, perm, volumes, node_volumes, job,
                    job_allocs(nodes, perm, job, P), count=5)


def affinity_case():
    """test_csi_place_full's negative affinity: most options score at or below 0,
    ten unavailable nodes, more than the seven nils one Select can take."""
    U = (3, 7, 12, 13, 19, 24, 30, 31, 38, 41)
    nodes, perm, volumes, node_volumes = dc_cluster(48, unavailable=U, dcs=("dc1",), mysql=lambda p: p % 3 != 0)
    mixed_node_class(nodes)
    job = full_job(8, affinities=AGAINST)
    return FullCase("affinity", nodes, perm, volumes, node_volumes, job,
                    job_allocs(nodes, perm, job, (0, 6, 9, 15, 18)), count=8)


def tie_case(wins):
    """test_csi_place_full's popped-option tie: every option non-positive, scores in bit-equal groups."""
    U = (4,)
    nodes, perm, volumes, node_volumes = dc_cluster(32, unavailable=U, dcs=("dc1",))
    job = full_job(3, affinities=AGAINST)
    P = tuple(p for p in range(32) if p not in U) + ((3,) if wins else ())
    return FullCase("tie_%s" % ("wins" if wins else "loses"), nodes, perm, volumes, node_volumes, job,
                    job_allocs(nodes, perm, job, P), count=2)


def latched_case():
    """The CSI group itself is plain; a Select of its sibling, which has an
    affinity, latched the limit (stack.go:165-167) with metrics on."""
    U, P = (2, 9, 14), (0, 4, 7, 12)
    nodes, perm, volumes, node_volumes = dc_cluster(48, unavailable=U, dcs=("dc1",))
    job = full_job(4, sibling_affinity=True)
    c = FullCase("latched", nodes, perm, volumes, node_volumes, job, job_allocs(nodes, perm, job, P), count=4,
                 sibling_first=True)
    c.cursor_after_sibling = 0          # a whole pass from 0 ends where it began
    return c


# (n, unavailable positions, count, cursor, positions holding an alloc of the job)
SHAPES = [
    (1, (), 3, 0, ()),
    (1, (0,), 2, 0, ()),
    (63, (1, 62), 4, 0, (3, 4)),                  # a stop at the last position
    (64, (10, 11), 4, 60, (61, 62, 2)),           # the wrap inside the first Select
    (65, (1, 63, 64), 4, 60, (61, 62, 2)),
    (65, (32,), 12, 0, (0, 1, 2)),                # every Select a whole pass but the ones that meet the stop
]


def shape_case(k):
    n, U, count, cursor, P = SHAPES[k]
    nodes, perm, volumes, node_volumes = dc_cluster(n, unavailable=U)
    job = full_job(count, spreads=TARGET)
    job.task_groups[0].tasks[0].cpu = 1900          # two per node
    return FullCase("shape%d" % k, nodes, perm, volumes, node_volumes, job, job_allocs(nodes, perm, job, P),
                    count=count, cursor=cursor)


def overfull_case():
    """A count larger than what fits (two per node on 12 nodes, one unavailable):
    the loop ends in a nil record, which has maps too."""
    nodes, perm, volumes, node_volumes = dc_cluster(12, unavailable=(7,))
    job = full_job(40, spreads=EVEN)
    job.task_groups[0].tasks[0].cpu = 1900
    return FullCase("overfull", nodes, perm, volumes, node_volumes, job, count=40)


def block_case(delta):
    """n = BLOCK - 1 and BLOCK + 1, the cursor three before the end: consumption
    sums past n, so the log offsets pass the list length."""
    n = block() + delta
    U = (5, n // 2, n - 1)
    nodes, perm, volumes, node_volumes = dc_cluster(n, unavailable=U)
    job = full_job(3, spreads=TARGET)
    return FullCase("block%+d" % delta, nodes, perm, volumes, node_volumes, job,
                    job_allocs(nodes, perm, job, (0, 1, 2, n - 2)), count=3, cursor=n - 3, check_plan=False)


def unmemoised_case():
    """No memo at call start: in each datacenter's class the first unavailable
    node is the skip that decides it (F[c]), a later one a stop; the log's stop
    bits must agree with the metrics shadow of the memo."""
    U = (0, 3, 9, 12, 15)
    nodes, perm, volumes, node_volumes = dc_cluster(48, unavailable=U)
    job = full_job(4, spreads=TARGET)
    return FullCase("unmemoised", nodes, perm, volumes, node_volumes, job, job_allocs(nodes, perm, job, (1, 2)),
                    count=4, memo=False)


def random_case(n, idx):
    """test_csi.random_cluster, a group that escapes its class (never a stop) and
    spreads: every Select consumes the whole list and meets all seven reasons."""
    nodes, volumes, node_volumes, job_id = random_cluster(n, seed=100 + n)
    perm = [int(x) for x in synth.shuffle(n, 7 + n)]
    job = csi_job(RANDOM_REQS, count=3, job_id=job_id, extra_group=True)
    job.task_groups[0].constraints = [Constraint("${node.unique.id}", "no-such-node", "!=")]
    job.task_groups[0].spreads = list(EVEN)
    return FullCase("random%d_%d" % (n, idx), nodes, perm, volumes, node_volumes, job, count=3, memo=False,
                    alloc_idx=[idx, 5, idx], escaped_tg=True, ref_elig=False)


def per_alloc_case():
    """vol[0] on plugin foo (every node), vol[1] on plugin bar (even visit
    positions): two record sets across alloc_idx, reason texts per record."""
    nodes, perm, volumes, node_volumes = dc_cluster(48)
    for p, r in enumerate(perm):
        if p % 2 == 0:
            nodes[r].csi_node_plugins["bar"] = CSINodePlugin(True)
    volumes = [CSIVolume("vol[0]", NS, "foo"), CSIVolume("vol[1]", NS, "bar")]
    job = full_job(4, spreads=TARGET, reqs=PER_ALLOC_REQS)
    return FullCase("per_alloc", nodes, perm, volumes, node_volumes, job, job_allocs(nodes, perm, job, (1, 4)),
                    count=4, alloc_idx=[0, 1, 0, 1])


def full_nodes_case():
    """Foreign allocs fill the CPU of some nodes and the bandwidth of others, the
    task asks for 100 MBits, under a spread: DimensionExhausted 'cpu' and
    'network: bandwidth exceeded'."""
    U = (7, 16)
    nodes, perm, volumes, node_volumes = dc_cluster(48, unavailable=U)
    mixed_node_class(nodes)
    job = full_job(5, spreads=TARGET)
    job.task_groups[0].tasks[0].network = NetworkResource(mbits=100, dynamic_ports=1)
    allocs = [Allocation(nodes[perm[p]].id, "other-job", "cache", cpu_shares=3700, memory_mb=256) for p in (1, 4, 11)]
    allocs += [Allocation(nodes[perm[p]].id, "other-job", "cache", cpu_shares=100, memory_mb=64, net_mbits=950)
               for p in (3, 6, 13)]
    return FullCase("full_nodes", nodes, perm, volumes, node_volumes, job, allocs, count=5)


def large_tables_case():
    """test_csi_place_full's 4200-value spread: the tables live in HBM (pset_g_tab)."""
    n, U = 4200, (3, 700, 701, 4199)
    nodes, perm, volumes, node_volumes = dc_cluster(n, unavailable=U, dcs=("dc1",))
    for k, nd in enumerate(nodes):
        nd.meta["unique.slot"] = "s%05d" % k         # (unique.*: not in the computed class)
        nd.compute_class()
    assert len({nd.computed_class for nd in nodes}) == 1
    job = full_job(3, spreads=[Spread("${meta.unique.slot}", 100, [])])
    return FullCase("large_tables", nodes, perm, volumes, node_volumes, job,
                    job_allocs(nodes, perm, job, (0, 1, 2, 5, 6)), count=3, check_plan=False)


RANDOM_PARAMS = [(n, idx) for n in (63, 130) for idx in RANDOM_INDICES]
BUILDERS = {}
for _k in range(len(SPREAD_CASES)):
    for _w in ("target", "even"):
        BUILDERS["spread%d_%s" % (_k, _w)] = (spread_case, _k, _w)
for _k in range(len(SHAPES)):
    BUILDERS["shape%d" % _k] = (shape_case, _k)
for _n, _i in RANDOM_PARAMS:
    BUILDERS["random%d_%d" % (_n, _i)] = (random_case, _n, _i)
BUILDERS.update(affinity=(affinity_case,), tie_wins=(tie_case, True), tie_loses=(tie_case, False),
                latched=(latched_case,), unmemoised=(unmemoised_case,), per_alloc=(per_alloc_case,),
                full_nodes=(full_nodes_case,), overfull=(overfull_case,))
# the CPU test walks BUILDERS; these run on the GPU alone (their references take seconds)
GPU_ONLY = {"block-1": (block_case, -1), "block+1": (block_case, 1), "large_tables": (large_tables_case,)}
_REFS = {}


def reference(name):
    """(case, Ref, want records, want maps), computed once per case."""
    if name in _REFS:
        return _REFS[name]
    from oracle.oracle import OracleGenericStack
    b = BUILDERS.get(name) or GPU_ONLY[name]
    case = b[0](*b[1:])
    probe = OracleGenericStack()
    probe.SetState(case.nodes, [])
    probe.SetJob(plain(case.job))
    known = memoised(case.nodes) if case.memo else {}
    cursor = case.cursor_after_sibling if case.sibling_first else case.cursor
    ref = Ref(case.nodes, case.perm, case.job, case.allocs, UNBOUNDED, cursor=cursor, known=known,
              job_fail=case.job_fail)
    if case.escaped_tg:
        ref.known = NeverKnown()
    want = ref.run(case.count, lambda i: set(case.codes(i)))
    # the maps: the oracle with metrics on over each window without the rows the checker fails
    o = OracleGenericStack()
    o.SetState(case.nodes, case.allocs)
    o.EnableMetrics(True)
    o.SetJob(plain(case.job))
    if case.memo:
        o.PutEligibility(class_elig(case.nodes))
    reaches = {}
    n, cur, maps = len(case.perm), cursor, []
    for k, w in enumerate(want):
        window = [case.perm[(cur + j) % n] for j in range(w["nodes_evaluated"])]
        failing = case.codes(k)
        removed = [r for r in window if r in failing and r not in case.job_fail and passes_checks(probe, reaches, r)]
        o.SetNodes([r for r in window if r not in removed])
        o.SetCursor(0, 0x7FFFFFFF)
        o.SelectRaw(0)                       # (its row is not asserted: see the module's text)
        m = o.LastMetrics()
        for r in removed:
            nd = case.nodes[r]
            if nd.node_class:
                m["ClassFiltered"][nd.node_class] = m["ClassFiltered"].get(nd.node_class, 0) + 1
            text = case.text(k, r)
            m["ConstraintFiltered"][text] = m["ConstraintFiltered"].get(text, 0) + 1
        maps.append(m)
        if w["row"] >= 0:
            o.Commit(0, w["row"])
        cur = w["new_offset"]
    _REFS[name] = (case, ref, want, maps)
    return _REFS[name]


# ---- CPU: the entry exists, and the inputs reach every case the GPU tests rely on ---------------

def test_binding_and_header_declare_the_entry():
    from nomad_amd.stack import GenericStack
    assert "pe_place_csi_full_metrics" in abi.ENGINE_SYMBOLS
    assert callable(getattr(GenericStack, "PlaceCSIFullMetrics", None))
    with open(HEADER) as fh:
        text = fh.read()
    assert "int pe_place_csi_full_metrics(pe_stack* s, uint32_t tg_index, uint32_t count, const uint32_t* alloc_idx," \
        in text
    lib = C.CDLL(LIB)
    assert hasattr(lib, "pe_place_csi_full_metrics")


def test_reference_reaches_every_case():
    kinds, reasons, dims, named = set(), set(), set(), {}
    four_stops = whole = wraps = final_one = evicts = tie = exhausted = classed = unclassed = False
    for name in BUILDERS:
        case, ref, want, maps = reference(name)
        n = len(case.perm)
        assert len(maps) == len(want) == len(ref.traces)
        cur = case.cursor_after_sibling if case.sibling_first else case.cursor
        for k, (w, m) in enumerate(zip(want, maps)):
            kinds |= set(ref.traces[k])
            four_stops = four_stops or ref.stops[k] >= 4
            whole = whole or (w["nodes_evaluated"] == n and n > 1)
            wraps = wraps or cur + w["nodes_evaluated"] > n
            hits = 0
            for r, code in case.codes(k).items():
                if case.text(k, r) in m["ConstraintFiltered"]:
                    reasons.add(code & 7)
                    hits += m["ConstraintFiltered"][case.text(k, r)]
                    classed = classed or bool(case.nodes[r].node_class)
                    unclassed = unclassed or not case.nodes[r].node_class
            if k == len(want) - 1 and k > 0 and w["row"] < 0 and w["nodes_evaluated"] == 1:
                final_one = final_one or (hits == 1 and sum(m["ConstraintFiltered"].values()) == 1)
            options = w["nodes_evaluated"] - w["nodes_filtered"] - w["nodes_exhausted"]
            evicts = evicts or (options > 5 and len(m["ScoreMetaData"]) == 5)
            norms = [x[1] for x in m["ScoreMetaData"]]
            tie = tie or len(set(norms)) < len(norms)
            for x in m["ScoreMetaData"]:
                for scorer, v in x[2].items():
                    if v != 0.0:
                        named[scorer] = True
            exhausted = exhausted or w["nodes_exhausted"] > 0
            dims |= set(m["DimensionExhausted"])
            assert sum(m["DimensionExhausted"].values()) == w["nodes_exhausted"]
            cur = w["new_offset"]
    assert kinds >= {'pop', 'dup', 'nilD'}
    assert four_stops and whole and wraps and final_one and evicts and tie and exhausted
    assert named.get("allocation-spread") and named.get("node-affinity")
    assert {"cpu", "network: bandwidth exceeded"} <= dims
    assert reasons == {1, 2, 3, 4, 5, 6, 7}
    assert classed and unclassed
    # per_alloc: the records of index 1 fail on plugin bar, those of index 0 on nothing
    _, _, pwant, pmaps = reference("per_alloc")
    assert len(pwant) >= 3
    assert any(k.startswith("CSI plugin bar is missing from client") for k in csi_keys(pmaps[1:2]))
    assert not csi_keys(pmaps[0:1]) and not csi_keys(pmaps[2:3])


# ---- GPU: parity --------------------------------------------------------------------------------

def run_case(name):
    """PlaceCSIFullMetrics against Ref and the maps' reference, and against
    PlaceCSIFull on a handle with metrics off: records, cursor with limit,
    Eligibility(), the plain sibling's next Select."""
    from nomad_amd.stack import EngineError
    case, ref, want, maps = reference(name)
    e, f = case.engine(True), case.engine(False)
    before = e.csi_avail_launches()
    got = e.PlaceCSIFullMetrics(0, case.count, alloc_idx=case.alloc_idx)
    launches = e.csi_avail_launches() - before
    got_maps = e.PlaceCSIMaps()
    assert_records(got, want)
    assert len(got_maps) == len(want)
    for k, (gm, wm) in enumerate(zip(got_maps, maps)):
        assert gm == wm, (name, k)
    with pytest.raises(EngineError):          # as after the other batched metrics calls
        e.LastMetrics()
    plain_got = f.PlaceCSIFull(0, case.count, alloc_idx=case.alloc_idx)
    assert len(plain_got) == len(got)
    for g, p in zip(got, plain_got):
        same_record(g, p)
        assert list(g.scores) == list(p.scores)
    assert e.GetCursor() == f.GetCursor() and e.GetCursor()[1] == UNBOUNDED
    assert e.Eligibility() == f.Eligibility()
    if case.ref_elig and not case.escaped_tg:
        assert e.GetCursor() == (ref.cursor, UNBOUNDED)
        ee, re_ = e.Eligibility(), ref.eligibility()
        if case.sibling_first:            # (the sibling's own Select memoised its group as well)
            ee["tgs"].pop("plain")
        assert ee["tgs"] == re_["tgs"] and ee["job"] == re_["job"]
    if case.check_plan:
        e.SetNodes(case.perm)
        f.SetNodes(case.perm)
        same_record(e.SelectRaw(1), f.SelectRaw(1))      # the plan and the spread counts, through the sibling's Select
    return case, launches, got_maps


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["target", "even"])
@pytest.mark.parametrize("k", range(len(SPREAD_CASES)))
def test_spread_cases(k, which):
    run_case("spread%d_%s" % (k, which))


@pytest.mark.gpu
def test_negative_affinity_many_non_positive_options_and_stops():
    case, _, maps = run_case("affinity")
    _, ref, _, _ = reference("affinity")
    assert any('pop' in t for t in ref.traces) and sum(ref.stops) >= 7
    assert any(x[2].get("node-affinity", 0.0) != 0.0 for m in maps for x in m["ScoreMetaData"])


@pytest.mark.gpu
@pytest.mark.parametrize("wins", [True, False])
def test_popped_option_tie(wins):
    name = "tie_wins" if wins else "tie_loses"
    case, _, _ = run_case(name)
    _, ref, want, _ = reference(name)
    assert 'pop' in ref.traces[0] and want[0]["row"] == case.perm[0 if wins else 3] and want[0]["final_score"] <= 0.0


@pytest.mark.gpu
def test_limit_latched_by_the_sibling_group_with_metrics_on():
    run_case("latched")
    _, ref, _, _ = reference("latched")
    assert sum(ref.stops) >= 1 and any(t for t in ref.traces)


# ---- GPU: shapes --------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_shapes(k):
    case, _, maps = run_case("shape%d" % k)
    _, _, want, _ = reference(case.name)
    n, _, _, cursor, _ = SHAPES[k]
    if cursor:
        assert cursor + want[0]["nodes_evaluated"] > n          # the wrap inside the first Select


@pytest.mark.gpu
def test_count_larger_than_what_fits_ends_in_a_nil_record_with_maps():
    case, _, maps = run_case("overfull")
    _, _, want, _ = reference("overfull")
    assert len(want) < 40 and want[-1]["row"] < 0 and len(maps) == len(want)
    assert sum(maps[-1]["DimensionExhausted"].values()) == want[-1]["nodes_exhausted"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-1, 1])
def test_shapes_around_the_block(delta):
    case, _, _ = run_case("block%+d" % delta)
    _, _, want, _ = reference(case.name)
    assert sum(w["nodes_evaluated"] for w in want) > len(case.perm)     # log offsets pass the list length


# ---- GPU: memo and classes ----------------------------------------------------------------------

@pytest.mark.gpu
def test_class_decided_during_the_call():
    run_case("unmemoised")
    _, ref, want, _ = reference("unmemoised")
    assert sum(ref.stops) >= 1 and want[0]["nodes_filtered"] > ref.stops[0]


@pytest.mark.gpu
@pytest.mark.parametrize("n,idx", RANDOM_PARAMS)
def test_escaped_group_over_random_clusters(n, idx):
    case, launches, maps = run_case("random%d_%d" % (n, idx))
    _, ref, want, _ = reference(case.name)
    assert launches <= 2                 # the distinct record sets of [idx, 5, idx], and no more
    assert sum(ref.stops) == 0 and all(w["nodes_evaluated"] == n for w in want)      # never a stop


@pytest.mark.gpu
def test_every_reason_text_over_the_random_clusters():
    reasons = set()
    for n, idx in RANDOM_PARAMS:
        case, _, _, maps = reference("random%d_%d" % (n, idx))
        for k, m in enumerate(maps):
            reasons |= {code & 7 for r, code in case.codes(k).items() if case.text(k, r) in m["ConstraintFiltered"]}
    assert reasons == {1, 2, 3, 4, 5, 6, 7}


# ---- GPU: record sets, exhaustion, large tables ---------------------------------------------------

@pytest.mark.gpu
def test_per_alloc_sources_two_record_sets():
    case, launches, maps = run_case("per_alloc")
    assert launches == 2                 # the distinct sets, and no more
    assert any(k.startswith("CSI plugin bar is missing from client") for k in csi_keys(maps[1:2]))
    assert not csi_keys(maps[0:1])


@pytest.mark.gpu
def test_full_nodes_and_network_ask_under_a_spread():
    _, _, maps = run_case("full_nodes")
    dims = {k for m in maps for k in m["DimensionExhausted"]}
    assert {"cpu", "network: bandwidth exceeded"} <= dims
    assert any(x[2].get("allocation-spread", 0.0) != 0.0 for m in maps for x in m["ScoreMetaData"])


@pytest.mark.gpu
def test_spread_tables_beyond_the_lds_budget():
    case, _, _ = run_case("large_tables")
    _, ref, want, _ = reference("large_tables")
    assert sum(ref.stops) >= 2 and sum(w["nodes_evaluated"] for w in want) > len(case.perm)


# ---- GPU: forwarding ----------------------------------------------------------------------------

@pytest.mark.gpu
def test_metrics_off_is_place_csi_full_and_has_no_maps():
    from nomad_amd.stack import EngineError
    case, _, want, _ = reference("spread1_target")
    e, f = case.engine(False), case.engine(False)
    got, plain_got = e.PlaceCSIFullMetrics(0, case.count), f.PlaceCSIFull(0, case.count)
    assert_records(got, want)
    for g, p in zip(got, plain_got):
        same_record(g, p)
        assert list(g.scores) == list(p.scores)
    assert e.GetCursor() == f.GetCursor() and e.Eligibility() == f.Eligibility()
    with pytest.raises(EngineError) as err:
        e.PlaceCSIMaps()
    assert err.value.code == abi.PE_ESTATE
    # the maps of a metrics call go with the next placing or state call
    m = case.engine(True)
    m.PlaceCSIFullMetrics(0, case.count)
    assert len(m.PlaceCSIMaps()) == len(want)
    m.SetNodes(case.perm)
    with pytest.raises(EngineError):
        m.PlaceCSIMaps()


@pytest.mark.gpu
def test_windowed_group_is_place_csi_metrics():
    from nomad_amd.stack import EngineError
    U, P = (1, 9, 13), (5, 8, 11)
    nodes, perm, volumes, node_volumes = dc_cluster(48, unavailable=U, dcs=("dc1",))
    job = full_job(4)
    allocs = job_allocs(nodes, perm, job, P)
    hs = []
    for _ in range(2):
        h = engine_with(nodes, volumes, node_volumes, job, perm, allocs=allocs)
        h.EnableMetrics(True)
        h.PutEligibility(class_elig(nodes))
        hs.append(h)
    e, f = hs
    got, want = e.PlaceCSIFullMetrics(0, 4), f.PlaceCSIMetrics(0, 4)
    assert len(got) == len(want) >= 2
    for g, w in zip(got, want):
        same_record(g, w)
        assert list(g.scores) == list(w.scores)
    assert e.PlaceCSIMaps() == f.PlaceCSIMaps()
    assert e.GetCursor() == f.GetCursor() and e.GetCursor()[1] < UNBOUNDED
    assert e.Eligibility() == f.Eligibility()
    with pytest.raises(EngineError):
        e.LastMetrics()


# ---- GPU: refusals ------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals_leave_the_handle_untouched():
    from nomad_amd.stack import Unsupported
    nodes, perm, volumes, node_volumes = dc_cluster(48, unavailable=(0, 5))
    n = len(perm)

    def refused(job, match, count=3, tg=0, other=1, allocs=(), stop=()):
        hs = []
        for metrics in (True, False):
            h = engine_with(nodes, volumes, node_volumes, job, perm, allocs=allocs)
            h.EnableMetrics(metrics)
            if stop:
                h.StopAllocs(stop)
            hs.append(h)
        e, f = hs
        cursor, elig = e.GetCursor(), e.Eligibility()
        with pytest.raises(Unsupported, match=match):
            if count > 64:      # refused before anything is written: no record buffer of that size
                out, placed = (abi.pe_ranked_node * 1)(), C.c_uint32(0)
                e._check(e._lib.pe_place_csi_full_metrics(e._h, tg, count, None, out, C.byref(placed)))
            else:
                e.PlaceCSIFullMetrics(tg, count)
        e.EnableMetrics(False)           # (the next Select of the plain group, on both handles alike)
        assert_untouched(e, f, cursor, elig, tg=other)
        e.EnableMetrics(True)
        return e

    job = full_job(3, spreads=TARGET)
    # distinct_property, alone and beside a spread
    dp = full_job(3)
    dp.task_groups[0].constraints = [Constraint("${node.datacenter}", "2", "distinct_property")]
    refused(dp, "distinct_property")
    dps = full_job(3, spreads=TARGET)
    dps.task_groups[0].constraints = [Constraint("${node.datacenter}", "2", "distinct_property")]
    refused(dps, "distinct_property")
    # a spread whose values plan stops clear (Plan.AppendStoppedAlloc of an alloc of the group)
    refused(job, "plan stops", allocs=job_allocs(nodes, perm, job, (1, 2)), stop=[0])
    # static ports
    st = full_job(3, spreads=TARGET)
    st.task_groups[0].network = NetworkResource(mode="host", dynamic_ports=1, reserved_ports=[8080],
                                                port_labels=["http"], host_network="default")
    refused(st, "static port")
    # reserved cores
    cores = full_job(3, spreads=TARGET)
    cores.task_groups[0].tasks[0].cores = 2
    refused(cores, "reserved cores")
    # two groups of one name
    twins = full_job(3, spreads=TARGET)
    twins.task_groups.append(TaskGroup(name="web", count=1, tasks=[Task(name="web", cpu=300, memory_mb=128)]))
    refused(twins, "one name")
    # the log cap: count * len(list) above 2^24, compared in 64 bits; the shadow memo did not move,
    # so the call is answered afterwards
    refused(job, "trace log", count=abi.PE_CSI_LOG_CAP // n + 1)
    refused(job, "trace log", count=(1 << 31) + 5)
    e = refused(job, "trace log", count=0xFFFFFFFF)
    e.PutEligibility(class_elig(nodes))
    got = e.PlaceCSIFullMetrics(0, 3)
    assert len(e.PlaceCSIMaps()) == len(got) >= 1
    # a group without CSI requests while metrics are on
    refused(job, "without CSI requests", tg=1, other=1)


@pytest.mark.gpu
def test_network_ask_on_multi_device_nodes_is_refused_untouched():
    from nomad_amd.stack import Unsupported
    from test_multi_nic import nic_cluster, nic_job
    nodes, allocs = nic_cluster(64, seed=77, two_nic=0.5)
    for nd in nodes[1:]:
        nd.csi_node_plugins = {"foo": CSINodePlugin(True)}
    perm = [int(x) for x in synth.shuffle(64, 78)]
    volumes = [CSIVolume("vol", NS, "foo")]
    job = nic_job(200, count=3, job_id="csi-nic")
    job.task_groups[0].csi_volumes = list(STOP_REQS)
    job.task_groups[0].spreads = list(EVEN)
    job.task_groups.append(TaskGroup(name="plain", count=1, tasks=[Task(name="plain", cpu=300, memory_mb=128)]))
    e = engine_with(nodes, volumes, {}, job, perm, allocs=allocs)
    f = engine_with(nodes, volumes, {}, job, perm, allocs=allocs)
    e.EnableMetrics(True)
    cursor, elig = e.GetCursor(), e.Eligibility()
    with pytest.raises(Unsupported, match="multi-device nodes"):
        e.PlaceCSIFullMetrics(0, 3)
    e.EnableMetrics(False)
    assert_untouched(e, f, cursor, elig)


@pytest.mark.gpu
def test_existing_entries_still_refuse_with_metrics_on():
    from nomad_amd.stack import Unsupported
    case, _, _, _ = reference("spread0_target")
    e = case.engine(True)
    cursor, elig = e.GetCursor(), e.Eligibility()
    with pytest.raises(Unsupported, match="pe_set_metrics"):
        e.PlaceCSIFull(0, 3)
    with pytest.raises(Unsupported, match="full passes"):
        e.PlaceCSIMetrics(0, 3)
    with pytest.raises(Unsupported, match="pe_set_metrics"):
        e.SelectRaw(0)
    assert e.GetCursor() == cursor and e.Eligibility() == elig
