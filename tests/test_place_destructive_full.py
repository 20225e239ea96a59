"""pe_place_destructive_full: computePlacements' loop over its `destructive`
list (generic_sched.go:493-649) in one call for a task group that runs full
passes: node affinities, spreads, or a limit that a sibling group's Select
latched to MaxInt32.

The yardstick is the oracle driven through place_destructive_by_select, the
per-call sequence; records are compared with test_plan_stops' `_key`: equal, not
close. For later state the yardstick is a second engine handle that ran the
sequence. Every scenario first shows, on the oracle alone, that it tests the
interleaving: its records differ from those of the same loop with no stops and
from those with every stop applied up front.

`destructive_spread_model` restates the spread counts each Select sees in closed
form (ks by the winner's value, kc by the stopped alloc's value); the CPU tests
pin it against the oracle's allocation-spread scores before any GPU is involved."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest

from nomad_amd import abi, synth
from nomad_amd.stack import place_destructive_by_select, place_destructive_metrics_by_select
from nomad_amd.structs import (Affinity, Allocation, Constraint, CSIVolumeRequest, Spread, SpreadTarget, Task,
                               TaskGroup)
from tests.test_inplace_update_spread import _even_boost, _node_value
from tests.test_place_destructive import (NIL_AT, Scenario, _count_loop, _devices, _job_with_own_allocs, _keys, _mixed,
                                          _nil)
from tests.test_plan_stops import _key

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nomad_pe.h")
LIB = os.path.join(ROOT, "nomad_amd", "libnomadpe.so")

CAPACITY = 8192        # k_destructive_full's LDS entries
BLOCK = 1024           # its workgroup
MAX_UPDATES = 4096     # updates of one call
MAXINT32 = 2147483647
LENGTHS = (1, 2, 63, 64, 65, 150)

TARGET = Spread("${node.class}", 60, [SpreadTarget("class-1", 40), SpreadTarget("class-2", 30)])
EVEN = Spread("${node.class}", 50, [])
AFFINITY = Affinity("${node.class}", "class-3", "=", 50)


def _target(job):
    job.task_groups[0].spreads = [copy.deepcopy(TARGET)]


def _even(job):
    job.task_groups[0].spreads = [copy.deepcopy(EVEN)]


def _aff(job):
    job.task_groups[0].affinities = [copy.deepcopy(AFFINITY)]


KINDS = {"target": _target, "even": _even, "aff": _aff}


# ---- scenarios --------------------------------------------------------------------

def _length(n, kind):
    own = 48 if n >= 8 else 2 * n + 1
    nodes, allocs, job, own_idx = _job_with_own_allocs(n, own, seed=300 + n, tight=0.5 if n >= 8 else 1.0)
    KINDS[kind](job)
    return Scenario(nodes, allocs, job, synth.shuffle(n, n + 3), own_idx[:48])


def _around_block(n):
    """An even spread on a list whose option count lies just above (n = 1080)
    or just below (n = 1060) the kernel's block of 1024 threads."""
    nodes, allocs, job, own_idx = _job_with_own_allocs(n, 64, seed=480 + n, tight=0.5)
    _even(job)
    return Scenario(nodes, allocs, job, synth.shuffle(n, 5), own_idx[:24])


def _nonpositive():
    """Every option scores at most 0 (an anti-affinity every node matches): each Select takes the skip rule."""
    nodes, allocs, job, own_idx = _job_with_own_allocs(150, 48, seed=411, tight=0.5)
    job.task_groups[0].affinities = [Affinity("${node.class}", "nope", "!=", -100)]
    return Scenario(nodes, allocs, job, synth.shuffle(150, 412), own_idx[:48])


def _distinct_hosts():
    """distinct_hosts with an affinity: every node that holds an own alloc is
    filtered until that alloc's stop, and every placement filters its node."""
    nodes, allocs, job, own_idx = _job_with_own_allocs(100, 60, seed=421, tight=0.5)
    job.task_groups[0].constraints = [Constraint("", "", "distinct_hosts")]
    _aff(job)
    return Scenario(nodes, allocs, job, synth.shuffle(100, 422), own_idx[:48])


def _two_levels():
    """A target spread at job level on an attribute a third of the nodes lack
    (the -1 boost) and an even spread at group level: two weight fractions."""
    nodes, allocs, job, own_idx = _job_with_own_allocs(150, 48, seed=431, tight=0.5)
    for k, nd in enumerate(nodes):
        if k % 3:
            nd.meta["zone"] = "z%d" % (k % 4)
            nd.compute_class()
    job.spreads = [Spread("${meta.zone}", 70, [SpreadTarget("z1", 50), SpreadTarget("z2", 30)])]
    _even(job)
    return Scenario(nodes, allocs, job, synth.shuffle(150, 432), own_idx[:48])


def _mixed_target():
    sc = _mixed()
    _target(sc.job)
    return sc


def _nil_even():
    sc = _nil()
    _even(sc.job)
    return sc


def _sibling(job):
    job.task_groups.append(TaskGroup(name="side", count=1, spreads=[Spread("${node.class}", 50, [])],
                                     tasks=[Task(name="side", driver="exec", cpu=100, memory_mb=64)]))


def _latch(st):
    """A Select and a commit of the sibling group with a spread: the limit stays MaxInt32 from then on."""
    r = st.SelectRaw(1)
    assert r.row >= 0
    st.Commit(1, r.row)


def _latched():
    nodes, allocs, job, own_idx = _job_with_own_allocs(150, 48, seed=441, tight=0.5)
    _sibling(job)
    return Scenario(nodes, allocs, job, synth.shuffle(150, 442), own_idx[:48], prep=_latch)


def _devices_aff():
    sc = _devices()
    sc.job.task_groups[0].affinities = [Affinity("${node.class}", "nope", "!=", 40)]
    return sc


def _other_group():
    """Three listed allocs belong to another group of the job (their nodes stay in that group's column)."""
    nodes, allocs, job, own_idx = _job_with_own_allocs(150, 48, seed=451, tight=0.5)
    _target(job)
    job.task_groups.append(TaskGroup(name="api", count=3, tasks=[Task(name="api", driver="exec", cpu=500,
                                                                        memory_mb=256)]))
    upd = own_idx[:40]
    for ai in (upd[3], upd[11], upd[12]):
        allocs[ai].task_group = "api"
    return Scenario(nodes, allocs, job, synth.shuffle(150, 452), upd)


def _off_list():
    """Four listed allocs sit on nodes that the node list does not name."""
    nodes, allocs, job, own_idx = _job_with_own_allocs(150, 48, seed=461, tight=0.5)
    _target(job)
    upd = own_idx[:40]
    by_id = {nd.id: k for k, nd in enumerate(nodes)}
    drop = {by_id[allocs[ai].node_id] for ai in (upd[2], upd[7], upd[8], upd[30])}
    perm = [int(r) for r in synth.shuffle(150, 462) if int(r) not in drop]
    return Scenario(nodes, allocs, job, perm, upd)


def _windowed():
    nodes, allocs, job, own_idx = _job_with_own_allocs(150, 48, seed=471, tight=0.5)
    return Scenario(nodes, allocs, job, synth.shuffle(150, 472), own_idx[:48])


SCENARIOS = {"above-block": lambda: _around_block(1080), "below-block": lambda: _around_block(1060),
             "nonpositive": _nonpositive, "distinct-hosts": _distinct_hosts, "two-levels": _two_levels,
             "mixed": _mixed_target, "nil": _nil_even, "latched": _latched, "devices": _devices_aff,
             "other-group": _other_group, "off-list": _off_list}
for _n in LENGTHS:
    for _k in KINDS:
        SCENARIOS["len%d-%s" % (_n, _k)] = functools.partial(_length, _n, _k)


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


def _options(key):
    return key[3] - key[4] - key[5]        # nodes_evaluated - nodes_filtered - nodes_exhausted


# ---- the spread counts in closed form -----------------------------------------------

def destructive_spread_model(nodes, allocs, job, tg, upd, winners, plan_nodes=(), stopped=()):
    """The allocation-spread part of each update's winner (`winners`: the
    records' rows by list position, -1 ends the loop) from the state at the
    call's start (`plan_nodes`: node ids of the plan's allocs of the group;
    `stopped`: alloc indices in NodeUpdate). Per spread set and value u, the
    Select of update i sees

        Craw    = Craw0[u] + kc[u] + (1 if update i's stopped alloc sits on u and passes the test)
        cleared = Craw - (1 if (prop0[u] or ks[u] > 0) and Craw > 1 else 0)
        count   = EP0[u] + ks[u] - cleared, not below 0

    where ks counts earlier placements by the *winner's* value and kc earlier
    updates by the *stopped* alloc's value (job, namespace and group test,
    terminal and re-stopped allocs included)."""
    g = job.task_groups[tg]
    by_id = {n.id: n for n in nodes}
    specs = list(job.spreads) + list(g.spreads)
    info = {}
    for sp in list(g.spreads) + list(job.spreads):
        info[sp.attribute] = sp
    wsum = sum(sp.weight for sp in specs)

    def mine(a):
        return a.job_id == job.id and a.namespace == job.namespace and a.task_group == g.name

    sets = []
    for sp in specs:
        ep0, craw0, prop0 = {}, {}, set()
        for a in allocs:
            v = _node_value(by_id[a.node_id], sp.attribute)
            if mine(a) and not a.terminal and v is not None:
                ep0[v] = ep0.get(v, 0) + 1
        for nid in plan_nodes:
            v = _node_value(by_id[nid], sp.attribute)
            if v is not None:
                ep0[v] = ep0.get(v, 0) + 1
                prop0.add(v)
        for ai in stopped:
            v = _node_value(by_id[allocs[ai].node_id], sp.attribute)
            if mine(allocs[ai]) and v is not None:
                craw0[v] = craw0.get(v, 0) + 1
        si = info[sp.attribute]
        total = float(g.count)
        desired, dsum = {}, 0.0
        for t in si.targets:
            d = (float(t.percent) / float(100)) * total
            desired[t.value] = d
            dsum += d
        star = desired.get("*")
        if 0 < dsum < total:
            star = total - dsum
        values = {_node_value(n, sp.attribute) for n in nodes} - {None}
        sets.append(dict(sp=sp, ep0=ep0, craw0=craw0, prop0=prop0, desired=desired, star=star, values=values,
                         frac=float(si.weight) / float(wsum), even=not si.targets, ks={}, kc={}))

    parts, seen = [], []
    for ai, row in zip(upd, winners):
        a = allocs[ai]
        own = mine(a)
        if row < 0:
            break
        total = 0.0
        for s in sets:
            vi = _node_value(by_id[a.node_id], s["sp"].attribute)
            wi = _node_value(nodes[row], s["sp"].attribute)

            def count(u):
                ks = s["ks"].get(u, 0)
                ep = s["ep0"].get(u, 0) + ks
                craw = s["craw0"].get(u, 0) + s["kc"].get(u, 0) + (1 if (u == vi and own) else 0)
                seen.append((craw, u in s["prop0"]))
                cleared = craw - (1 if ((u in s["prop0"] or ks > 0) and craw > 1) else 0)
                return ep - cleared if ep >= cleared else 0

            if wi is None:
                b = -1.0
            elif s["even"]:
                used = [c for c in (count(u) for u in sorted(s["values"])) if c > 0]
                b = _even_boost(min(used) if used else 0, max(used) if used else 0, len(used), count(wi))
            else:
                d = s["desired"].get(wi, s["star"])
                b = -1.0 if d is None else ((d - float(count(wi) + 1)) / d) * s["frac"]
            total += b
            if wi is not None:
                s["ks"][wi] = s["ks"].get(wi, 0) + 1
            if own and vi is not None:
                s["kc"][vi] = s["kc"].get(vi, 0) + 1
        parts.append(total)
    return parts, seen


def _oracle_spread_parts(sc, before=None):
    """The oracle's interleaved loop with its maps on: per placed record the
    winner's row and its `allocation-spread` score (0.0 when not appended)."""
    st = sc.oracle()
    if before:
        before(st)
    st.EnableMetrics(True)
    recs, maps = place_destructive_metrics_by_select(st, 0, sc.upd)
    rows, parts = [], []
    for r, m in zip(recs, maps):
        rows.append(r.row)
        if r.row < 0:
            break
        named = [x[2] for x in m["ScoreMetaData"] if x[0] == sc.nodes[r.row].id]
        assert len(named) == 1, "the winner is not in the record's top scores"
        parts.append(named[0].get("allocation-spread", 0.0))
    return rows, parts


# ---- CPU, no device ---------------------------------------------------------------

def test_header_library_and_binding_declare_the_entry():
    from nomad_amd.stack import GenericStack
    assert "pe_place_destructive_full" in abi.ENGINE_SYMBOLS
    assert callable(getattr(GenericStack, "PlaceDestructiveFull", None))
    with open(HEADER) as fh:
        text = fh.read()
    assert "int pe_place_destructive_full(pe_stack* s, uint32_t tg_index, const uint32_t* allocs, uint32_t n, " \
           "pe_ranked_node* out,\n                              uint32_t* placed);" in text
    assert hasattr(C.CDLL(LIB), "pe_place_destructive_full")


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario_tests_the_interleaving(name):
    sc, inter, none, front = reference(name)
    assert len(sc.upd) == len(set(sc.upd)) and len(sc.upd) >= 1
    assert sum(1 for a, b in zip(inter, none) if a != b) >= 1 or len(inter) != len(none), \
        "the loop with no stops gives the same records"
    assert sum(1 for a, b in zip(inter, front) if a != b) >= 1 or len(inter) != len(front), \
        "all stops up front give the same records"
    assert sum(1 for k in inter if k[0] >= 0) >= 1
    assert all(k[3] == len(sc.perm) and k[6] == 0 for k in inter)      # full passes, the cursor stays


def test_block_scenarios_lie_on_either_side_of_the_block():
    _, above, _, _ = reference("above-block")
    _, below, _, _ = reference("below-block")
    assert len(above) == len(below) == 24
    assert all(1032 <= _options(k) <= 1038 for k in above), [_options(k) for k in above]
    assert all(1000 <= _options(k) < BLOCK for k in below), [_options(k) for k in below]


def test_nonpositive_scenario_takes_the_skip_rule_every_time():
    _, inter, _, _ = reference("nonpositive")
    assert len(inter) == 48 and all(k[0] >= 0 and k[1] <= 0.0 for k in inter)


def test_distinct_hosts_scenario_swaps_a_filtered_node_per_update():
    sc, inter, _, _ = reference("distinct-hosts")
    assert len(inter) == 48 and all(k[0] >= 0 for k in inter)
    assert len({k[4] for k in inter}) == 1 and inter[0][4] > 0          # filtered: constant, non-zero
    assert inter[0][4] >= len(sc.upd)                                    # more than the affinity-free classes filter


def test_nil_scenario_runs_out_at_its_update():
    sc, inter, none, front = reference("nil")
    assert len(inter) == NIL_AT + 1 and inter[-1][0] == -1 and all(k[0] >= 0 for k in inter[:-1])


def test_latched_scenario_reads_the_latched_limit():
    sc, inter, _, _ = reference("latched")
    st = sc.oracle()
    assert st.GetCursor()[1] == MAXINT32
    assert not sc.job.task_groups[0].spreads and not sc.job.task_groups[0].affinities and not sc.job.spreads


def test_mixed_and_other_scenarios_hold_their_kinds():
    sc, inter, _, _ = reference("mixed")
    node = [sc.allocs[a].node_id for a in sc.upd]
    assert len(set(node)) < len(node) and sum(1 for a in sc.upd if sc.allocs[a].terminal) == 1
    assert len(inter) == len(sc.upd)
    sc, inter, _, _ = reference("other-group")
    assert sum(1 for a in sc.upd if sc.allocs[a].task_group == "api") == 3 and len(inter) == len(sc.upd)
    sc, inter, _, _ = reference("off-list")
    listed = {sc.nodes[r].id for r in sc.perm}
    assert sum(1 for a in sc.upd if sc.allocs[a].node_id not in listed) == 4 and len(inter) == len(sc.upd)
    sc, inter, _, _ = reference("two-levels")
    assert sum(1 for nd in sc.nodes if "zone" not in nd.meta) == 50
    by_id = {nd.id: nd for nd in sc.nodes}
    assert any("zone" not in by_id[sc.allocs[a].node_id].meta for a in sc.upd)  # a stop on a node without the value


def test_devices_scenario_stops_meet_placements_of_the_call():
    sc, inter, _, _ = reference("devices")
    st = sc.oracle()
    rows = [st.row(sc.allocs[ai].node_id) for ai in sc.upd]
    assert any(rows[i] in {k[0] for k in inter[:i]} for i in range(1, len(inter)))
    assert any(k[8] for k in inter)                                           # device offers


def _before(sc):
    """Earlier stops and commits of the group before the loop: three own allocs
    of one class stopped (Craw0 = 3 there) and two placements committed on
    nodes of that class (prop0 set there)."""
    by_id = {nd.id: nd for nd in sc.nodes}
    cls = {}
    for ai in sc.upd[40:]:
        cls.setdefault(by_id[sc.allocs[ai].node_id].node_class, []).append(ai)
    name, stopped = max(cls.items(), key=lambda kv: len(kv[1]))
    stopped = stopped[:3]
    assert len(stopped) == 3
    placed = []

    def run(st):
        st.StopAllocs(stopped)
        st.SetNodes([k for k, nd in enumerate(sc.nodes) if nd.node_class == name])
        for _ in range(2):
            r = st.SelectRaw(0)
            assert r.row >= 0
            st.Commit(0, r.row)
            placed.append(sc.nodes[r.row].id)
        st.SetNodes(sc.perm)

    return run, stopped, placed


@pytest.mark.parametrize("kind", ["target", "even"])
@pytest.mark.parametrize("earlier", [False, True], ids=["fresh", "earlier"])
def test_destructive_spread_model_equals_the_oracle(kind, earlier):
    nodes, allocs, job, own_idx = _job_with_own_allocs(150, 64, seed=500, tight=0.5)
    KINDS[kind](job)
    sc = Scenario(nodes, allocs, job, synth.shuffle(150, 501), own_idx[:48])
    sc.upd = own_idx[:64]
    run, stopped, placed = _before(sc) if earlier else (None, [], [])
    sc.upd = own_idx[:40] if earlier else own_idx[:48]
    assert not set(stopped) & set(sc.upd)
    rows, want = _oracle_spread_parts(sc, run)
    assert len(want) >= 40
    parts, seen = destructive_spread_model(nodes, allocs, job, 0, sc.upd, rows, plan_nodes=placed, stopped=stopped)
    assert parts == want                                          # == on the doubles
    assert len({round(p, 12) for p in parts}) > 3
    if earlier:
        assert any(craw > 1 and prop for craw, prop in seen)      # Craw0 > 1 with prop0 set


# ---- GPU --------------------------------------------------------------------------

def _parity(name, later=20):
    """Records against the oracle; then cursor, limit and Eligibility against
    the oracle, and a Place of `later` against the oracle and a second handle
    that ran the sequence."""
    sc, inter, _, _ = reference(name)
    a, b, ora = sc.engine(), sc.engine(), sc.oracle()
    got = a.PlaceDestructiveFull(0, sc.upd, fallback=False)
    assert _keys(got) == inter
    assert _keys(place_destructive_by_select(b, 0, sc.upd)) == inter
    place_destructive_by_select(ora, 0, sc.upd)
    assert a.GetCursor() == b.GetCursor() == ora.GetCursor() and a.GetCursor()[1] == MAXINT32
    assert a.Eligibility() == b.Eligibility() == ora.Eligibility()
    if later:
        want = _count_loop(ora, later)
        assert _keys(a.Place(0, later)) == want
        assert _count_loop(b, later) == want
        assert a.Eligibility() == b.Eligibility()
    return sc, got


@gpu
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("n", LENGTHS)
def test_parity_over_list_lengths(n, kind):
    _parity("len%d-%s" % (n, kind))


@gpu
@pytest.mark.parametrize("name", ["above-block", "below-block"])
def test_option_counts_around_the_block(name):
    _parity(name, later=4)


@gpu
def test_nonpositive_maximum_takes_the_skip_rule():
    _parity("nonpositive")


@gpu
def test_distinct_hosts_stops_bring_filtered_nodes_back():
    _parity("distinct-hosts")


@gpu
def test_job_and_group_spreads_with_a_missing_attribute():
    _parity("two-levels")


@gpu
def test_stops_that_share_a_node_or_change_nothing():
    _parity("mixed", later=12)


@gpu
def test_plain_group_under_a_latched_limit():
    sc, _ = _parity("latched")
    assert sc.engine().GetCursor()[1] == MAXINT32


@gpu
def test_device_asks_take_the_returned_instances():
    sc, got = _parity("devices", later=10)
    stopped_rows = [sc.oracle().row(sc.allocs[a].node_id) for a in sc.upd]
    # a stop returns instances: some update's winner is the node just freed, with device offers, and a later
    # stop lands on a row that already holds a placement of the call
    assert any(r.row == row and r.device_offers for r, row in zip(got, stopped_rows))
    assert any(stopped_rows[i] in {r.row for r in got[:i]} for i in range(1, len(got)))


@gpu
def test_listed_alloc_of_another_group_of_the_job():
    sc, inter, _, _ = reference("other-group")
    a, b, ora = sc.engine(), sc.engine(), sc.oracle()
    assert _keys(a.PlaceDestructiveFull(0, sc.upd, fallback=False)) == inter
    for st in (b, ora):
        place_destructive_by_select(st, 0, sc.upd)
    assert a.GetCursor() == b.GetCursor() == ora.GetCursor()
    for tg in (1, 0):                                   # the other group's column, rebuilt from the mirrors
        want = _count_loop_tg(ora, tg, 3)
        assert _count_loop_tg(a, tg, 3) == want and _count_loop_tg(b, tg, 3) == want


def _count_loop_tg(st, tg, k):
    out = []
    for _ in range(k):
        r = st.SelectRaw(tg)
        out.append(_key(r))
        if r.row < 0:
            break
        st.Commit(tg, r.row)
    return out


@gpu
def test_listed_allocs_on_nodes_outside_the_list():
    _parity("off-list")


@gpu
def test_nil_pops_its_stop_and_ends_the_loop():
    sc, inter, _, _ = reference("nil")
    eng, ora = sc.engine(), sc.oracle()
    got = eng.PlaceDestructiveFull(0, sc.upd, fallback=False)
    assert _keys(got) == inter and len(got) == NIL_AT + 1 and got[-1].row == -1
    place_destructive_by_select(ora, 0, sc.upd)
    assert eng.GetCursor() == ora.GetCursor() and eng.Eligibility() == ora.Eligibility()
    # allocs[k] is back in the proposed state: its node answers as the oracle's does, and is full
    row = eng.row(sc.allocs[sc.upd[NIL_AT]].node_id)
    for st in (eng, ora):
        st.PopUpdate(sc.upd[NIL_AT])                    # nothing left to pop
        st.SetNodes([row])
    r = eng.SelectRaw(0)
    assert _key(r) == _key(ora.SelectRaw(0)) and r.row < 0 and r.nodes_exhausted == 1
    for st in (eng, ora):
        st.SetNodes(sc.perm)
    rest = sc.upd[NIL_AT + 1:]
    assert _keys(eng.PlaceDestructiveFull(0, rest, fallback=False)) == \
        _keys(place_destructive_by_select(ora, 0, rest))
    assert _keys(eng.Place(0, 4)) == _count_loop(ora, 4)


@gpu
def test_two_calls_equal_one():
    sc, inter, _, _ = reference("len150-target")
    a, b, ora = sc.engine(), sc.engine(), sc.oracle()
    first = _keys(a.PlaceDestructiveFull(0, sc.upd[:20], fallback=False))
    rest = _keys(a.PlaceDestructiveFull(0, sc.upd[20:], fallback=False))
    assert first + rest == inter
    assert _keys(b.PlaceDestructiveFull(0, sc.upd, fallback=False)) == inter
    place_destructive_by_select(ora, 0, sc.upd)
    assert a.GetCursor() == b.GetCursor() == ora.GetCursor() and a.Eligibility() == b.Eligibility()
    want = _count_loop(ora, 20)
    assert _keys(a.Place(0, 20)) == want and _keys(b.Place(0, 20)) == want


@gpu
def test_windowed_group_forwards_to_place_destructive():
    sc = _windowed()
    a, b, ora = sc.engine(), sc.engine(), sc.oracle()
    got, want = a.PlaceDestructiveFull(0, sc.upd, fallback=False), b.PlaceDestructive(0, sc.upd, fallback=False)
    assert _keys(got) == _keys(want) == _keys(place_destructive_by_select(ora, 0, sc.upd))
    assert len({k[3] for k in _keys(got)}) > 1 and a.GetCursor()[1] < MAXINT32       # windowed Selects
    assert a.GetCursor() == b.GetCursor() and a.Eligibility() == b.Eligibility()
    assert a.place_destructive_stats() == b.place_destructive_stats()
    assert _keys(a.Place(0, 20)) == _keys(b.Place(0, 20)) == _count_loop(ora, 20)


@gpu
def test_counters_do_not_depend_on_n():
    sc, inter, _, _ = reference("len150-even")
    x, y = sc.engine(), sc.engine()
    x.PlaceDestructiveFull(0, sc.upd[:4], fallback=False)
    x.PlaceDestructiveFull(0, sc.upd[4:24], fallback=False)          # 20 updates
    y.PlaceDestructiveFull(0, sc.upd[:4], fallback=False)
    y.PlaceDestructiveFull(0, sc.upd[4:48], fallback=False)          # 44 updates
    t20, t44 = x.place_destructive_stats(), y.place_destructive_stats()
    assert t20 == t44 == (1, 1, 2)      # the launch; the synchronisation; the staged list and the argument copy


def _refusals():
    """name -> (match, job mutation, stack keywords, preparation, cluster mutation)"""
    from tests.test_place_destructive import _refusals as windowed
    rows = {k: v for k, v in windowed().items()
            if k not in ("node affinities", "spreads", "a latched limit", "distinct_property")}

    def with_spread(mutate):
        def both(job):
            _target(job)
            if mutate:
                mutate(job)
        return both

    out = {k: (m, with_spread(mut), kw, prep, cl) for k, (m, mut, kw, prep, cl) in rows.items()}

    def distinct_group(job):
        _target(job)
        job.task_groups[0].constraints = [Constraint("${node.class}", "100", "distinct_property")]

    def distinct_job(job):
        _aff(job)
        job.constraints = list(job.constraints) + [Constraint("${node.class}", "100", "distinct_property")]

    def three_sets(job):
        job.spreads = [Spread("${node.class}", 50, []), Spread("${attr.cpu.arch}", 30, [])]
        job.task_groups[0].spreads = [Spread("${node.datacenter}", 20, [])]

    def wide_set(job):
        job.task_groups[0].spreads = [Spread("${node.unique.name}", 50, [])]

    def many_scores(job):
        # node names are node-00000 .. node-00299: one weight per units, tens and hundreds digit, so that the
        # 300 nodes' weight sums (-99 .. 200) and with them their normalised affinity scores are all distinct
        aff = [Affinity("${node.unique.name}", "%d$" % d, "regexp", d + 1) for d in range(10)]
        aff += [Affinity("${node.unique.name}", "%d[0-9]$" % t, "regexp", 10 * t) for t in range(1, 10)]
        aff += [Affinity("${node.unique.name}", "0[0-9][0-9]$", "regexp", -100),
                Affinity("${node.unique.name}", "2[0-9][0-9]$", "regexp", 100)]
        job.task_groups[0].affinities = aff

    out["more than 256 affinity scores"] = ("folded per-node word", many_scores, {}, None, "wide")
    out["distinct_property in the group"] = ("distinct_property", distinct_group, {}, None, None)
    out["distinct_property in the job"] = ("distinct_property", distinct_job, {}, None, None)
    out["three spread sets"] = ("folded per-node word", three_sets, {}, None, None)
    out["a set of more than 255 values"] = ("folded per-node word", wide_set, {}, None, "wide")
    out["a row named twice"] = ("names a row twice", with_spread(None), {}, None, "twice")
    return out


def _refusal_scenario(case):
    match, mutate, kw, prep, cluster = _refusals()[case]
    n = 300 if cluster == "wide" else 120
    nodes, allocs, job, own_idx = _job_with_own_allocs(n, 24, seed=201)
    upd = own_idx[:16]
    if mutate:
        mutate(job)
    if callable(cluster):
        cluster(nodes, allocs, upd)
    perm = [int(r) for r in synth.shuffle(n, 202)]
    if cluster == "twice":
        perm = perm + perm[:1]
    return match, kw, Scenario(nodes, allocs, job, perm, upd, prep=prep)


@gpu
@pytest.mark.parametrize("case", sorted(_refusals()))
def test_refusals_leave_the_handle_as_it_was(case):
    from nomad_amd.stack import Unsupported
    match, kw, sc = _refusal_scenario(case)
    eng, fresh = sc.engine(**kw), sc.engine(**kw)
    cursor, elig = eng.GetCursor(), eng.Eligibility()
    with pytest.raises(Unsupported, match=match) as err:
        eng.PlaceDestructiveFull(0, sc.upd, fallback=False)
    if case != "the group's own reason":
        assert "pe_place_destructive_full: " in str(err.value)
    assert eng.GetCursor() == cursor and eng.Eligibility() == elig
    try:
        want = _keys(place_destructive_by_select(fresh, 0, sc.upd))
    except Unsupported:
        # the engine's own Select refuses this job too: the refused handle's answer as well
        with pytest.raises(Unsupported):
            place_destructive_by_select(eng, 0, sc.upd)
        return
    # cursor, plan and NodeUpdate untouched: the fallback's sequence answers as a fresh handle's does
    assert _keys(eng.PlaceDestructiveFull(0, sc.upd)) == want
    if not kw and case != "metrics on":
        assert want == _keys(place_destructive_by_select(sc.oracle(), 0, sc.upd))
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
    job = csi_job([CSIVolumeRequest("volume-id")], count=2)
    job.task_groups[0].spreads = [Spread("${node.class}", 50, [])]
    eng = engine_with(nodes, volumes, node_volumes, job, allocs=allocs)
    cursor = eng.GetCursor()
    with pytest.raises(Unsupported, match="pe_place_destructive_full: a group with CSI requests"):
        eng.PlaceDestructiveFull(0, [0], fallback=False)
    assert eng.GetCursor() == cursor


@gpu
def test_refusal_beyond_the_entries_of_one_workgroup():
    # every node of the list is an option: more entries than the kernel's LDS holds. The kernel finds it
    # while it builds its entries, before the first stop is applied
    from nomad_amd.stack import GenericStack, Unsupported
    n = CAPACITY + 8
    nodes, _ = synth.cluster_c2(n, seed=71, other_allocs=False)
    allocs = [Allocation(node_id=nodes[k].id, job_id="svc-c2", task_group="web", cpu_shares=500, memory_mb=256,
                         disk_mb=150, priority=50) for k in (5, 900, 8100)]
    job = synth.job_c2(3)
    job.version = 7
    _aff(job)
    perm = synth.shuffle(n, 72)

    def stack(cls):
        st = cls()
        st.SetState(nodes, allocs)
        st.SetJob(job)
        st.SetNodes(perm)
        return st

    eng, fresh = stack(GenericStack), stack(GenericStack)
    cursor, elig = eng.GetCursor(), eng.Eligibility()
    with pytest.raises(Unsupported, match="pe_place_destructive_full: more options .* LDS holds \\(%d" % CAPACITY):
        eng.PlaceDestructiveFull(0, [0, 1, 2], fallback=False)
    assert eng.GetCursor() == cursor and eng.Eligibility() == elig
    want = _keys(place_destructive_by_select(fresh, 0, [0, 1, 2]))
    assert all(_options(k) > CAPACITY for k in want)
    assert _keys(eng.PlaceDestructiveFull(0, [0, 1, 2])) == want            # no stop had been applied
    assert eng.GetCursor() == fresh.GetCursor() and eng.Eligibility() == fresh.Eligibility()


@gpu
def test_refusal_beyond_the_updates_of_one_call():
    from nomad_amd.stack import GenericStack, Unsupported
    nodes, allocs = synth.cluster_c2(6000, seed=61)
    assert len(allocs) > MAX_UPDATES + 1
    job = synth.job_c2(10)
    _target(job)
    eng = GenericStack()
    eng.SetState(nodes, allocs)
    eng.SetJob(job)
    eng.SetNodes(synth.shuffle(6000, 7))
    cursor = eng.GetCursor()
    lst = np.arange(MAX_UPDATES + 1, dtype=np.uint32)
    out, placed = (abi.pe_ranked_node * 1)(), C.c_uint32(0)    # refused before anything is written
    with pytest.raises(Unsupported, match="pe_place_destructive_full: n exceeds"):
        eng._check(eng._lib.pe_place_destructive_full(eng._h, 0, lst.ctypes.data_as(abi.u32p), len(lst), out,
                                                      C.byref(placed)))
    assert eng.GetCursor() == cursor and placed.value == 0


@gpu
def test_invalid_arguments_change_nothing():
    from nomad_amd.stack import EngineError
    sc, inter, _, _ = reference("len150-target")
    eng = sc.engine()
    cursor, elig = eng.GetCursor(), eng.Eligibility()
    for tg, lst in ((1, sc.upd[:4]), (0, sc.upd[:3] + [len(sc.allocs)]), (0, sc.upd[:3] + [sc.upd[1]])):
        with pytest.raises(EngineError) as err:
            eng.PlaceDestructiveFull(tg, lst, fallback=False)
        assert err.value.code == abi.PE_EINVAL
        assert eng.GetCursor() == cursor and eng.Eligibility() == elig
    assert eng.PlaceDestructiveFull(0, [], fallback=False) == []
    assert eng.GetCursor() == cursor
    lst = np.asarray(sc.upd[:2], dtype=np.uint32)
    assert eng._lib.pe_place_destructive_full(eng._h, 0, lst.ctypes.data_as(abi.u32p), 2, None, None) == abi.PE_EINVAL
    assert _keys(eng.PlaceDestructiveFull(0, sc.upd, fallback=False)) == inter     # nothing had changed


@gpu
@pytest.mark.parametrize("name", ["len150-target", "nil"])
def test_shim_sends_a_destructive_run_through_the_entry(name):
    # the shim's run: the plan and its mirror take what the call did, so the next stack call replays nothing
    from nomad_amd.shim import DeviceStack, Plan
    sc, inter, _, _ = reference(name)
    eng, ora = sc.engine(), sc.oracle()
    shim = DeviceStack(eng, Plan())
    shim.SetJob(sc.job)
    shim.SetNodes(sc.perm)
    if sc.prep:
        sc.prep(eng)
    placed = shim.PlaceDestructive(0, sc.upd)
    want = [k for k in inter if k[0] >= 0]
    assert _keys(placed) == want
    place_destructive_by_select(ora, 0, sc.upd)
    assert sorted(a for lst in shim.plan.node_update.values() for a in lst) == sorted(sc.upd[:len(want)])
    assert sorted(a.node_row for lst in shim.plan.node_allocation.values() for a in lst) == sorted(k[0] for k in want)
    nxt = shim.Select(0)
    assert _key(nxt) == _key(ora.Select(0))
    assert eng.GetCursor() == ora.GetCursor() and eng.Eligibility() == ora.Eligibility()


@gpu
def test_shim_answers_a_refused_run_update_by_update():
    from nomad_amd.shim import DeviceStack, Plan
    match, kw, sc = _refusal_scenario("distinct_property in the group")
    eng, fresh = sc.engine(), sc.engine()
    shim = DeviceStack(eng, Plan())
    shim.SetJob(sc.job)
    shim.SetNodes(sc.perm)
    want = [k for k in _keys(place_destructive_by_select(fresh, 0, sc.upd)) if k[0] >= 0]
    assert _keys(shim.PlaceDestructive(0, sc.upd)) == want and len(want) >= 1
    assert eng.GetCursor() == fresh.GetCursor()
