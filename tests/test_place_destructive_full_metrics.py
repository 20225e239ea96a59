"""pe_place_destructive_full_metrics: computePlacements' destructive-update
loop (generic_sched.go:543-645) in one call for a task group that runs full
passes (node affinities, spreads, a latched limit) with AllocMetric kept
(DESIGN.md §50): per update the maps GenericScheduler stores on the new alloc,
or in failedTGAllocs for the nil Select that ends the loop.

Yardsticks: the oracle with EnableMetrics(True) driven through
place_destructive_metrics_by_select (records and maps), and for later state a
second engine handle that ran that per-call sequence with metrics on. Records
are compared with test_plan_stops' `_key`, maps with `==` on the dicts: equal,
not close. The scenarios are test_place_destructive_full's and one more,
`many-nonoptions`; the CPU tests first show, on the oracle alone, that each of
them tests the stops' effect on the maps and that together they reach the map
kinds the GPU tests are meant to compare."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from nomad_amd import abi, synth
from nomad_amd.stack import place_destructive_metrics_by_select
from nomad_amd.structs import Allocation, Constraint, CSIVolumeRequest, Spread
from oracle.oracle import OracleGenericStack
from tests.test_place_destructive import NIL_AT, Scenario, _job_with_own_allocs
from tests.test_place_destructive_full import (CAPACITY, KINDS, LENGTHS, MAXINT32, SCENARIOS, _aff, _refusal_scenario,
                                               _refusals, _windowed, reference)
from tests.test_plan_stops import _key

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nomad_pe.h")
LIB = os.path.join(ROOT, "nomad_amd", "libnomadpe.so")

ENTRY = "pe_place_destructive_full_metrics: "
TRACE_CAP = 1 << 24    # traced positions of one call (pe_place_csi_metrics' constant)
TOP_WAVE = 1024        # positions per record above which trace_records asks k_trace_top for its lists
TOP_OTHER = 128        # entries of one such list


def _many_nonoptions():
    """1500 nodes, 420 of them with an own alloc that distinct_hosts filters until its stop, half of those full
    besides: every record has more traced positions than TOP_WAVE and more entries that are not options than one
    k_trace_top list holds."""
    nodes, allocs, job, own_idx = _job_with_own_allocs(1500, 420, seed=521, tight=0.5)
    job.task_groups[0].constraints = [Constraint("", "", "distinct_hosts")]
    _aff(job)
    return Scenario(nodes, allocs, job, synth.shuffle(1500, 522), own_idx[:24])


ALL = dict(SCENARIOS)
ALL["many-nonoptions"] = _many_nonoptions


def _stack(sc: Scenario, cls, metrics=True, **kw):
    """Scenario.stack with AllocMetric on before the first Select (the preparation's included)."""
    st = cls(batch=sc.batch, **kw)
    st.SetState(sc.nodes, sc.allocs)
    st.SetJob(sc.job)
    st.SetNodes(sc.perm)
    if metrics:
        st.EnableMetrics(True)
    if sc.prep:
        sc.prep(st)
    return st


def _oracle(sc):
    return _stack(sc, OracleGenericStack)


def _engine(sc, metrics=True, **kw):
    from nomad_amd.stack import GenericStack
    return _stack(sc, GenericStack, metrics, **kw)


def _keys(records):
    return [_key(r) for r in records]


def _count_loop(st, k, tg=0):
    """The count loop with metrics: (record keys, maps)."""
    keys, maps = [], []
    for _ in range(k):
        r = st.SelectRaw(tg)
        keys.append(_key(r))
        maps.append(st.LastMetrics())
        if r.row < 0:
            break
        st.Commit(tg, r.row)
    return keys, maps


@functools.lru_cache(maxsize=None)
def _scenario(name):
    return reference(name)[0] if name in SCENARIOS else ALL[name]()


@functools.lru_cache(maxsize=None)
def reference_maps(name):
    """The scenario, and the oracle's records and maps of the interleaved loop
    with metrics on. Computed once and shared; nothing changes it afterwards."""
    sc = _scenario(name)
    recs, maps = place_destructive_metrics_by_select(_oracle(sc), 0, sc.upd)
    return sc, _keys(recs), maps


def _differing(a, b):
    n = max(len(a), len(b))
    return sum(1 for k in range(n) if k >= len(a) or k >= len(b) or a[k] != b[k])


# ---- CPU, no device ---------------------------------------------------------------

def test_header_library_and_binding_declare_the_entry():
    from nomad_amd.stack import GenericStack
    assert "pe_place_destructive_full_metrics" in abi.ENGINE_SYMBOLS
    assert callable(getattr(GenericStack, "PlaceDestructiveFullMetrics", None))
    with open(HEADER) as fh:
        text = fh.read()
    assert "int pe_place_destructive_full_metrics(pe_stack* s, uint32_t tg_index, const uint32_t* allocs, uint32_t n,\n" \
           "                                      pe_ranked_node* out, uint32_t* placed);" in text
    assert hasattr(C.CDLL(LIB), "pe_place_destructive_full_metrics")


@pytest.mark.parametrize("name", sorted(ALL))
def test_scenario_maps_depend_on_the_interleaving(name):
    sc, keys, maps = reference_maps(name)
    assert len(maps) == len(keys)
    if name in SCENARIOS:
        assert keys == reference(name)[1]                 # metrics change no record
    _, none = _count_loop(_oracle(sc), len(sc.upd))
    st = _oracle(sc)
    st.StopAllocs(sc.upd)
    _, front = _count_loop(st, len(sc.upd))
    d_none, d_front = _differing(maps, none), _differing(maps, front)
    print(name, "records whose maps differ from no stops / all stops up front:", d_none, "/", d_front, "of", len(maps))
    assert d_none >= 1, "the loop with no stops gives the same maps"
    assert d_front >= 1, "all stops up front give the same maps"


def test_scenarios_reach_the_map_kinds():
    parts, nonzero, dims, cons, most_scores = set(), set(), set(), set(), 0
    for name in sorted(SCENARIOS):
        _, keys, maps = reference_maps(name)
        for m in maps:
            dims |= set(m["DimensionExhausted"])
            cons |= set(m["ConstraintFiltered"])
            most_scores = max(most_scores, len(m["ScoreMetaData"]))
            for _, _, scores in m["ScoreMetaData"]:
                parts |= set(scores)
                nonzero |= {k for k, v in scores.items() if v != 0.0}
    assert {"allocation-spread", "node-affinity", "devices"} <= parts
    assert {"allocation-spread", "node-affinity"} <= nonzero
    assert {"cpu", "memory", "devices: no devices match request"} <= dims
    assert {"distinct_hosts", "missing devices", "computed class ineligible"} <= cons
    assert most_scores == 5
    # a final nil record, with maps of its own
    _, keys, maps = reference_maps("nil")
    assert len(maps) == NIL_AT + 1 and keys[-1][0] == -1 and maps[-1]["DimensionExhausted"]
    assert maps[-1]["ScoreMetaData"] == []


def _traced_and_others(key, m):
    """Of one record: the positions that pass the feasibility wrapper (what the trace sees), and those of them
    that are not options (distinct_hosts filters behind the wrapper; exhausted nodes)."""
    dh = m["ConstraintFiltered"].get("distinct_hosts", 0)
    return key[3] - (key[4] - dh), dh + key[5]


def test_many_nonoptions_overflows_the_list_of_entries_that_are_not_options():
    sc, keys, maps = reference_maps("many-nonoptions")
    assert len(keys) == len(sc.upd) == 24 and all(k[0] >= 0 for k in keys)
    for k, m in zip(keys, maps):
        traced, others = _traced_and_others(k, m)
        assert traced > TOP_WAVE and others > TOP_OTHER, (traced, others)
        assert m["ConstraintFiltered"].get("distinct_hosts", 0) > 0 and m["DimensionExhausted"].get("cpu", 0) > 0
    # above-block takes the list path as well, without overflow
    sc, keys, maps = reference_maps("above-block")
    for k, m in zip(keys, maps):
        traced, others = _traced_and_others(k, m)
        assert traced > TOP_WAVE and others <= TOP_OTHER, (traced, others)


# ---- GPU --------------------------------------------------------------------------

def _assert_parity(name):
    sc, keys, maps = reference_maps(name)
    eng = _engine(sc)
    recs, got = eng.PlaceDestructiveFullMetrics(0, sc.upd, fallback=False)
    assert _keys(recs) == keys
    assert len(got) == len(maps)
    for k, (g, w) in enumerate(zip(got, maps)):
        assert g == w, "record %d of %s" % (k, name)
    return sc, eng, recs


@gpu
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("n", LENGTHS)
def test_parity_over_list_lengths(n, kind):
    _assert_parity("len%d-%s" % (n, kind))


@gpu
@pytest.mark.parametrize("name", ["above-block", "below-block", "nonpositive", "distinct-hosts", "two-levels", "mixed",
                                  "latched", "devices", "other-group", "off-list", "many-nonoptions"])
def test_parity_of_records_and_maps(name):
    sc, eng, _ = _assert_parity(name)
    ora = _oracle(sc)
    place_destructive_metrics_by_select(ora, 0, sc.upd)
    assert eng.GetCursor() == ora.GetCursor() and eng.GetCursor()[1] == MAXINT32
    assert eng.Eligibility() == ora.Eligibility()


@gpu
def test_nil_record_has_maps_and_its_stop_is_back():
    sc, eng, recs = _assert_parity("nil")
    assert len(recs) == NIL_AT + 1 and recs[-1].row == -1
    ora = _oracle(sc)
    place_destructive_metrics_by_select(ora, 0, sc.upd)
    assert eng.GetCursor() == ora.GetCursor() and eng.Eligibility() == ora.Eligibility()
    row = eng.row(sc.allocs[sc.upd[NIL_AT]].node_id)
    for st in (eng, ora):
        st.SetNodes([row])
    r = eng.SelectRaw(0)
    assert _key(r) == _key(ora.SelectRaw(0)) and r.row < 0 and r.nodes_exhausted == 1
    assert eng.LastMetrics() == ora.LastMetrics()


@gpu
@pytest.mark.parametrize("name", ["len65-target", "len2-even", "len150-aff", "mixed", "nil", "devices", "latched"])
def test_equal_to_the_plain_call_on_a_handle_without_metrics(name):
    sc, keys, _ = reference_maps(name)
    on, off = _engine(sc), _engine(sc, metrics=False)
    recs, _ = on.PlaceDestructiveFullMetrics(0, sc.upd, fallback=False)
    plain = off.PlaceDestructiveFull(0, sc.upd, fallback=False)
    assert _keys(recs) == _keys(plain) == keys
    assert [list(r.scores) for r in recs] == [list(r.scores) for r in plain]
    assert on.GetCursor() == off.GetCursor() and on.GetCursor()[1] == MAXINT32
    assert on.Eligibility() == off.Eligibility()


@gpu
def test_later_state_equals_the_per_call_sequence():
    sc, keys, maps = reference_maps("len150-target")
    assert len(sc.upd) == 48
    a, b, ora = _engine(sc), _engine(sc), _oracle(sc)
    # the list split at 20 into two calls is the sequence too, with maps per call
    r1, m1 = a.PlaceDestructiveFullMetrics(0, sc.upd[:20], fallback=False)
    assert a.PlaceDestructiveMaps() == m1
    r2, m2 = a.PlaceDestructiveFullMetrics(0, sc.upd[20:], fallback=False)
    assert len(m1) == 20 and len(m2) == 28
    assert _keys(r1 + r2) == keys and m1 + m2 == maps
    rb, mb = place_destructive_metrics_by_select(b, 0, sc.upd)
    assert _keys(rb) == keys and mb == maps
    place_destructive_metrics_by_select(ora, 0, sc.upd)
    assert a.GetCursor() == b.GetCursor() == ora.GetCursor()
    assert a.Eligibility() == b.Eligibility() == ora.Eligibility()
    # a PopUpdate and a Select with its maps on a stopped node
    last = sc.upd[-1]
    row = a.row(sc.allocs[last].node_id)
    got = []
    for st in (a, b, ora):
        st.PopUpdate(last)
        st.SetNodes([row])
        one = _key(st.SelectRaw(0))
        one_maps = st.LastMetrics()
        st.SetNodes(sc.perm)
        got.append(([one], [one_maps]))
    assert got[0] == got[1] == got[2]
    # a Place of 20 (the property sets and build_job_counts from the mirrors)
    pa, pb = _keys(a.Place(0, 20)), _keys(b.Place(0, 20))
    po, _ = _count_loop(ora, 20)
    assert pa == pb == po
    assert a.GetCursor() == b.GetCursor() and a.Eligibility() == b.Eligibility()


@gpu
@pytest.mark.parametrize("name", ["latched", "other-group"])
def test_sibling_groups_next_select_equals_the_sequences(name):
    sc, keys, maps = reference_maps(name)
    a, b, ora = _engine(sc), _engine(sc), _oracle(sc)
    recs, got = a.PlaceDestructiveFullMetrics(0, sc.upd, fallback=False)
    assert _keys(recs) == keys and got == maps
    for st in (b, ora):
        place_destructive_metrics_by_select(st, 0, sc.upd)
    want = _count_loop(ora, 2, tg=1)
    assert _count_loop(a, 2, tg=1) == want and _count_loop(b, 2, tg=1) == want
    want = _count_loop(ora, 3)
    assert _count_loop(a, 3) == want and _count_loop(b, 3) == want
    assert a.GetCursor() == b.GetCursor() == ora.GetCursor() and a.Eligibility() == b.Eligibility()


@gpu
def test_windowed_group_forwards_to_the_windowed_entries():
    from nomad_amd.stack import EngineError
    sc = _windowed()
    ora = _oracle(sc)
    want, want_maps = place_destructive_metrics_by_select(ora, 0, sc.upd)
    # metrics on: pe_place_destructive_metrics
    a, b = _engine(sc), _engine(sc)
    recs, maps = a.PlaceDestructiveFullMetrics(0, sc.upd, fallback=False)
    rb, mb = b.PlaceDestructiveMetrics(0, sc.upd, fallback=False)
    assert _keys(recs) == _keys(rb) == _keys(want) and maps == mb == want_maps
    assert len({k[3] for k in _keys(recs)}) > 1 and a.GetCursor()[1] < MAXINT32       # windowed Selects
    assert a.GetCursor() == b.GetCursor() and a.Eligibility() == b.Eligibility()
    assert a.place_destructive_stats() == b.place_destructive_stats()
    # metrics off: pe_place_destructive_full (which forwards to pe_place_destructive), no maps
    c, d = _engine(sc, metrics=False), _engine(sc, metrics=False)
    recs, none = c.PlaceDestructiveFullMetrics(0, sc.upd, fallback=False)
    assert none is None and _keys(recs) == _keys(d.PlaceDestructiveFull(0, sc.upd, fallback=False)) == _keys(want)
    assert c.place_destructive_stats() == d.place_destructive_stats() and c.place_destructive_stats()[1] == 1
    with pytest.raises(EngineError) as err:
        c.PlaceDestructiveMaps()
    assert err.value.code == abi.PE_ESTATE


@gpu
def test_metrics_off_is_the_plain_full_pass_call():
    from nomad_amd.stack import EngineError
    sc, keys, _ = reference_maps("len150-even")
    x, y = _engine(sc, metrics=False), _engine(sc, metrics=False)
    recs, none = x.PlaceDestructiveFullMetrics(0, sc.upd, fallback=False)
    assert none is None and _keys(recs) == keys == _keys(y.PlaceDestructiveFull(0, sc.upd, fallback=False))
    assert x.place_destructive_stats() == y.place_destructive_stats()           # no further launch
    assert x.place_destructive_stats()[1] == 1
    with pytest.raises(EngineError) as err:
        x.PlaceDestructiveMaps()
    assert err.value.code == abi.PE_ESTATE


@gpu
@pytest.mark.parametrize("name", ["len150-even", "len150-aff", "above-block", "many-nonoptions"])
def test_counters_do_not_depend_on_n(name):
    sc, _, _ = reference_maps(name)
    x, y = _engine(sc), _engine(sc)
    n = len(sc.upd)
    x.PlaceDestructiveFullMetrics(0, sc.upd[:4], fallback=False)
    x.PlaceDestructiveFullMetrics(0, sc.upd[4:n // 2], fallback=False)     # 20 of 48 (8 of 24)
    y.PlaceDestructiveFullMetrics(0, sc.upd[:4], fallback=False)
    y.PlaceDestructiveFullMetrics(0, sc.upd[4:n - 4], fallback=False)      # 40 of 48 (16 of 24)
    few, many = x.place_destructive_stats(), y.place_destructive_stats()
    print(name, "launches, synchronisations, uploads:", few, many)
    assert few == many
    # uploads: the staged list, the argument copy, the trace's rows and events
    assert few[2] == 3
    # synchronisations: the loop's and the trace's; one more when a list of entries that are not options overflowed
    assert few[1] == (3 if name == "many-nonoptions" else 2)


@gpu
def test_counters_for_20_and_44_updates():
    sc, _, _ = reference_maps("len150-target")
    x, y = _engine(sc), _engine(sc)
    x.PlaceDestructiveFullMetrics(0, sc.upd[:4], fallback=False)
    x.PlaceDestructiveFullMetrics(0, sc.upd[4:24], fallback=False)          # 20 updates
    y.PlaceDestructiveFullMetrics(0, sc.upd[:4], fallback=False)
    y.PlaceDestructiveFullMetrics(0, sc.upd[4:48], fallback=False)          # 44 updates
    t20, t44 = x.place_destructive_stats(), y.place_destructive_stats()
    print("launches, synchronisations, uploads:", t20, t44)
    assert t20 == t44 and t20[1] == 2 and t20[2] == 3


@gpu
@pytest.mark.parametrize("case", sorted(k for k in _refusals() if k != "metrics on"))
def test_refusals_leave_the_handle_as_it_was(case):
    from nomad_amd.stack import Unsupported
    match, kw, sc = _refusal_scenario(case)
    eng, fresh = _engine(sc, **kw), _engine(sc, **kw)
    cursor, elig = eng.GetCursor(), eng.Eligibility()
    with pytest.raises(Unsupported, match=match) as err:
        eng.PlaceDestructiveFullMetrics(0, sc.upd, fallback=False)
    if case != "the group's own reason":
        assert ENTRY in str(err.value)
    assert eng.GetCursor() == cursor and eng.Eligibility() == elig
    try:
        want, want_maps = place_destructive_metrics_by_select(fresh, 0, sc.upd)
    except Unsupported:
        # the engine's own Select refuses this job too: the refused handle's answer as well
        with pytest.raises(Unsupported):
            place_destructive_metrics_by_select(eng, 0, sc.upd)
        return
    # cursor, plan, NodeUpdate and the metrics shadow untouched: the fallback answers as a fresh handle does
    recs, maps = eng.PlaceDestructiveFullMetrics(0, sc.upd)
    assert _keys(recs) == _keys(want) and maps == want_maps
    assert eng.GetCursor() == fresh.GetCursor() and eng.Eligibility() == fresh.Eligibility()


@gpu
def test_existing_entries_keep_their_metrics_rows_and_a_csi_group_is_refused():
    from nomad_amd.stack import Unsupported
    from tests.test_csi import csi_job, engine_with, kat
    sc, _, _ = reference_maps("len2-target")
    eng = _engine(sc)
    with pytest.raises(Unsupported, match="pe_place_destructive_full: pe_set_metrics on"):
        eng.PlaceDestructiveFull(0, sc.upd, fallback=False)
    with pytest.raises(Unsupported, match="pe_place_destructive_metrics: a group that runs full passes"):
        eng.PlaceDestructiveMetrics(0, sc.upd, fallback=False)
    nodes, volumes, node_volumes = kat()
    allocs = [Allocation(node_id=nodes[0].id, job_id="csi-job", task_group="web", cpu_shares=100, memory_mb=64)]
    job = csi_job([CSIVolumeRequest("volume-id")], count=2)
    job.task_groups[0].spreads = [Spread("${node.class}", 50, [])]
    eng = engine_with(nodes, volumes, node_volumes, job, allocs=allocs)
    eng.EnableMetrics(True)
    cursor = eng.GetCursor()
    with pytest.raises(Unsupported, match=ENTRY + "a group with CSI requests"):
        eng.PlaceDestructiveFullMetrics(0, [0], fallback=False)
    assert eng.GetCursor() == cursor


@gpu
def test_refusal_beyond_the_trace_of_one_call():
    # 2047 x 8200 positions lie just above 2^24: decided on the host, nothing is launched
    from nomad_amd.stack import GenericStack, Unsupported
    n, listed = 8200, 2047
    assert listed * n > TRACE_CAP >= (listed - 1) * n
    nodes, allocs = synth.cluster_c2(n, seed=61)
    assert len(allocs) >= listed
    job = synth.job_c2(10)
    _aff(job)
    eng = GenericStack()
    eng.SetState(nodes, allocs)
    eng.SetJob(job)
    eng.SetNodes(synth.shuffle(n, 7))
    eng.EnableMetrics(True)
    cursor, elig, stats = eng.GetCursor(), eng.Eligibility(), eng.place_destructive_stats()
    lst = np.arange(listed, dtype=np.uint32)
    out, placed = (abi.pe_ranked_node * 1)(), C.c_uint32(0)    # refused before anything is written
    with pytest.raises(Unsupported, match=ENTRY + "n times the node list's length exceeds the trace"):
        eng._check(eng._lib.pe_place_destructive_full_metrics(eng._h, 0, lst.ctypes.data_as(abi.u32p), len(lst), out,
                                                              C.byref(placed)))
    assert eng.GetCursor() == cursor and eng.Eligibility() == elig and placed.value == 0
    assert eng.place_destructive_stats() == stats == (0, 0, 0)


@gpu
def test_refusal_beyond_the_entries_of_one_workgroup():
    # §48's shape with metrics on: the kernel finds the overflow while it builds its entries, before the first
    # stop; the host walk has not run then, so the metrics shadow of the memo is untouched as well
    from nomad_amd.stack import GenericStack, Unsupported
    n = CAPACITY + 8
    nodes, _ = synth.cluster_c2(n, seed=71, other_allocs=False)
    allocs = [Allocation(node_id=nodes[k].id, job_id="svc-c2", task_group="web", cpu_shares=500, memory_mb=256,
                         disk_mb=150, priority=50) for k in (5, 900, 8100)]
    job = synth.job_c2(3)
    job.version = 7
    _aff(job)
    sc = Scenario(nodes, allocs, job, synth.shuffle(n, 72), [0, 1, 2])
    eng, fresh = _engine(sc), _engine(sc)
    cursor, elig = eng.GetCursor(), eng.Eligibility()
    with pytest.raises(Unsupported, match=ENTRY + "more options .* LDS holds \\(%d" % CAPACITY):
        eng.PlaceDestructiveFullMetrics(0, sc.upd, fallback=False)
    assert eng.GetCursor() == cursor and eng.Eligibility() == elig
    want, want_maps = place_destructive_metrics_by_select(fresh, 0, sc.upd)
    recs, maps = eng.PlaceDestructiveFullMetrics(0, sc.upd)                 # no stop had been applied
    assert _keys(recs) == _keys(want) and maps == want_maps
    assert eng.GetCursor() == fresh.GetCursor() and eng.Eligibility() == fresh.Eligibility()


@gpu
def test_maps_lifetime_and_last_metrics():
    from nomad_amd.stack import EngineError
    sc, keys, maps = reference_maps("len65-target")
    eng = _engine(sc)
    with pytest.raises(EngineError) as err:                    # no call yet
        eng.PlaceDestructiveMaps()
    assert err.value.code == abi.PE_ESTATE
    recs, got = eng.PlaceDestructiveFullMetrics(0, sc.upd[:30], fallback=False)
    assert got == maps[:30] and eng.PlaceDestructiveMaps() == got      # read twice
    with pytest.raises(EngineError) as err:                    # as after pe_place_destructive_metrics
        eng.LastMetrics()
    assert err.value.code == abi.PE_ESTATE
    assert eng.PlaceDestructiveFullMetrics(0, [], fallback=False) == ([], [])   # n == 0: PE_OK, nothing changed
    assert eng.PlaceDestructiveMaps() == got
    r = eng.SelectRaw(0)                                       # the handle's next mutating call
    assert r.row >= 0 and eng.LastMetrics()["ScoreMetaData"]
    with pytest.raises(EngineError) as err:
        eng.PlaceDestructiveMaps()
    assert err.value.code == abi.PE_ESTATE


@gpu
def test_invalid_arguments_change_nothing():
    from nomad_amd.stack import EngineError
    sc, keys, maps = reference_maps("len150-target")
    eng = _engine(sc)
    cursor, elig = eng.GetCursor(), eng.Eligibility()
    for tg, lst in ((1, sc.upd[:4]), (0, sc.upd[:3] + [len(sc.allocs)]), (0, sc.upd[:3] + [sc.upd[1]])):
        with pytest.raises(EngineError) as err:
            eng.PlaceDestructiveFullMetrics(tg, lst, fallback=False)
        assert err.value.code == abi.PE_EINVAL
        assert eng.GetCursor() == cursor and eng.Eligibility() == elig
    lst = np.asarray(sc.upd[:2], dtype=np.uint32)
    placed = C.c_uint32(0)
    assert eng._lib.pe_place_destructive_full_metrics(eng._h, 0, lst.ctypes.data_as(abi.u32p), 2, None,
                                                      C.byref(placed)) == abi.PE_EINVAL
    assert eng._lib.pe_place_destructive_full_metrics(None, 0, lst.ctypes.data_as(abi.u32p), 2, None,
                                                      C.byref(placed)) == abi.PE_EINVAL
    recs, got = eng.PlaceDestructiveFullMetrics(0, sc.upd, fallback=False)     # nothing had changed
    assert _keys(recs) == keys and got == maps


@gpu
@pytest.mark.parametrize("name", ["len150-target", "nil"])
def test_shim_sends_a_run_with_metrics_through_the_entry(name):
    from nomad_amd.shim import DeviceStack, Plan
    sc, keys, _ = reference_maps(name)
    eng, ora = _engine(sc), _oracle(sc)
    calls = []
    entry = eng.PlaceDestructiveFullMetrics

    def counted(tg, allocs, fallback=True):
        calls.append((tg, len(allocs), fallback))
        return entry(tg, allocs, fallback=fallback)

    eng.PlaceDestructiveFullMetrics = counted
    shim = DeviceStack(eng, Plan())
    shim.SetJob(sc.job)
    shim.SetNodes(sc.perm)
    eng.EnableMetrics(True)
    if sc.prep:
        sc.prep(eng)
    placed = shim.PlaceDestructive(0, sc.upd)
    assert calls == [(0, len(sc.upd), False)]
    want = [k for k in keys if k[0] >= 0]
    assert _keys(placed) == want
    assert eng.place_destructive_stats()[1] >= 2                           # the loop's and the trace's
    place_destructive_metrics_by_select(ora, 0, sc.upd)
    assert sorted(a for lst in shim.plan.node_update.values() for a in lst) == sorted(sc.upd[:len(want)])
    assert sorted(a.node_row for lst in shim.plan.node_allocation.values() for a in lst) == sorted(k[0] for k in want)
    nxt = shim.Select(0)
    assert _key(nxt) == _key(ora.Select(0))
    assert eng.GetCursor() == ora.GetCursor() and eng.Eligibility() == ora.Eligibility()


@gpu
def test_shim_answers_a_refused_run_with_metrics_update_by_update():
    from nomad_amd.shim import DeviceStack, Plan
    match, kw, sc = _refusal_scenario("distinct_property in the group")
    eng, fresh = _engine(sc), _engine(sc)
    shim = DeviceStack(eng, Plan())
    shim.SetJob(sc.job)
    shim.SetNodes(sc.perm)
    eng.EnableMetrics(True)
    recs, _ = place_destructive_metrics_by_select(fresh, 0, sc.upd)
    want = [k for k in _keys(recs) if k[0] >= 0]
    assert _keys(shim.PlaceDestructive(0, sc.upd)) == want and len(want) >= 1
    assert eng.GetCursor() == fresh.GetCursor()
