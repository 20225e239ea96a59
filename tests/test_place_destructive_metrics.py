"""pe_place_destructive_metrics / pe_place_destructive_maps: computePlacements'
destructive-update loop (generic_sched.go:543-645) in one call with AllocMetric
kept: per update the maps GenericScheduler stores on the new alloc, or in
failedTGAllocs for the nil Select that ends the loop.

Yardsticks: the oracle with EnableMetrics(True) driven through
place_destructive_metrics_by_select (records and maps), and for later state a
second engine handle that ran that per-call sequence with metrics on. Records
are compared with test_plan_stops' `_key`, maps with `==` on the dicts: equal,
not close. The scenarios are test_place_destructive's; a CPU test first shows,
on the oracle alone, that each of them tests the stops' effect on the maps."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from nomad_amd import abi, synth
from nomad_amd.stack import place_destructive_metrics_by_select
from nomad_amd.structs import Allocation, CSIVolumeRequest
from oracle.oracle import OracleGenericStack
from tests.test_place_destructive import NIL_AT, Scenario, _refusal_scenario, _refusals, reference
from tests.test_plan_stops import _key

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nomad_pe.h")
LIB = os.path.join(ROOT, "nomad_amd", "libnomadpe.so")

PARITY_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129)
COVERAGE = ("cut300", "cut100", "mixed", "nil", "devices", "len65-svc", "len2-svc")


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


def _count_loop(st, k):
    """The count loop with metrics: (record keys, maps)."""
    keys, maps = [], []
    for _ in range(k):
        r = st.SelectRaw(0)
        keys.append(_key(r))
        maps.append(st.LastMetrics())
        if r.row < 0:
            break
        st.Commit(0, r.row)
    return keys, maps


def _keys(records):
    return [_key(r) for r in records]


@functools.lru_cache(maxsize=None)
def reference_maps(name):
    """The scenario, and the oracle's records and maps of the interleaved loop
    with metrics on. Computed once and shared; nothing changes it afterwards."""
    sc = reference(name)[0]
    recs, maps = place_destructive_metrics_by_select(_oracle(sc), 0, sc.upd)
    return sc, _keys(recs), maps


def _differing(a, b):
    n = max(len(a), len(b))
    return sum(1 for k in range(n) if k >= len(a) or k >= len(b) or a[k] != b[k])


# ---- CPU, no device ---------------------------------------------------------------

def test_header_library_and_binding_declare_both_entries():
    from nomad_amd.stack import GenericStack
    assert "pe_place_destructive_metrics" in abi.ENGINE_SYMBOLS and "pe_place_destructive_maps" in abi.ENGINE_SYMBOLS
    assert callable(getattr(GenericStack, "PlaceDestructiveMetrics", None))
    assert callable(getattr(GenericStack, "PlaceDestructiveMaps", None))
    with open(HEADER) as fh:
        text = fh.read()
    assert "int pe_place_destructive_metrics(pe_stack* s, uint32_t tg_index, const uint32_t* allocs, uint32_t n,\n" \
           "                                 pe_ranked_node* out, uint32_t* placed);" in text
    assert "int pe_place_destructive_maps(const pe_stack* s, const pe_metric_count** counts, " \
           "const uint32_t** counts_off,\n                              const pe_metric_score** scores, " \
           "const uint32_t** scores_off, uint32_t* n_rec);" in text
    lib = C.CDLL(LIB)
    assert hasattr(lib, "pe_place_destructive_metrics") and hasattr(lib, "pe_place_destructive_maps")


@pytest.mark.parametrize("name", COVERAGE)
def test_scenario_maps_depend_on_the_interleaving(name):
    sc, keys, maps = reference_maps(name)
    # metrics change no record
    assert keys == reference(name)[1]
    assert len(maps) == len(keys)
    _, none = _count_loop(_oracle(sc), len(sc.upd))
    st = _oracle(sc)
    st.StopAllocs(sc.upd)
    _, front = _count_loop(st, len(sc.upd))
    d_none, d_front = _differing(maps, none), _differing(maps, front)
    print(name, "records whose maps differ from no stops / all stops up front:", d_none, "/", d_front, "of", len(maps))
    assert d_none >= 1, "the loop with no stops gives the same maps"
    assert d_front >= 1, "all stops up front give the same maps"


def test_scenarios_reach_the_map_kinds():
    dims, most_scores = set(), 0
    for name in COVERAGE:
        _, keys, maps = reference_maps(name)
        for m in maps:
            dims |= set(m["DimensionExhausted"])
            most_scores = max(most_scores, len(m["ScoreMetaData"]))
    assert {"cpu", "memory", "devices: no devices match request"} <= dims
    assert most_scores == 5
    # a final nil record, with maps of its own
    _, keys, maps = reference_maps("nil")
    assert len(maps) == NIL_AT + 1 and keys[-1][0] == -1 and maps[-1]["DimensionExhausted"]
    assert maps[-1]["ScoreMetaData"] == []


def test_a_stop_changes_a_non_zero_job_anti_affinity():
    # 'mixed' holds two own allocs per node: after the stop of one, the node's penalty counts the other
    # alone (rank.go:588-591: -(collisions + 1) / count). The collisions are restated here from the list.
    sc, keys, maps = reference_maps("mixed")
    st = _oracle(sc)
    tg = sc.job.task_groups[0]
    base, stopped = {}, {}
    for i, a in enumerate(sc.allocs):
        if a.job_id == sc.job.id and a.task_group == tg.name and not a.terminal:
            base[a.node_id] = base.get(a.node_id, 0) + 1
    pre = [sc.upd[9]]                                          # _mixed stops this one before the call
    for ai in pre:
        base[sc.allocs[ai].node_id] -= 1
    placed = {}
    found = 0
    for i, ai in enumerate(sc.upd):
        a = sc.allocs[ai]
        if not a.terminal and ai not in pre:
            stopped[a.node_id] = stopped.get(a.node_id, 0) + 1
        for node, _, scores in maps[i]["ScoreMetaData"]:
            c = base.get(node, 0) - stopped.get(node, 0) + placed.get(node, 0)
            assert scores.get("job-anti-affinity", 0.0) == (-(c + 1) / tg.count if c > 0 else 0.0)
            if c > 0 and stopped.get(node, 0) > 0:
                found += 1
        if keys[i][0] >= 0:
            node = sc.nodes[keys[i][0]].id
            assert st.row(node) == keys[i][0]
            placed[node] = placed.get(node, 0) + 1
    assert found >= 1, "no ScoreMetaData entry whose non-zero job-anti-affinity a stop changed"


def test_devices_scenario_traces_a_row_with_a_placement_and_a_later_stop():
    sc, keys, maps = reference_maps("devices")
    st = _oracle(sc)
    rows = [st.row(sc.allocs[a].node_id) for a in sc.upd]
    n = len(sc.perm)
    pos = {int(r): p for p, r in enumerate(sc.perm)}
    start = [st.GetCursor()[0]]
    for k in keys:
        start.append(k[6])                       # new_offset
    found = False
    for j in range(1, len(keys)):
        row = rows[j]
        if row not in {k[0] for k in keys[:j]}:
            continue
        for k in range(j, len(keys)):            # the row lies in the window of a record that saw the stop
            if (pos[row] - start[k]) % n < keys[k][3]:     # nodes_evaluated
                found = True
    assert found


# ---- GPU --------------------------------------------------------------------------

def _assert_parity(name):
    sc, keys, maps = reference_maps(name)
    eng = _engine(sc)
    recs, got = eng.PlaceDestructiveMetrics(0, sc.upd, fallback=False)
    assert _keys(recs) == keys
    assert len(got) == len(maps)
    for k, (g, w) in enumerate(zip(got, maps)):
        assert g == w, "record %d of %s" % (k, name)
    return sc, eng, recs


@gpu
@pytest.mark.parametrize("batch", [False, True], ids=["svc", "batch"])
@pytest.mark.parametrize("n", PARITY_LENGTHS)
def test_parity_over_list_lengths(n, batch):
    _assert_parity("len%d-%s" % (n, "batch" if batch else "svc"))


@gpu
@pytest.mark.parametrize("name", ["cut300", "cut100", "mixed", "devices", "large"])
def test_parity_of_records_and_maps(name):
    _assert_parity(name)


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
@pytest.mark.parametrize("name", ["len65-svc", "len2-batch", "mixed", "nil", "devices"])
def test_equal_to_the_plain_call(name):
    sc, keys, _ = reference_maps(name)
    on, off = _engine(sc), _engine(sc, metrics=False)
    recs, _ = on.PlaceDestructiveMetrics(0, sc.upd, fallback=False)
    plain = off.PlaceDestructive(0, sc.upd, fallback=False)
    assert _keys(recs) == _keys(plain) == keys
    assert [list(r.scores) for r in recs] == [list(r.scores) for r in plain]
    assert on.GetCursor() == off.GetCursor() and on.Eligibility() == off.Eligibility()


@gpu
def test_later_state_equals_the_per_call_sequence():
    sc, keys, maps = reference_maps("len300-svc")
    assert len(sc.upd) == 64
    a, b, ora = _engine(sc), _engine(sc), _oracle(sc)
    # two calls over one list are the sequence too
    r1, m1 = a.PlaceDestructiveMetrics(0, sc.upd[:20], fallback=False)
    r2, m2 = a.PlaceDestructiveMetrics(0, sc.upd[20:], fallback=False)
    assert _keys(r1 + r2) == keys and m1 + m2 == maps
    rb, mb = place_destructive_metrics_by_select(b, 0, sc.upd)
    assert _keys(rb) == keys and mb == maps
    place_destructive_metrics_by_select(ora, 0, sc.upd)
    assert a.GetCursor() == b.GetCursor() == ora.GetCursor()
    assert a.Eligibility() == b.Eligibility() == ora.Eligibility()
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
    # a Place of 20 forces build_job_counts from the mirrors
    pa, pb = _keys(a.Place(0, 20)), _keys(b.Place(0, 20))
    po, _ = _count_loop(ora, 20)
    assert pa == pb == po
    assert a.GetCursor() == b.GetCursor() and a.Eligibility() == b.Eligibility()


@gpu
def test_counters_do_not_depend_on_n():
    sc, _, _ = reference_maps("len300-svc")
    x, y = _engine(sc), _engine(sc)
    x.PlaceDestructiveMetrics(0, sc.upd[:20], fallback=False)
    x.PlaceDestructiveMetrics(0, sc.upd[20:], fallback=False)          # 44 updates
    y.PlaceDestructiveMetrics(0, sc.upd[:44], fallback=False)
    y.PlaceDestructiveMetrics(0, sc.upd[44:], fallback=False)          # 20 updates
    t44, t20 = x.place_destructive_stats(), y.place_destructive_stats()
    print("launches, synchronisations, uploads:", t44, t20)
    assert t44 == t20
    # the loop's and the trace's synchronisation; the stop list and the trace's rows
    assert t44[1] == 2 and t44[2] == 2


@gpu
@pytest.mark.parametrize("case", sorted(k for k in _refusals() if k != "metrics on"))
def test_refusals_leave_the_handle_as_it_was(case):
    from nomad_amd.stack import Unsupported
    match, kw, sc = _refusal_scenario(case)
    eng, fresh = _engine(sc, **kw), _engine(sc, **kw)
    cursor, elig = eng.GetCursor(), eng.Eligibility()
    with pytest.raises(Unsupported, match=match):
        eng.PlaceDestructiveMetrics(0, sc.upd, fallback=False)
    assert eng.GetCursor() == cursor and eng.Eligibility() == elig
    try:
        want, want_maps = place_destructive_metrics_by_select(fresh, 0, sc.upd)
    except Unsupported:
        # the engine's own Select refuses this job too: the refused handle's answer as well
        with pytest.raises(Unsupported):
            place_destructive_metrics_by_select(eng, 0, sc.upd)
        return
    # cursor, plan, NodeUpdate and the metrics shadow untouched: the fallback answers as a fresh handle does
    recs, maps = eng.PlaceDestructiveMetrics(0, sc.upd)
    assert _keys(recs) == _keys(want) and maps == want_maps
    assert eng.GetCursor() == fresh.GetCursor() and eng.Eligibility() == fresh.Eligibility()


@gpu
def test_plain_call_still_refuses_metrics_and_the_new_one_refuses_csi():
    from nomad_amd.stack import Unsupported
    from tests.test_csi import csi_job, engine_with, kat
    sc, _, _ = reference_maps("len2-svc")
    eng = _engine(sc)
    with pytest.raises(Unsupported, match="pe_set_metrics on"):
        eng.PlaceDestructive(0, sc.upd, fallback=False)
    nodes, volumes, node_volumes = kat()
    allocs = [Allocation(node_id=nodes[0].id, job_id="csi-job", task_group="web", cpu_shares=100, memory_mb=64)]
    eng = engine_with(nodes, volumes, node_volumes, csi_job([CSIVolumeRequest("volume-id")], count=2), allocs=allocs)
    eng.EnableMetrics(True)
    cursor = eng.GetCursor()
    with pytest.raises(Unsupported, match="pe_place_destructive_metrics: a group with CSI requests"):
        eng.PlaceDestructiveMetrics(0, [0], fallback=False)
    assert eng.GetCursor() == cursor


@gpu
def test_refusal_beyond_the_overlay_of_one_launch():
    from nomad_amd.stack import GenericStack, Unsupported
    nodes, allocs = synth.cluster_c2(3000, seed=61)
    assert len(allocs) > 2049
    eng = GenericStack()
    eng.SetState(nodes, allocs)
    eng.SetJob(synth.job_c2(10))
    eng.SetNodes(synth.shuffle(3000, 7))
    eng.EnableMetrics(True)
    cursor = eng.GetCursor()
    lst = np.arange(2049, dtype=np.uint32)
    out, placed = (abi.pe_ranked_node * 1)(), C.c_uint32(0)    # refused before anything is written
    with pytest.raises(Unsupported, match="overlay of one launch"):
        eng._check(eng._lib.pe_place_destructive_metrics(eng._h, 0, lst.ctypes.data_as(abi.u32p), len(lst), out,
                                                         C.byref(placed)))
    assert eng.GetCursor() == cursor and placed.value == 0


@gpu
def test_metrics_off_forwards_and_the_maps_answer_estate():
    from nomad_amd.stack import EngineError
    sc, keys, maps = reference_maps("len65-svc")
    eng = _engine(sc, metrics=False)
    recs, none = eng.PlaceDestructiveMetrics(0, sc.upd, fallback=False)
    assert _keys(recs) == keys and none is None
    assert eng.place_destructive_stats()[1] == 1               # the plain call's one synchronisation
    with pytest.raises(EngineError) as err:
        eng.PlaceDestructiveMaps()
    assert err.value.code == abi.PE_ESTATE


@gpu
def test_maps_lifetime_and_last_metrics():
    from nomad_amd.stack import EngineError
    sc, keys, maps = reference_maps("len65-svc")
    eng = _engine(sc)
    with pytest.raises(EngineError) as err:                    # no call yet
        eng.PlaceDestructiveMaps()
    assert err.value.code == abi.PE_ESTATE
    recs, got = eng.PlaceDestructiveMetrics(0, sc.upd[:30], fallback=False)
    assert got == maps[:30] and eng.PlaceDestructiveMaps() == got      # read twice
    with pytest.raises(EngineError) as err:                    # as after pe_place_csi_metrics
        eng.LastMetrics()
    assert err.value.code == abi.PE_ESTATE
    assert eng.PlaceDestructiveMetrics(0, [], fallback=False) == ([], [])   # n == 0: PE_OK, nothing changed
    assert eng.PlaceDestructiveMaps() == got
    r = eng.SelectRaw(0)                                       # the handle's next mutating call
    assert r.row >= 0 and eng.LastMetrics()["ScoreMetaData"]
    with pytest.raises(EngineError) as err:
        eng.PlaceDestructiveMaps()
    assert err.value.code == abi.PE_ESTATE


@gpu
def test_invalid_arguments_change_nothing():
    from nomad_amd.stack import EngineError
    sc, keys, maps = reference_maps("len65-svc")
    eng = _engine(sc)
    cursor, elig = eng.GetCursor(), eng.Eligibility()
    for tg, lst in ((1, sc.upd[:4]), (0, sc.upd[:3] + [len(sc.allocs)]), (0, sc.upd[:3] + [sc.upd[1]])):
        with pytest.raises(EngineError) as err:
            eng.PlaceDestructiveMetrics(tg, lst, fallback=False)
        assert err.value.code == abi.PE_EINVAL
        assert eng.GetCursor() == cursor and eng.Eligibility() == elig
    lst = np.asarray(sc.upd[:2], dtype=np.uint32)
    placed = C.c_uint32(0)
    assert eng._lib.pe_place_destructive_metrics(eng._h, 0, lst.ctypes.data_as(abi.u32p), 2, None,
                                                 C.byref(placed)) == abi.PE_EINVAL
    assert eng._lib.pe_place_destructive_metrics(None, 0, lst.ctypes.data_as(abi.u32p), 2, None,
                                                 C.byref(placed)) == abi.PE_EINVAL
    n = C.c_uint32(0)
    assert eng._lib.pe_place_destructive_maps(eng._h, None, None, None, None, C.byref(n)) == abi.PE_EINVAL
    recs, got = eng.PlaceDestructiveMetrics(0, sc.upd, fallback=False)     # nothing had changed
    assert _keys(recs) == keys and got == maps
