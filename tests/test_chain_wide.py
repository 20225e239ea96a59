"""The chain's wide phases ("wide phases"), engine vs oracle.

k_phase resolves one rotation's Selects across many workgroups before k_chain
when the window holds no non-positive option; k_chain starts from what the
wide launches left (ChainSeed) and resolves the rest, or everything when a
phase was declined. Every case compares the full records with the oracle's
and with the engine's own with PE_CHAIN_WIDE=0, and asserts the counters of
phases resolved / declined, so a fallback cannot hide a failure. The lists
are the smallest that reach each edge: bitmap word edges (33, 64, 65), one
and several lanes' worth of Selects, a cursor in mid-list (the prefix wraps),
rows that win in both phases (base1, the shared writeback slot) and rows whose
second value is "exhausted" (the option bitmap changes between the phases).
"""
import numpy as np
import pytest

from nomad_amd import synth
from nomad_amd.structs import Allocation, Constraint
from oracle.oracle import OracleGenericStack
from tests.helpers import assert_same_placements, run_place
from tests.test_chain_load_batches import roomy_cluster, small_job
from tests.test_chain_windows import big_job, one_slot_cluster

pytestmark = pytest.mark.gpu


def _engine(**kw):
    from nomad_amd.stack import GenericStack
    return GenericStack(**kw)


@pytest.fixture
def unfused(monkeypatch):
    monkeypatch.delenv("PE_CHAIN_ITEMS", raising=False)
    monkeypatch.delenv("PE_CHAIN_WIDE", raising=False)
    monkeypatch.setenv("PE_CHAIN_FUSED", "0")


def _limit(n):
    return int(np.ceil(np.log2(n)))


def _three(monkeypatch, nodes, allocs, job, perm, counts):
    """Place `counts` (one call each, on one stack) on the oracle, the engine
    and the engine without the wide phases; the records of all three equal.
    Returns the records and the wide engine's (resolved, declined)."""
    out = []
    for cls, wide in ((OracleGenericStack, None), (_engine, True), (_engine, False)):
        if wide is False:
            monkeypatch.setenv("PE_CHAIN_WIDE", "0")
        st, limit, res = run_place(cls, nodes, allocs, job, perm, count=counts[0])
        for c in counts[1:]:
            res = res + st.Place(0, c)
        out.append((limit, res, st.ChainWideStats() if wide is not None else None))
        if wide is False:
            monkeypatch.delenv("PE_CHAIN_WIDE")
    (lo, ro, _), (le, re, stats), (l0, r0, stats0) = out
    print("wide phases (resolved, declined):", stats)
    assert lo == le == l0
    assert stats0 == (0, 0)
    assert_same_placements(re, ro)
    assert_same_placements(re, r0)
    return re, stats, lo


# 1. two phases resolve 2 n / limit Selects, k_chain the rest of the count
@pytest.mark.parametrize("n", [33, 64, 65, 1000, 1025, 4097])
def test_two_phases(unfused, monkeypatch, n):
    nodes, allocs = synth.cluster_c2(n, seed=42)
    count = n // _limit(n) + 60
    re, stats, limit = _three(monkeypatch, nodes, allocs, synth.job_c2(count), synth.shuffle(n, 21), [count])
    assert limit == _limit(n) and count * limit > n
    assert stats == (2, 0)
    assert sum(1 for x in re if x.row >= 0) == count


# 2. nine rotations: the wide phases take two, k_chain goes on from their records
def test_hand_off_to_k_chain(unfused, monkeypatch):
    nodes = roomy_cluster(300, seed=5)
    re, stats, limit = _three(monkeypatch, nodes, [], small_job(300), synth.shuffle(300, 23), [300])
    assert limit == 9
    assert stats == (2, 0)
    wins = np.bincount([x.row for x in re if x.row >= 0])
    assert (wins >= 3).sum() >= 10, "the list must make rows win three and more times"


# 3. the count ends inside the first rotation: one wide launch, k_chain exits at once
def test_one_phase_only(unfused, monkeypatch):
    nodes, allocs = synth.cluster_c2(1000, seed=42)
    re, stats, limit = _three(monkeypatch, nodes, allocs, synth.job_c2(40), synth.shuffle(1000, 22), [40])
    assert 40 * limit < 1000
    assert stats == (1, 0)
    assert sum(1 for x in re if x.row >= 0) == 40


# 4. holes in the option bitmap: filtered classes; rows exhausted after one placement
def test_filtered_classes(unfused, monkeypatch):
    nodes, allocs = synth.cluster_c2(1000, seed=11)
    count = 200
    job = synth.job_c2(count)
    job.constraints = list(job.constraints) + [Constraint("${node.class}", "class-[3-7]", "regexp")]
    re, stats, limit = _three(monkeypatch, nodes, allocs, job, synth.shuffle(1000, 24), [count])
    kept = sum(nd.node_class in ("class-3", "class-4", "class-5", "class-6", "class-7") for nd in nodes)
    assert 0.5 * len(nodes) < kept < 0.75 * len(nodes)   # about a third of the classes filtered
    assert count * limit > kept
    assert stats == (2, 0)
    assert any(x.nodes_filtered for x in re)


def test_one_slot_rows_change_the_bitmap(unfused, monkeypatch):
    nodes = roomy_cluster(200, seed=6) + one_slot_cluster(100, seed=32)
    re, stats, limit = _three(monkeypatch, nodes, [], big_job(80), synth.shuffle(300, 25), [80])
    assert limit == 9
    assert stats == (2, 0)
    one_slot = {i for i in range(200, 300)}
    assert any(x.row in one_slot for x in re), "one-slot rows must win (their base1 is exhausted)"
    assert any(x.nodes_exhausted for x in re)


# 5. declined phases: k_chain resolves them as before
def test_declined_non_positive_options(unfused, monkeypatch):
    nodes, allocs = synth.cluster_c2(300, seed=13)
    job = synth.job_c2(2)   # desired count 2: each collision costs -(c + 1) / 2
    allocs = allocs + [Allocation(node_id=nd.id, job_id=job.id, task_group="web")
                       for nd in nodes[::5] for _ in range(3)]
    re, stats, _ = _three(monkeypatch, nodes, allocs, job, synth.shuffle(300, 26), [30])
    assert stats[1] >= 1 and stats[0] == 0
    assert sum(1 for x in re if x.row >= 0) == 30


def test_declined_fewer_options_than_limit(unfused, monkeypatch):
    nodes = one_slot_cluster(40, seed=33)
    allocs = [Allocation(node_id=nd.id, job_id="other", task_group="tg", cpu_shares=3000, memory_mb=256,
                         disk_mb=300, priority=50) for nd in nodes[4:]]
    re, stats, limit = _three(monkeypatch, nodes, allocs, big_job(3), synth.shuffle(40, 27), [3])
    assert limit == 6
    assert stats[1] >= 1 and stats[0] == 0
    assert sum(1 for x in re if x.row >= 0) == 3


# 6. the second call starts in mid-list: the rank prefix wraps around the list's end
def test_non_zero_cursor(unfused, monkeypatch):
    nodes, allocs = synth.cluster_c2(1000, seed=42)
    rest = 1000 // 10 + 60
    re, stats, limit = _three(monkeypatch, nodes, allocs, synth.job_c2(30 + rest), synth.shuffle(1000, 28),
                              [30, rest])
    assert limit == 10 and 0 < re[-1].new_offset < 1000
    assert stats == (3, 0)


# 7. the caller protocol: the C loop with the view on, and a deviation through the view
def test_dropin_loop_with_the_view(unfused, monkeypatch):
    from tools import dropin
    from nomad_amd.stack import GenericStack
    nodes, allocs = synth.cluster_c2(1000, seed=42)
    job = synth.job_c2(600)
    order = np.asarray(synth.shuffle(1000, 29), dtype=np.uint32)[None, :]
    rows = {}
    for mode in ("wide", "off", "oracle"):
        if mode == "off":
            monkeypatch.setenv("PE_CHAIN_WIDE", "0")
        st = OracleGenericStack() if mode == "oracle" else GenericStack()
        monkeypatch.delenv("PE_CHAIN_WIDE", raising=False)
        st.SetState(nodes, allocs)
        dropin.use_view(True)
        placed, evals, selects, secs, last = dropin.prepare(st, job)(order, 600)
        rows[mode] = (placed, evals, list(last))
        if mode == "wide":
            assert st.ChainWideStats() == (2, 0)
        elif mode == "off":
            assert st.ChainWideStats() == (0, 0)
        st.close()
    assert rows["wide"] == rows["oracle"]
    assert rows["wide"] == rows["off"]


def test_deviation_after_the_wide_phases(unfused, monkeypatch):
    from tests.test_dropin import assert_equal_runs, compute_placements
    from tests.test_spec_view import ViewCaller, _pair, view_placements
    nodes, allocs = synth.cluster_c2(1000, seed=42)
    perm = synth.shuffle(1000, 30)
    dev = lambda i, o: (int(perm[77]) if i == 500 else None)
    eng, ora = _pair(nodes, allocs, synth.job_c2(600), perm)
    monkeypatch.setenv("PE_CHAIN_WIDE", "0")
    eng0, _ = _pair(nodes, allocs, synth.job_c2(600), perm)
    monkeypatch.delenv("PE_CHAIN_WIDE")
    a = view_placements(ViewCaller(eng), 600, deviate=dev)
    a0 = view_placements(ViewCaller(eng0), 600, deviate=dev)
    b = compute_placements(ora, 600, deviate=dev)
    assert_equal_runs(a, b)
    assert_equal_runs(a, a0)
    resolved, declined = eng.ChainWideStats()
    assert resolved >= 2 and declined == 0
    assert eng0.ChainWideStats() == (0, 0)
    assert eng.SpeculationStats()[2] >= 1   # the deviation rolled the run back


# 8. AllocMetric on: every Select's answer and maps equal the oracle's, with the
#    wide phases (the counters prove they ran) and with the switch off
def test_alloc_metric_on(unfused, monkeypatch):
    from tests.test_metrics import _metrics_pair, _view_metrics_protocol
    nodes, allocs = synth.cluster_c2(1000, seed=42)
    count = 1000 // 10 + 60
    for wide in (True, False):
        if not wide:
            monkeypatch.setenv("PE_CHAIN_WIDE", "0")
        eng, ora = _metrics_pair(nodes, allocs, synth.job_c2(count), synth.shuffle(1000, 21))
        monkeypatch.delenv("PE_CHAIN_WIDE", raising=False)
        _view_metrics_protocol(eng, ora, count)
        resolved, declined = eng.ChainWideStats()
        print("wide phases (resolved, declined):", (resolved, declined))
        if wide:
            assert resolved >= 2 and declined == 0
        else:
            assert (resolved, declined) == (0, 0)
