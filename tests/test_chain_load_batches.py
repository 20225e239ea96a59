"""The chain's batched loads ("load batches"), engine vs oracle.

k_chain reads the window's values in groups of BATCH positions per lane, with
clamped always-valid indices, and reads the re-evaluated values back in the
same groups; k_base<FOLD> has its first position in flight under the class
table copy and stores node_feas from its main loop when the visit list is a
permutation of the table (FoldArgs::list_covers), else in a pass of its own.
The lists here are the smallest that reach each new edge: positions per lane
of 1, BATCH, BATCH + 1 and 2 BATCH + 1, a last item with one live lane
(n = 1 mod 1024), a second phase with a shortened window, rows that win three
and more times, both verdicts of the fold on a permutation and on a subset.
The three exits of build_emit_rec (nil Select, device offers, plain) run
fused and unfused: the fused chain's later phases read their values through
the same batched loop before its tail builds the records.
"""
import numpy as np
import pytest

from nomad_amd import synth
from nomad_amd.structs import Constraint, Job, NetworkResource, Task, TaskGroup
from oracle.oracle import OracleGenericStack
from tests.helpers import assert_same_placements, run_place
from tests.test_chain_windows import big_job, one_slot_cluster

pytestmark = pytest.mark.gpu

BATCH = 4          # kChainLoadBatch (nomad_amd/csrc/kernels.hip)
LANES = 1024       # kChainBlock


def _engine(**kw):
    from nomad_amd.stack import GenericStack
    return GenericStack(**kw)


@pytest.fixture
def unfused16(monkeypatch):
    monkeypatch.setenv("PE_CHAIN_ITEMS", "16")
    monkeypatch.setenv("PE_CHAIN_FUSED", "0")


@pytest.fixture
def unfused(monkeypatch):
    monkeypatch.delenv("PE_CHAIN_ITEMS", raising=False)
    monkeypatch.setenv("PE_CHAIN_FUSED", "0")


def _c2(n):
    return synth.cluster_c2(n, seed=42)


def _count_for(n):
    # two phases at least: count x limit > n (limit = ceil(log2 n))
    limit = int(np.ceil(np.log2(n)))
    return n // limit + 60


# positions per lane 1, BATCH, BATCH + 1, 2 BATCH + 1: once with the last item
# full of live lanes' worth of positions, once with a single live lane
EDGE_LENGTHS = sorted({1000,
                       (BATCH - 1) * LANES + 1, BATCH * LANES,
                       BATCH * LANES + 1, BATCH * LANES + 600,
                       2 * BATCH * LANES + 1, 2 * BATCH * LANES + 700})


@pytest.mark.parametrize("n", EDGE_LENGTHS)
def test_batch_edges_shape16(unfused16, n):
    assert -(-n // LANES) in (1, BATCH, BATCH + 1, 2 * BATCH + 1)
    nodes, allocs = _c2(n)
    count = _count_for(n)
    job = synth.job_c2(count)
    perm = synth.shuffle(n, 21)
    _, lo, ro = run_place(OracleGenericStack, nodes, allocs, job, perm)
    _, le, re = run_place(_engine, nodes, allocs, job, perm)
    assert lo == le and count * lo > n
    assert_same_placements(re, ro)
    assert sum(1 for x in re if x.row >= 0) == count


@pytest.mark.parametrize("n,count,fused", [(900, 150, True), (900, 150, False), (2900, 256, True), (2900, 330, False)])
def test_natural_shapes(monkeypatch, n, count, fused):
    # shapes 1 and 4 as the engine picks them, as one fused launch and unfused
    monkeypatch.delenv("PE_CHAIN_ITEMS", raising=False)
    if fused:
        monkeypatch.delenv("PE_CHAIN_FUSED", raising=False)
    else:
        monkeypatch.setenv("PE_CHAIN_FUSED", "0")
    nodes, allocs = _c2(n)
    job = synth.job_c2(count)
    perm = synth.shuffle(n, 22)
    _, lo, ro = run_place(OracleGenericStack, nodes, allocs, job, perm)
    _, le, re = run_place(_engine, nodes, allocs, job, perm)
    assert lo == le and count * lo > n
    assert_same_placements(re, ro)


def roomy_cluster(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    nodes = []
    for k, nid in enumerate(sorted(synth.uuids(n, seed))):
        nd = synth.mock_node(nid)
        nd.name = "node-%05d" % k
        nd.cpu_shares = int(rng.integers(20000, 40000))   # dozens of 500 MHz asks fit
        nd.memory_mb = int(rng.choice([32768, 65536]))
        nd.compute_class()
        nodes.append(nd)
    return nodes


def small_job(count, constraints=()):
    return Job(id="pile", constraints=list(constraints), task_groups=[TaskGroup(
        name="web", count=count, ephemeral_disk_mb=150,
        network=NetworkResource(mode="host", dynamic_ports=1, host_network="default"),
        tasks=[Task(name="web", driver="exec", cpu=500, memory_mb=256)])])


@pytest.mark.parametrize("items", ["4", "16"])
def test_redo_read_back(monkeypatch, items):
    # binpack piles the placements on few rows: rows holding two and more
    # placements of the launch are re-evaluated phase after phase and read back
    monkeypatch.setenv("PE_CHAIN_ITEMS", items)
    monkeypatch.setenv("PE_CHAIN_FUSED", "0")
    nodes = roomy_cluster(1100, seed=5)
    job = small_job(400)
    perm = synth.shuffle(1100, 23)
    _, _, ro = run_place(OracleGenericStack, nodes, [], job, perm)
    _, _, re = run_place(_engine, nodes, [], job, perm)
    assert_same_placements(re, ro)
    wins = np.bincount([x.row for x in ro if x.row >= 0])
    assert (wins >= 3).sum() >= 10, "the list must make rows win three and more times"


def two_arch_cluster(n, seed):
    # cluster_c2's odd node classes are arm64: the job's constraint fails them
    return synth.cluster_c2(n, seed=seed)


def _arch_job(count):
    job = synth.job_c2(count)
    job.constraints = list(job.constraints) + [Constraint("${attr.cpu.arch}", "amd64", "=")]
    return job


def _feasible(nd):
    return nd.attributes["cpu.arch"] == "amd64"


def test_fold_on_a_permutation(unfused):
    from tests.test_dropin import assert_equal_runs, both
    nodes, allocs = two_arch_cluster(300, seed=7)
    a, b, _ = both(nodes, allocs, _arch_job(60), list(synth.shuffle(300, 24)), count=60)
    assert_equal_runs(a, b)
    assert 60 < sum(_feasible(nd) for nd in nodes) < 240   # both verdicts occur
    assert any(x is not None for x in a)
    assert all(x is None or _feasible(nodes[x[0]]) for x in a)


def test_fold_on_a_subset(unfused):
    from tests.test_dropin import assert_equal_runs, both
    nodes, allocs = two_arch_cluster(300, seed=7)
    perm = list(synth.shuffle(300, 25))[:263]
    a, b, _ = both(nodes, allocs, _arch_job(60), perm, count=60)
    assert_equal_runs(a, b)
    assert all(x is None or _feasible(nodes[x[0]]) for x in a)


def test_fold_subset_then_whole_table(unfused):
    # the fold rides in the first launch, whose list is a subset; the launches
    # after SetNodes(all) read node_feas of rows that list did not contain
    from tests.test_dropin import assert_equal_runs, compute_placements
    nodes, allocs = two_arch_cluster(300, seed=8)
    order = list(synth.shuffle(300, 26))
    job = _arch_job(80)
    res = []
    for st in (_engine(), OracleGenericStack()):
        st.SetState(nodes, allocs)
        st.SetJob(job)
        st.SetNodes(order[:100])
        out = compute_placements(st, 12)
        st.SetNodes(order)
        out += compute_placements(st, 60)
        res.append(out)
    assert_equal_runs(res[0], res[1])
    late = {x[0] for x in res[0][12:] if x is not None}
    assert late - set(order[:100]), "later Selects must reach rows outside the first list"
    assert all(_feasible(nodes[r]) for r in late)


@pytest.mark.parametrize("fused", [True, False])
def test_emit_nil_select(monkeypatch, fused):
    # the count exceeds the cluster: the last Select returns no node (row < 0)
    monkeypatch.delenv("PE_CHAIN_ITEMS", raising=False)
    if fused:
        monkeypatch.delenv("PE_CHAIN_FUSED", raising=False)
    else:
        monkeypatch.setenv("PE_CHAIN_FUSED", "0")
    nodes = one_slot_cluster(150, seed=31)
    job = big_job(170)
    perm = synth.shuffle(150, 27)
    _, _, ro = run_place(OracleGenericStack, nodes, [], job, perm)
    _, _, re = run_place(_engine, nodes, [], job, perm)
    assert_same_placements(re, ro)
    assert re[-1].row < 0 and sum(1 for x in re if x.row >= 0) == 150


@pytest.mark.parametrize("fused", [True, False])
def test_emit_device_offers(monkeypatch, fused):
    monkeypatch.delenv("PE_CHAIN_ITEMS", raising=False)
    if fused:
        monkeypatch.delenv("PE_CHAIN_FUSED", raising=False)
    else:
        monkeypatch.setenv("PE_CHAIN_FUSED", "0")
    nodes, allocs = synth.cluster_c5(500, seed=1)
    job = synth.job_c5(120)
    perm = synth.shuffle(len(nodes), 28)
    _, _, ro = run_place(OracleGenericStack, nodes, allocs, job, perm)
    _, _, re = run_place(_engine, nodes, allocs, job, perm)
    assert_same_placements(re, ro)
    assert [x.device_offers for x in re] == [x.device_offers for x in ro]
    assert any(x.device_offers for x in re)


@pytest.mark.parametrize("fused", [True, False])
def test_emit_plain(monkeypatch, fused):
    monkeypatch.delenv("PE_CHAIN_ITEMS", raising=False)
    if fused:
        monkeypatch.delenv("PE_CHAIN_FUSED", raising=False)
    else:
        monkeypatch.setenv("PE_CHAIN_FUSED", "0")
    from tests.test_dropin import assert_equal_runs, both
    nodes, allocs = _c2(700)
    a, b, _ = both(nodes, allocs, synth.job_c2(90), list(synth.shuffle(700, 29)), count=90)
    assert_equal_runs(a, b)
