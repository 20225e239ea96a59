"""Both wide phases in one launch (k_phases), engine vs oracle.

k_phases resolves the two rotations k_phase(0) and k_phase(1) resolve, in one
workgroup, from options compacted by rank in LDS. Every case compares the full
records of four legs: the oracle, the engine with the one-launch kernel, the
engine with PE_CHAIN_WIDE_ONE=0 (two k_phase launches) and the engine with
PE_CHAIN_WIDE=0 (k_chain alone). Every case asserts the counters of phases
resolved / declined and of wide launches by kind, so a fallback cannot hide a
failure. The lists are the smallest that reach each edge.
"""
import numpy as np
import pytest

from nomad_amd import synth
from nomad_amd.structs import Allocation
from oracle.oracle import OracleGenericStack
from tests.helpers import assert_same_placements, run_place
from tests.test_chain_load_batches import roomy_cluster, small_job
from tests.test_chain_windows import big_job, one_slot_cluster

ONE_LANES = 1024   # kOneBlock: the lanes of k_phases' workgroup


def _engine(**kw):
    from nomad_amd.stack import GenericStack
    return GenericStack(**kw)


@pytest.fixture
def unfused(monkeypatch):
    for name in ("PE_CHAIN_ITEMS", "PE_CHAIN_WIDE", "PE_CHAIN_WIDE_ONE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("PE_CHAIN_FUSED", "0")


def _limit(n):
    return int(np.ceil(np.log2(n)))


LEGS = (("oracle", None), ("one", {}), ("two", {"PE_CHAIN_WIDE_ONE": "0"}), ("off", {"PE_CHAIN_WIDE": "0"}))


def _four(monkeypatch, nodes, allocs, job, perm, counts, kind="one"):
    """Place `counts` (one call each, on one stack) on the oracle, the engine
    with one k_phases launch, with two k_phase launches and without the wide
    phases; the records of all four equal. `kind` is the launch kind the
    default leg must have taken ("two": the list is past the LDS cap). Returns
    the records, the default leg's (resolved, declined) and the limit."""
    out = {}
    for leg, env in LEGS:
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        st, limit, res = run_place(OracleGenericStack if env is None else _engine, nodes, allocs, job, perm,
                                   count=counts[0])
        for k in (env or {}):
            monkeypatch.delenv(k)
        first_offset = res[-1].new_offset
        for c in counts[1:]:
            res = res + st.Place(0, c)
        stats = launches = None
        if env is not None:
            stats, launches = st.ChainWideStats(), st.ChainWideLaunches()
            st.close()
        out[leg] = (limit, res, stats, launches, first_offset)
    print("wide phases (resolved, declined):", out["one"][2], out["two"][2], "launches (two, one):",
          out["one"][3], out["two"][3])
    assert out["oracle"][0] == out["one"][0] == out["two"][0] == out["off"][0]
    for leg in ("one", "two", "off"):
        assert_same_placements(out[leg][1], out["oracle"][1])
    assert out["off"][2] == (0, 0) and out["off"][3] == (0, 0)
    assert out["two"][2] == out["one"][2]
    n_launch = sum(out["two"][3])
    assert n_launch >= 1 and out["two"][3] == (n_launch, 0)
    assert out["one"][3] == ((0, n_launch) if kind == "one" else (n_launch, 0))
    return out["one"][1], out["one"][2], out["oracle"][0], out["oracle"][4]


# 1. bitmap word and lane edges, both phases inside the one launch
@pytest.mark.gpu
@pytest.mark.parametrize("n", [33, 64, 65, 1025])
def test_two_phases_in_one_launch(unfused, monkeypatch, n):
    nodes, allocs = synth.cluster_c2(n, seed=42)
    count = n // _limit(n) + 60
    re, stats, limit, _ = _four(monkeypatch, nodes, allocs, synth.job_c2(count), synth.shuffle(n, 21), [count])
    assert limit == _limit(n) and count * limit > n
    assert stats == (2, 0)
    assert sum(1 for x in re if x.row >= 0) == count


def _lanes_n():
    n = 2
    while n // _limit(n) <= ONE_LANES:
        n += 1
    return n


# 2. more Selects in a rotation than the workgroup has lanes (the list also sits near the LDS cap)
@pytest.mark.gpu
def test_more_selects_than_lanes(unfused, monkeypatch):
    n = _lanes_n()
    limit = _limit(n)
    assert n // limit == ONE_LANES + 1 and (n - 1) // _limit(n - 1) <= ONE_LANES
    nodes = roomy_cluster(n, seed=7)
    count = n // limit + 60
    takes, need, cap = _engine().ChainWideOneLds(n, count, limit)
    assert takes and need <= cap
    re, stats, lim, _ = _four(monkeypatch, nodes, [], big_job(count), synth.shuffle(n, 31), [count])
    assert lim == limit
    assert stats == (2, 0)
    # every position is an option, so the first rotation holds n // limit Selects
    assert all(x.nodes_filtered == 0 and x.nodes_exhausted == 0 for x in re[:n // limit])
    assert re[n // limit - 1].new_offset == (n // limit) * limit % n and n // limit > ONE_LANES
    assert sum(1 for x in re if x.row >= 0) == count


def _cap_n(st):
    """The largest list one k_phases launch takes at count = n // limit + 60
    (both rotations), by the launcher's own gate."""
    fits = lambda n: st.ChainWideOneLds(n, n // _limit(n) + 60, _limit(n))[0]
    lo, hi = 8193, 16384   # limit 14 throughout; the need grows with n
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid
    return lo


# 3. the LDS cap: the largest list the gate admits runs k_phases, the next one the two k_phase launches
@pytest.mark.gpu
@pytest.mark.parametrize("past", [0, 1])
def test_lds_cap(unfused, monkeypatch, past):
    st = _engine()
    n = _cap_n(st) + past
    limit = _limit(n)
    count = n // limit + 60
    takes, need, cap = st.ChainWideOneLds(n, count, limit)
    st.close()
    print("n", n, "count", count, "need", need, "cap", cap)
    assert takes == (past == 0) and (need <= cap) == (past == 0)
    nodes = roomy_cluster(n, seed=8)
    re, stats, lim, _ = _four(monkeypatch, nodes, [], big_job(count), synth.shuffle(n, 32), [count],
                              kind="two" if past else "one")
    assert lim == limit and count * limit > n
    assert stats == (2, 0)
    assert sum(1 for x in re if x.row >= 0) == count


# 4. the cursor in mid-word across both phases: the relative rank wraps in phase 0 and in phase 1
@pytest.mark.gpu
def test_cursor_in_mid_word(unfused, monkeypatch):
    nodes, allocs = synth.cluster_c2(1000, seed=42)
    rest = 1000 // 10 + 60
    re, stats, limit, first_offset = _four(monkeypatch, nodes, allocs, synth.job_c2(30 + rest),
                                           synth.shuffle(1000, 28), [30, rest])
    assert limit == 10 and rest * limit > 1000
    assert 0 < first_offset < 1000 and first_offset % 32 != 0
    assert stats == (3, 0)


# 5. rows that win in both phases (the shared writeback slot, base1 values) and
#    rows exhausted after one placement (the option bitmap changes between the phases)
#    (binpack makes most one-slot rows win, so few roomy rows win twice on the mixed
#    list; the roomy list with the small job has many rows that do)
@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [True, False])
def test_winners_of_both_phases_and_one_slot_rows(unfused, monkeypatch, mixed):
    if mixed:
        nodes = roomy_cluster(260, seed=6) + one_slot_cluster(40, seed=32)
        job, count, shuffle, again_min = big_job(80), 80, 25, 1
    else:
        nodes = roomy_cluster(300, seed=6)
        job, count, shuffle, again_min = small_job(300), 100, 23, 5
    re, stats, limit, _ = _four(monkeypatch, nodes, [], job, synth.shuffle(300, shuffle), [count])
    assert limit == 9 and count * limit > 300
    assert stats == (2, 0)
    if mixed:
        assert any(x.row >= 260 for x in re), "one-slot rows must win (their base1 is exhausted)"
        assert any(x.nodes_exhausted for x in re)
    # the rotations' first Selects: where the cursor wraps
    rot = [0] + [i for i in range(1, len(re)) if re[i].new_offset < re[i - 1].new_offset]
    assert len(rot) >= 3
    won0 = {x.row for x in re[:rot[1]]}
    again = sum(1 for x in re[rot[1]:rot[2]] if x.row in won0)
    assert again >= again_min, "phase 0 winners must win again in phase 1 (the shared writeback slot)"


# 6. phase 0 resolved, phase 1 declined inside the launch: exactly `limit` rows are
#    free, phase 0 resolves one Select, phase 1 has limit - 1 options (ns == 0)
@pytest.mark.gpu
def test_phase_one_declined_inside_the_launch(unfused, monkeypatch):
    nodes = one_slot_cluster(40, seed=33)
    limit = _limit(40)
    allocs = [Allocation(node_id=nd.id, job_id="other", task_group="tg", cpu_shares=3000, memory_mb=256,
                         disk_mb=300, priority=50) for nd in nodes[limit:]]
    count = 40 // limit + 1
    re, stats, lim, _ = _four(monkeypatch, nodes, allocs, big_job(count), synth.shuffle(40, 27), [count])
    assert lim == limit == 6 and count * limit > 40
    assert stats == (1, 1)
    assert sum(1 for x in re if x.row >= 0) == limit and re[-1].row < 0


# 7. phase 0 declined: non-positive options; nothing stored but the seed, k_chain resolves all
@pytest.mark.gpu
def test_phase_zero_declined(unfused, monkeypatch):
    nodes, allocs = synth.cluster_c2(300, seed=13)
    job = synth.job_c2(2)   # desired count 2: each collision costs -(c + 1) / 2
    allocs = allocs + [Allocation(node_id=nd.id, job_id=job.id, task_group="web")
                       for nd in nodes[::5] for _ in range(3)]
    re, stats, _, _ = _four(monkeypatch, nodes, allocs, job, synth.shuffle(300, 26), [30])
    assert stats[1] >= 1 and stats[0] == 0
    assert sum(1 for x in re if x.row >= 0) == 30


# 8. the caller protocol: the C loop with the view on
@pytest.mark.gpu
def test_dropin_loop_with_the_view(unfused, monkeypatch):
    from tools import dropin
    from nomad_amd.stack import GenericStack
    nodes, allocs = synth.cluster_c2(1000, seed=42)
    job = synth.job_c2(600)
    order = np.asarray(synth.shuffle(1000, 29), dtype=np.uint32)[None, :]
    rows = {}
    for leg, env in LEGS:
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        st = OracleGenericStack() if env is None else GenericStack()
        for k in (env or {}):
            monkeypatch.delenv(k)
        st.SetState(nodes, allocs)
        dropin.use_view(True)
        placed, evals, selects, secs, last = dropin.prepare(st, job)(order, 600)
        rows[leg] = (placed, evals, list(last))
        if leg == "one":
            assert st.ChainWideStats() == (2, 0)
            assert st.ChainWideLaunches() == (0, 1)
        elif leg == "two":
            assert st.ChainWideStats() == (2, 0)
            assert st.ChainWideLaunches() == (1, 0)
        elif leg == "off":
            assert st.ChainWideStats() == (0, 0)
            assert st.ChainWideLaunches() == (0, 0)
        st.close()
    assert rows["one"] == rows["oracle"]
    assert rows["one"] == rows["two"]
    assert rows["one"] == rows["off"]


# host-only logic against a plain restatement (no GPU)
def test_lds_bytes_and_gate_restated():
    """The launcher's LDS-size function: 8 bytes of value and 2 of position
    (rounded up to 16 in all) for each of min(n_visit, count * limit) entries;
    the gate admits a launch exactly when that is within the cap it reports
    (no device: cap 0, nothing admitted)."""
    import ctypes as C
    from nomad_amd.stack import load_engine
    lib = load_engine()
    buf = (C.c_uint64 * 2)()
    for n, count, limit in ((33, 65, 6), (1000, 40, 10), (1000, 160, 10), (10000, 1000, 14), (14350, 1085, 14),
                            (16384, 1, 14), (16384, 1231, 14), (16384, 262143, 18)):
        rc = lib.pe_chain_wide_one_lds(n, count, limit, buf)
        entries = min(n, count * limit)
        assert int(buf[0]) == 8 * entries + (2 * entries + 15) // 16 * 16
        assert rc == (1 if int(buf[0]) <= int(buf[1]) else 0)
    # bad arguments are never admitted
    for n, count, limit in ((0, 10, 6), (16385, 10, 15), (100, 0, 7), (100, 10, 0), (100, 10, 19)):
        assert lib.pe_chain_wide_one_lds(n, count, limit, buf) == 0


def test_rank_to_select_arithmetic():
    """An option's entry is its rank relative to the cursor, entry k belongs to
    Select k // L: restated with a sort over the set positions."""
    rng = np.random.Generator(np.random.PCG64(3))
    for n, L, cur in ((33, 6, 0), (64, 6, 31), (65, 7, 64), (1000, 10, 333), (1025, 11, 1024)):
        bits = rng.random(n) < 0.7
        pos = np.flatnonzero(bits)
        tot = len(pos)
        words = np.zeros((n + 31) // 32, dtype=np.uint32)
        for p in pos:
            words[p >> 5] |= np.uint32(1) << np.uint32(p & 31)
        prefix = np.concatenate([[0], np.cumsum([bin(int(w)).count("1") for w in words])])
        rank = lambda p: int(prefix[p >> 5]) + bin(int(words[p >> 5]) & ((1 << (p & 31)) - 1)).count("1")
        c_opt = rank(cur) if cur < n else tot
        ns = tot // L
        entry = {}
        for p in pos:
            r = rank(int(p))
            k = r - c_opt if r >= c_opt else r + tot - c_opt
            if k < ns * L:
                entry[k] = int(p)
        plain = sorted(int(p) for p in pos if p >= cur) + sorted(int(p) for p in pos if p < cur)
        assert [entry[k] for k in range(ns * L)] == plain[:ns * L]
        for s in range(ns):
            assert [entry[k] for k in range(s * L, (s + 1) * L)] == plain[s * L:(s + 1) * L]
