"""In-place updates of jobs with spread stanzas in one call
(pe_inplace_update_spread). SpreadIterator never filters
(spread.go:110-174): the walk decides the statuses without the spread sets and a
second stage adds the allocation-spread part in list order, from the property
counts each update's Select sees in the per-call sequence. Ground truth is that
sequence on the oracle (nomad_amd.stack.inplace_update_by_select, or
inplace_update_metrics_by_select with the maps on); the same helper on a second
engine handle is the second witness. Records are compared bit for bit, every
score included.

`spread_model` below restates the counts in closed form (the formula of §38).
The CPU tests pin the yardstick by hand and the model against the oracle; the
GPU tests use the model only to show that a shape exercises what it is there
for (a prefix that matters, the -1 boost, Craw0 > 1, ...)."""
import ctypes as C

import numpy as np
import pytest

from nomad_amd import abi, synth
from nomad_amd.stack import inplace_update_by_select, inplace_update_metrics_by_select
from nomad_amd.structs import Allocation, Constraint, NetworkResource, Spread, SpreadTarget, Task, TaskGroup
from oracle.oracle import OracleGenericStack, OracleSystemStack
from tests.test_inplace_update import _assert_same_after, _key, _keys, _loop, _multi_own, _setup
from tests.test_inplace_update_metrics import _mkeys, _same_metrics_oracle, _well_formed

gpu = pytest.mark.gpu

CHUNK = 128   # pe::kInplaceSpreadChunk (engine_types.h)
LDS_VALUES = 2048   # pe::kLdsPsetValues

TARGET = Spread("${node.class}", 60, [SpreadTarget("class-1", 40), SpreadTarget("class-2", 30)])
EVEN = Spread("${node.class}", 50, [])


# ---- the closed form ---------------------------------------------------------------

def _node_value(node, attribute):
    key = attribute.strip()
    assert key.startswith("${") and key.endswith("}"), attribute
    key = key[2:-1]
    if key == "node.class":
        return node.node_class
    if key == "node.unique.id":
        return node.id
    if key.startswith("attr."):
        return node.attributes.get(key[5:])
    if key.startswith("meta."):
        return node.meta.get(key[5:])
    raise AssertionError(attribute)


def _even_boost(mn, mx, present, cur):
    """evenSpreadScoreBoost (spread.go:178-228) from min / max / number of the used values."""
    if present == 0:
        return 0.0
    delta = -1.0 if mn == 0 else float(mn - cur) / float(mn)
    if cur != mn:
        return delta
    if mn == mx:
        return -1.0
    if mn == 0:
        return 1.0
    return float(mx - mn) / float(mn)


def spread_model(nodes, allocs, job, tg, upd, status, plan_nodes=(), stopped=()):
    """The allocation-spread part of every update of `upd` (None where status
    is not 0), from the state at the call's start (`plan_nodes`: node ids of the
    plan's allocs of the group; `stopped`: alloc indices in NodeUpdate) and the
    statuses alone. Returns (parts, columns): columns[k] = (EP0, Craw0, prop0)
    of set k, job-level sets first."""
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
        sets.append(dict(sp=sp, ep0=ep0, craw0=craw0, prop0=prop0, desired=desired, star=star,
                         frac=float(si.weight) / float(wsum), even=not si.targets, ks={}, kc={}))

    parts = []
    for ai, st in zip(upd, status):
        a = allocs[ai]
        own = mine(a)
        total = 0.0
        for s in sets:
            vi = _node_value(by_id[a.node_id], s["sp"].attribute)

            def count(u):
                ks = s["ks"].get(u, 0)
                ep = s["ep0"].get(u, 0) + ks
                craw = s["craw0"].get(u, 0) + s["kc"].get(u, 0) + (1 if (u == vi and own) else 0)
                cleared = craw - (1 if ((u in s["prop0"] or ks > 0) and craw > 1) else 0)
                return ep - cleared if ep >= cleared else 0

            if vi is None:
                b = -1.0
            elif s["even"]:
                used = [c for c in (count(u) for u in s["ep0"]) if c > 0]
                b = _even_boost(min(used) if used else 0, max(used) if used else 0, len(used), count(vi))
            else:
                d = s["desired"].get(vi, s["star"])
                b = -1.0 if d is None else ((d - float(count(vi) + 1)) / d) * s["frac"]
            total += b
            if st == 0 and vi is not None:
                s["ks"][vi] = s["ks"].get(vi, 0) + 1
                if own:
                    s["kc"][vi] = s["kc"].get(vi, 0) + 1
        parts.append(total if st == 0 else None)
    return parts, [(s["ep0"], s["craw0"], s["prop0"]) for s in sets]


def _with_part(base, part):
    """A record's key with the spread part appended as score_into appends it."""
    if base is None:
        return None
    scores = list(base[2])
    total = scores[0]
    for x in scores[1:]:
        total += x
    if part != 0.0:
        total += part
        scores.append(part)
    return (base[0], total / float(len(scores)), tuple(scores)) + tuple(base[3:])


# ---- CPU: the yardstick by hand ----------------------------------------------------

def _tiny():
    """Four mock nodes in two classes, three allocs of the group (two in class
    a), ten wanted, half per class: desired 5.0 per value, weight fraction 1."""
    nodes, _ = synth.cluster_c1(4, seed=5)
    for k, nd in enumerate(nodes):
        nd.node_class = "a" if k < 2 else "b"
        nd.compute_class()
    allocs = [Allocation(node_id=nodes[k].id, job_id="svc-c2", task_group="web", cpu_shares=500, memory_mb=256,
                         disk_mb=150) for k in (0, 1, 2)]
    job = synth.job_c2(10)
    job.version = 2
    job.task_groups[0].spreads = [Spread("${node.class}", 50, [SpreadTarget("a", 50), SpreadTarget("b", 50)])]
    return nodes, allocs, job


def test_hand_counts_first_and_second_update_on_a_value():
    nodes, allocs, job = _tiny()
    st = _setup(OracleGenericStack, nodes, allocs, job)
    records, status = inplace_update_by_select(st, 0, [0, 1, 2])
    assert status == [0, 0, 0]
    # alloc 0, value a: two existing, its own staged stop is the one cleared
    # value and nothing is proposed on a: the Select sees E - 1 = 1
    assert records[0].scores[-1] == ((5.0 - 2.0) / 5.0) * 1.0
    # alloc 1, value a: two existing + alloc 0's update = 3; alloc 0's stop and
    # the staged one are cleared, a is proposed and 2 > 1, so one comes back:
    # the Select sees 3 - 1 = 2 = E
    assert records[1].scores[-1] == ((5.0 - 3.0) / 5.0) * 1.0
    # alloc 2, value b: the first update there sees E - 1 = 0
    assert records[2].scores[-1] == ((5.0 - 1.0) / 5.0) * 1.0
    for r in records:
        assert len(r.scores) == 2                      # binpack, allocation-spread
        assert r.final_score == (r.scores[0] + r.scores[1]) / 2.0
    assert spread_model(nodes, allocs, job, 0, [0, 1, 2], status)[0] == [r.scores[-1] for r in records]


def test_hand_counts_earlier_stop_and_commit():
    nodes, allocs, job = _tiny()
    st = _setup(OracleGenericStack, nodes, allocs, job)
    st.StopAllocs([1])                                  # an own alloc on another node of class a
    st.SetNodes([st.row(nodes[1].id)])
    assert st.Select(0).row == st.row(nodes[1].id)
    st.Commit(0, st.row(nodes[1].id))                   # a is proposed
    records, status = inplace_update_by_select(st, 0, [0])
    assert status == [0]
    # two existing + the commit = 3; cleared: alloc 1's stop and the staged one,
    # a is proposed and 2 > 1: one comes back, the Select sees 2. Without that
    # branch it would see 1 and score 0.6
    assert records[0].scores[-1] == ((5.0 - 3.0) / 5.0) * 1.0
    parts, cols = spread_model(nodes, allocs, job, 0, [0], status, plan_nodes=[nodes[1].id], stopped=[1])
    assert parts == [records[0].scores[-1]]
    assert cols[0] == ({"a": 3, "b": 1}, {"a": 1}, {"a"})


# ---- CPU: the closed form against the oracle's per-call records ----------------------

def _prepared(n_stop, n_commit, seed=79, own=200, n=64):
    """_multi_own with `n_stop` of the job's allocs stopped earlier (and not
    listed) and `n_commit` earlier commits: (nodes, allocs, job, upd, stops)."""
    nodes, allocs, job, upd = _multi_own(n, own, seed=seed)
    stops, upd = upd[:n_stop], upd[n_stop:]
    return nodes, allocs, job, upd, stops, n_commit


def _prep_of(stops, n_commit, n, log=None, seed=17):
    """Earlier StopAllocs and commits; the committed rows go to `log`."""
    if not stops and not n_commit:
        return None

    def prep(st):
        if stops:
            st.StopAllocs(stops)
        st.SetNodes(synth.shuffle(n, seed))
        for _ in range(n_commit):
            opt = st.Select(0)
            assert opt is not None
            st.Commit(0, opt.row)
            if log is not None:
                log.append(opt.row)
    return prep


@pytest.mark.parametrize("form", ["target", "even"])
@pytest.mark.parametrize("n_stop,n_commit", [(0, 0), (5, 4), (6, 5)])
def test_closed_form_equals_the_oracle(form, n_stop, n_commit):
    nodes, allocs, job, upd, stops, _ = _prepared(n_stop, n_commit)
    job.task_groups[0].spreads = [TARGET if form == "target" else EVEN]
    rows = []
    prep = _prep_of(stops, n_commit, 64, rows)
    st = _setup(OracleGenericStack, nodes, allocs, job)
    if prep:
        prep(st)
    want = _keys(inplace_update_by_select(st, 0, upd))
    # the same updates without the spread, from the same plan: the statuses and the other parts
    job.task_groups[0].spreads = []
    base = _setup(OracleGenericStack, nodes, allocs, job)
    if stops:
        base.StopAllocs(stops)
    for row in rows:
        base.Commit(0, row)
    plain = _keys(inplace_update_by_select(base, 0, upd))
    assert plain[1] == want[1] and 0 in want[1] and 2 in want[1]
    job.task_groups[0].spreads = [TARGET if form == "target" else EVEN]
    parts, _ = spread_model(nodes, allocs, job, 0, upd, want[1], plan_nodes=[st.nodes[r].id for r in rows],
                            stopped=stops)
    got = [_with_part(b, p) for b, p in zip(plain[0], parts)]
    assert got == want[0]                              # == on every double
    assert sum(1 for k in want[0] if k is not None) >= 140


# ---- GPU: the call against the per-call sequence --------------------------------------

def _three(nodes, allocs, job, upd, prep=None, system=False, config=None, metrics=False):
    """The new call on one engine handle, the helper on the oracle and on a
    second engine handle: [(stack, answer)] x 3, answers as (record keys,
    statuses[, maps])."""
    from nomad_amd.stack import GenericStack, SystemStack
    eng_cls, ora_cls = (SystemStack, OracleSystemStack) if system else (GenericStack, OracleGenericStack)
    helper = inplace_update_metrics_by_select if metrics else inplace_update_by_select
    out = []
    for cls, batched in ((eng_cls, True), (ora_cls, False), (eng_cls, False)):
        st = _setup(cls, nodes, allocs, job, config=config)
        if metrics:
            st.EnableMetrics(True)
        if prep:
            prep(st)
        res = st.InplaceUpdateSpread(0, upd, fallback=False) if batched else helper(st, 0, upd)
        if batched:
            assert (res[2] is not None) == metrics
        out.append((st, (_mkeys(res) if metrics else _keys(res[:2])), res))
    return out


def _same(three):
    (eng, a, _), (ora, b, _), (eng2, c, _) = three
    assert a[1] == b[1] == c[1]                        # statuses
    assert a[0] == b[0] == c[0]                        # records, every score, bit for bit
    return (eng, ora, eng2), a


def _last_parts(keys):
    return [k[2][-1] if k is not None else None for k in keys]


def _shape_a(spreads, seed=79, own=200):
    nodes, allocs, job, upd = _multi_own(64, own, seed=seed)
    job.task_groups[0].spreads = spreads
    return nodes, allocs, job, upd


@gpu
def test_target_spread_several_allocs_per_node():                       # (a), (m)
    from nomad_amd.stack import GenericStack
    nodes, allocs, job, upd = _shape_a([TARGET])
    per_node = {}
    for i in upd:
        per_node[allocs[i].node_id] = per_node.get(allocs[i].node_id, 0) + 1
    assert max(per_node.values()) >= 5
    stacks, a = _same(_three(nodes, allocs, job, upd))
    assert 0 in a[1] and 2 in a[1]
    parts, _ = spread_model(nodes, allocs, job, 0, upd, a[1])
    assert [p for p in parts if p] == [x for x, p in zip(_last_parts(a[0]), parts) if p]
    assert len({p for p in parts if p is not None}) > 8   # more than one part per class: the prefix shows
    # PopUpdate of a finished update that is its node's last NodeUpdate entry, and of one that is not
    done = {}
    for i, st in zip(upd, a[1]):
        if st == 0:
            done.setdefault(allocs[i].node_id, []).append(i)
    last = next(v[-1] for v in done.values() if len(v) >= 2)
    not_last = next(v[0] for v in done.values() if len(v) >= 2 and v[-1] != last)
    for st in stacks:
        st.PopUpdate(not_last)
        st.PopUpdate(last)
    _assert_same_after(stacks, 64, 12)
    # a new evaluation on the handle starts from the snapshot again
    eng = stacks[0]
    eng.ResetPlan()
    eng.SetJob(job)
    eng.SetNodes(synth.shuffle(64, 13))
    fresh = _setup(GenericStack, nodes, allocs, job)
    fresh.SetNodes(synth.shuffle(64, 13))
    assert _key(eng.Select(0)) == _key(fresh.Select(0))


@gpu
def test_even_spread_the_prefix_matters():                              # (b)
    nodes, allocs, job, upd = _shape_a([EVEN])
    stacks, a = _same(_three(nodes, allocs, job, upd))
    assert 0 in a[1] and 2 in a[1]
    by_id = {n.id: n for n in nodes}
    seen = {}
    for i, k in zip(upd, a[0]):
        if k is not None and len(k[2]) >= 2:
            seen.setdefault(by_id[allocs[i].node_id].node_class, set()).add(k[2][-1])
    assert max(len(v) for v in seen.values()) >= 2     # two updates on one value, different parts
    parts, _ = spread_model(nodes, allocs, job, 0, upd, a[1])
    assert [p for p in parts if p] == [x for x, p in zip(_last_parts(a[0]), parts) if p]
    _assert_same_after(stacks, 64, 22)


def _shape_c():
    """A job-level target spread on a meta key and a group-level even spread on
    an attribute; a third of the nodes lack the one, a quarter the other."""
    nodes, allocs, job, upd = _multi_own(64, 160, seed=85)
    for k, nd in enumerate(nodes):
        if k % 3:
            nd.meta["rack"] = "r%d" % (k % 5)
        if k % 4:
            nd.attributes["zone"] = "z%d" % (k % 3)
        nd.compute_class()
    job.spreads = [Spread("${meta.rack}", 60, [SpreadTarget("r0", 30), SpreadTarget("r1", 30)])]
    job.task_groups[0].spreads = [Spread("${attr.zone}", 40, [])]
    return nodes, allocs, job, upd


@gpu
def test_job_and_group_spreads_with_missing_values():                   # (c)
    nodes, allocs, job, upd = _shape_c()
    stacks, a = _same(_three(nodes, allocs, job, upd))
    assert 0 in a[1]
    by_id = {n.id: n for n in nodes}
    parts, _ = spread_model(nodes, allocs, job, 0, upd, a[1])
    both = [p for i, p in zip(upd, parts) if p is not None and "rack" not in by_id[allocs[i].node_id].meta
            and "zone" not in by_id[allocs[i].node_id].attributes]
    assert both and set(both) == {-2.0}                # the -1 boost of either set
    assert [p for p in parts if p] == [x for x, p in zip(_last_parts(a[0]), parts) if p]
    _assert_same_after(stacks, 64, 23)


@gpu
def test_earlier_stops_and_commits():                                   # (d)
    # eight of the job's allocs are stopped earlier (and not listed); a commit
    # follows on the nodes of the first four, so their classes are proposed too
    nodes, allocs, job, upd, stops, _ = _prepared(8, 0, seed=86)
    job.task_groups[0].spreads = [TARGET]
    logs = []

    def prep(st):
        st.StopAllocs(stops)
        logs.append([])
        for ai in stops[:4]:
            st.SetNodes([st.row(allocs[ai].node_id)])
            opt = st.Select(0)
            if opt is not None:
                st.Commit(0, opt.row)
                logs[-1].append(opt.row)

    stacks, a = _same(_three(nodes, allocs, job, upd, prep=prep))
    assert 0 in a[1] and 2 in a[1]
    assert logs[0] == logs[1] == logs[2] and len(logs[0]) >= 2   # the same plan on all three
    rows = logs[0]
    _, cols = spread_model(nodes, allocs, job, 0, upd, a[1], plan_nodes=[stacks[0].nodes[r].id for r in rows],
                           stopped=stops)
    ep0, craw0, prop0 = cols[0]
    assert any(craw0.get(v, 0) > 1 and v in prop0 for v in ep0)
    _assert_same_after(stacks, 64, 24)


@gpu
def test_listed_alloc_of_another_group():                               # (e)
    nodes, allocs, job, upd = _shape_a([TARGET], seed=87, own=120)
    job.task_groups.append(TaskGroup(name="side", count=20, tasks=[Task(name="s", driver="exec", cpu=300,
                                                                         memory_mb=128)]))
    side = []
    for k in range(0, 40, 2):
        side.append(len(allocs))
        allocs.append(Allocation(node_id=nodes[k].id, job_id="svc-c2", task_group="side", cpu_shares=300,
                                 memory_mb=128, disk_mb=150, priority=50))
    upd = upd[:40] + side[:10] + upd[40:80] + side[10:] + upd[80:]
    stacks, a = _same(_three(nodes, allocs, job, upd))
    where = {i: k for k, i in enumerate(upd)}
    assert sum(1 for i in side if a[1][where[i]] == 0) >= 10   # updated: they move ks, never kc
    parts, _ = spread_model(nodes, allocs, job, 0, upd, a[1])
    assert [p for p in parts if p] == [x for x, p in zip(_last_parts(a[0]), parts) if p]
    _assert_same_after(stacks, 64, 25)


@gpu
def test_chunk_boundaries_are_crossed():                                # (f)
    nodes, allocs, job, upd = _multi_own(64, 3 * CHUNK - 40, seed=88, cpu=520, mem=260)
    job.spreads = [TARGET]
    job.task_groups[0].spreads = [Spread("${attr.cpu.arch}", 40, [])]
    assert len(upd) >= 2.5 * CHUNK
    stacks, a = _same(_three(nodes, allocs, job, upd))
    for c in range(0, len(upd), CHUNK):
        assert 0 in a[1][c:c + CHUNK]                  # updates in every chunk
    parts, _ = spread_model(nodes, allocs, job, 0, upd, a[1])
    assert [p for p in parts if p] == [x for x, p in zip(_last_parts(a[0]), parts) if p]
    _assert_same_after(stacks, 64, 26)


@gpu
def test_set_larger_than_lds():                                         # (g)
    n = 2100
    assert n > LDS_VALUES
    nodes, allocs, job, upd = _multi_own(n, 300, seed=89)
    job.task_groups[0].spreads = [Spread("${node.unique.id}", 50, [])]
    stacks, a = _same(_three(nodes, allocs, job, upd))
    assert a[1].count(0) >= 100
    assert len({k[2][-1] for k in a[0] if k is not None}) >= 2
    _assert_same_after(stacks, n, 27, count=10)


@gpu
def test_metrics_on():                                                  # (h)
    nodes, allocs, job, upd = _shape_a([TARGET], own=150)
    job.spreads = [Spread("${attr.cpu.arch}", 40, [])]
    (eng, a, ra), (ora, b, rb), (eng2, c, rc) = _three(nodes, allocs, job, upd, metrics=True)
    _well_formed(ra)
    assert a == c                                      # bit-equal, the maps included
    assert a[:2] == b[:2]                              # records and statuses against the oracle, bit for bit
    _same_metrics_oracle(ra[2], rb[2])
    items = 0
    for k, m in zip(a[0], ra[2]):                      # the allocation-spread item is the record's last part
        part = m["ScoreMetaData"][0][2].get("allocation-spread") if m["ScoreMetaData"] else None
        if part is not None:
            assert part != 0.0 and part == k[2][-1]
            items += 1
    assert items >= 80
    # the maps alone (out == NULL): the same maps
    from nomad_amd.stack import GenericStack
    alone = _setup(GenericStack, nodes, allocs, job)
    alone.EnableMetrics(True)
    rc_, _, status, updated = _raw(alone, "pe_inplace_update_spread", upd, records=False)
    assert rc_ == abi.PE_OK and status == a[1] and updated == a[1].count(0)
    assert alone.InplaceMetrics(status) == ra[2]
    _assert_same_after((eng, ora, eng2), 64, 28)


def _raw(st, name, upd, records=True):
    n = len(upd)
    arr = np.asarray(upd or [0], dtype=np.uint32)
    out = (abi.pe_ranked_node * max(1, n))() if records else None
    status = np.full(max(1, n), 255, dtype=np.uint8)
    updated = C.c_uint32(0)
    rc = getattr(st._lib, name)(st._h, 0, arr.ctypes.data_as(abi.u32p), n, out, status.ctypes.data_as(abi.u8p),
                                C.byref(updated))
    return rc, out, status[:n].tolist(), updated.value


@gpu
def test_statuses_only_when_no_records_are_asked_for():                 # (i)
    from nomad_amd.stack import GenericStack
    nodes, allocs, job, upd = _shape_a([TARGET], seed=90, own=120)
    eng = _setup(GenericStack, nodes, allocs, job)
    eng2 = _setup(GenericStack, nodes, allocs, job)
    want = _keys(eng2.InplaceUpdateSpread(0, upd, fallback=False)[:2])
    assert eng2.inplace_stage_ms()[1] > 0.0            # the second stage ran
    rc, _, status, updated = _raw(eng, "pe_inplace_update_spread", upd, records=False)
    assert rc == abi.PE_OK and status == want[1] and updated == want[1].count(0)
    assert 0 in want[1] and 2 in want[1]
    assert eng.inplace_stage_ms()[1] == 0.0            # ... and here it did not
    perm = synth.shuffle(64, 21)
    eng.SetNodes(perm)
    eng2.SetNodes(perm)
    assert _loop(eng, 30) == _loop(eng2, 30)
    assert eng.Eligibility() == eng2.Eligibility()


@gpu
def test_system_stack_drops_the_spreads():                              # (j)
    from nomad_amd.stack import SystemStack
    n = 300
    nodes, allocs = synth.cluster_c4(n, seed=91)
    rng = np.random.Generator(np.random.PCG64(92))
    base = len(allocs)
    for k in range(n):
        if rng.random() < 0.8:
            allocs.append(Allocation(node_id=nodes[k].id, job_id="mock-system-0", task_group="web", cpu_shares=500,
                                     memory_mb=256, disk_mb=300, net_mbits=50, dyn_ports=1, priority=100))
    job = synth.mock_system_job()
    job.version = 4
    job.task_groups[0].tasks[0].cpu = 1500
    job.spreads = [Spread("${node.class}", 50, [])]
    job.task_groups[0].spreads = [Spread("${node.datacenter}", 50, [SpreadTarget("dc1", 70)])]
    upd = [base + int(k) for k in rng.permutation(len(allocs) - base)]
    (eng, a, _), (ora, b, _), (eng2, c, _) = _three(nodes, allocs, job, upd, system=True)
    assert a == c                                      # engine against engine: bit for bit
    assert a[1] == b[1] and 0 in a[1]
    assert [k and (k[0], k[1]) for k in a[0]] == [k and (k[0], k[1]) for k in b[0]]
    assert eng.inplace_stage_ms()[1] == 0.0            # no spread sets reach the stack: no second stage
    plain = _setup(SystemStack, nodes, allocs, job)
    assert _keys(plain.InplaceUpdate(0, upd, fallback=False)) == a
    assert eng.Eligibility() == ora.Eligibility() == eng2.Eligibility()


@gpu
def test_without_spreads_it_is_the_metrics_call():                      # (k)
    from nomad_amd.stack import GenericStack
    nodes, allocs, job, upd = _multi_own(64, 120, seed=93)
    for metrics in (False, True):
        x, y = (_setup(GenericStack, nodes, allocs, job) for _ in range(2))
        if metrics:
            x.EnableMetrics(True)
            y.EnableMetrics(True)
        rx = _raw(x, "pe_inplace_update_spread", upd)
        ry = _raw(y, "pe_inplace_update_metrics", upd)
        assert rx[0] == ry[0] == abi.PE_OK
        assert bytes(rx[1]) == bytes(ry[1]) and rx[2:] == ry[2:] and 0 in rx[2]
        assert x.inplace_stage_ms()[1] == 0.0
        if metrics:
            assert x.InplaceMetrics(rx[2]) == y.InplaceMetrics(ry[2])


def _refusals():
    def distinct_property(job):
        job.constraints.append(Constraint("${meta.database}", "3", "distinct_property"))

    def distinct_property_in_the_group(job):
        job.task_groups[0].constraints.append(Constraint("${node.class}", "100", "distinct_property"))

    def cores(job):
        job.task_groups[0].tasks[0].cores = 1

    def static_ports(job):
        job.task_groups[0].network = NetworkResource(mode="host", reserved_ports=[8080], port_labels=["http"])

    return {"distinct_property": distinct_property, "distinct_property in the group": distinct_property_in_the_group,
            "a reserved-cores ask": cores, "static ports": static_ports}


@gpu
@pytest.mark.parametrize("case", sorted(_refusals()))
def test_refusals_leave_the_handle_as_it_was(case):                     # (l)
    from nomad_amd.stack import GenericStack, Unsupported
    nodes, allocs, job, upd = _shape_a([TARGET], seed=94, own=40)
    _refusals()[case](job)
    eng = _setup(GenericStack, nodes, allocs, job)
    rc, _, status, _ = _raw(eng, "pe_inplace_update_spread", upd)
    assert rc == abi.PE_EUNSUPPORTED and set(status) == {255}
    with pytest.raises(Unsupported):
        eng.InplaceUpdateSpread(0, upd, fallback=False)
    fresh = _setup(GenericStack, nodes, allocs, job)
    try:
        want = _keys(inplace_update_by_select(fresh, 0, upd))
    except Unsupported:
        # the engine's own Select refuses this job too: the refused handle's answer as well
        with pytest.raises(Unsupported):
            inplace_update_by_select(eng, 0, upd)
        return
    ora = _setup(OracleGenericStack, nodes, allocs, job)
    assert _keys(inplace_update_by_select(ora, 0, upd)) == want
    assert _keys(eng.InplaceUpdateSpread(0, upd)[:2]) == want   # the refusal changed nothing; the fallback answers
    assert len(want[1]) == len(upd)


@gpu
def test_the_three_earlier_calls_still_refuse_spreads():
    from nomad_amd.stack import GenericStack
    nodes, allocs, job, upd = _shape_a([TARGET], seed=94, own=40)
    eng = _setup(GenericStack, nodes, allocs, job)
    for name in ("pe_inplace_update", "pe_inplace_update_preempt", "pe_inplace_update_metrics"):
        rc, _, status, _ = _raw(eng, name, upd)
        assert rc == abi.PE_EUNSUPPORTED and set(status) == {255}
    assert eng.InplaceUpdateSpread(0, [], fallback=False) == ([], [], None)
