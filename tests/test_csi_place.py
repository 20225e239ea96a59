"""pe_place_csi: computePlacements' loop for a task group with CSI requests in
one launch (k_csi_first, k_csi_loop), and the LimitIterator / MaxScoreIterator
fold with transient nils that the kernel steps (csi_limit.h, pe_csi_limit_fold).

Reference (the oracle has no CSI): `limit_max` / `Ref`, a sequential
restatement of FeasibilityWrapper.Next (scheduler/feasible.go:1061-1153),
LimitIterator (select.go:35-67) and MaxScoreIterator (select.go:95-116) over a
source that returns nil at an unavailable node of a class already memoised
eligible and goes on with the following node when asked again. The oracle
scores the options one node at a time (the job without its CSI requests) and
commits each winner. `test_restatement_equals_oracle_limit_iterator` pins the
restatement to the oracle's LimitIterator on streams without a transient nil.

Column de-duplication: the engine keeps one code column per distinct set of
*resolved request records* (volume found, plugin, volume-level reason), so the
alloc indices [0, 3, 0, 3] of `per_alloc_cluster`, whose vol[0] and vol[3] both
resolve to plugin foo with no volume-level reason, share one column (one
k_csi_avail launch); [0, 1, 0, 1] needs two.
"""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from nomad_amd import abi, synth
from nomad_amd.structs import (Affinity, Allocation, CSINodePlugin, CSIVolume, CSIVolumeRequest, RequestedDevice,
                               SchedulerConfig, Spread, SpreadTarget, Task, TaskGroup)

from test_csi import NS, STOP_REQS, csi_job, engine_generic, engine_system, engine_with, plain, same_option, stop_cluster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nomad_amd", "libnomadpe.so")
CSRC = os.path.join(ROOT, "nomad_amd", "csrc")
MAX_SKIP = 3


# ---- the restatement ---------------------------------------------------------------

def limit_max(stream, limit, max_skip=MAX_SKIP, thr=0.0):
    """stream() -> (kind, id, score) | None (a transient nil, or the end again and
    again). Returns (best, trace, seen, order, ended_nil): the first strict
    maximum in return order, the event kinds met ('pop', 'dup', 'nilD'),
    LimitIterator.seen, the options in return order, and whether the Select
    ended at a nil Next (else at seen == limit)."""
    seen, skipped, si, best, trace, order = 0, [], 0, None, [], []

    def next_option():
        nonlocal si
        x = stream()
        if x is None and si < len(skipped):
            trace.append('pop')
            x = skipped[si]
            si += 1
        return x

    while True:
        o = None
        if seen != limit:
            o = next_option()
            if o is not None:
                if len(skipped) < max_skip:
                    while o is not None and o[2] <= thr and len(skipped) < max_skip:
                        if o in skipped:
                            trace.append('dup')
                        skipped.append(o)
                        o = stream()
                        if o is None:
                            trace.append('nilD')
                seen += 1
                if o is None:
                    o = next_option()
        if o is None:
            return best, trace, seen, order, seen != limit
        order.append(o)
        if best is None or o[2] > best[2]:
            best = o


def list_stream(items):
    """A recorded stream: item i is ('opt', i, score) or None; past the end, None for ever."""
    state = {"k": 0}

    def stream():
        if state["k"] >= len(items):
            return None
        x = items[state["k"]]
        state["k"] += 1
        return x
    return stream, state


def restated(scores, kinds, limit):
    items = [None if k else ("opt", i, float(s)) for i, (s, k) in enumerate(zip(scores, kinds))]
    stream, state = list_stream(items)
    best, trace, seen, order, ended_nil = limit_max(stream, limit)
    return (best[1] if best else -1, seen, state["k"], int(ended_nil)), trace, order


def fold_lib():
    return abi.bind_csi_limit_fold(C.CDLL(LIB))


def folded(lib, scores, kinds, limit):
    s = np.ascontiguousarray(np.asarray(scores, dtype=np.float64))
    k = np.ascontiguousarray(np.asarray(kinds, dtype=np.uint8))
    w, seen, used, nil = C.c_int32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    rc = lib.pe_csi_limit_fold(s.ctypes.data_as(abi.f64p), k.ctypes.data_as(abi.u8p), len(scores), limit,
                               C.byref(w), C.byref(seen), C.byref(used), C.byref(nil))
    assert rc == 0
    return w.value, seen.value, used.value, nil.value


# ---- CPU tests ----------------------------------------------------------------------

def test_restatement_equals_oracle_limit_iterator():
    from oracle import oracle
    rng = np.random.Generator(np.random.PCG64(5))
    cases = [list(p) for n in range(0, 6) for p in itertools.product([1.0, 0.0, -1.0], repeat=n)]
    cases += [[float(x) for x in rng.choice([-0.5, 0.0, 0.25, 0.25, 0.75], size=int(rng.integers(6, 30)))]
              for _ in range(300)]
    for scores in cases:
        for limit in (1, 2, 3, 4, 7):
            want_order, want_winner, want_pulled = oracle.limit_iter(scores, limit=limit, threshold=0.0, max_skip=MAX_SKIP)
            (winner, seen, pulled, _), trace, order = restated(scores, [0] * len(scores), limit)
            assert [o[1] for o in order] == want_order, (scores, limit)
            assert (winner, pulled) == (want_winner, want_pulled), (scores, limit)
            assert seen == len(want_order)


EVENTS = [(1.0, 0), (0.0, 0), (0.0, 1)]   # positive option, non-positive option, nil


def exhaustive_streams(max_len=7):
    for n in range(0, max_len + 1):
        for combo in itertools.product(range(3), repeat=n):
            yield [EVENTS[c][0] for c in combo], [EVENTS[c][1] for c in combo]


def test_fold_equals_restatement_on_every_short_stream():
    lib = fold_lib()
    kinds_met = set()
    total = 0
    for scores, kinds in exhaustive_streams():
        for limit in (1, 2, 3, 4):
            want, trace, _ = restated(scores, kinds, limit)
            assert folded(lib, scores, kinds, limit) == want, (scores, kinds, limit)
            kinds_met |= set(trace)
            total += 1
    assert total == 4 * sum(3 ** n for n in range(8))
    assert kinds_met == {'pop', 'dup', 'nilD'}


def test_fold_equals_restatement_on_random_long_streams():
    """Bit-equal scores, so the return order decides the winner."""
    lib = fold_lib()
    rng = np.random.Generator(np.random.PCG64(11))
    values = [0.5, 0.5, 0.25, 0.0, -0.25, -0.25]
    popped_won = 0
    for _ in range(4000):
        n = int(rng.integers(8, 60))
        scores = [float(values[int(i)]) for i in rng.integers(0, len(values), n)]
        kinds = [int(x < 0.2) for x in rng.random(n)]
        if rng.random() < 0.3:      # every option non-positive: a popped option against later equal scores
            scores = [min(s, 0.0) if s != 0.5 else -0.25 for s in scores]
        limit = int(rng.integers(1, 9))
        want, trace, order = restated(scores, kinds, limit)
        assert folded(lib, scores, kinds, limit) == want, (scores, kinds, limit)
        if 'pop' in trace and order and want[0] >= 0 and sum(1 for o in order if o[2] == scores[want[0]]) > 1:
            popped_won += 1
    assert popped_won > 50


def test_fold_limit_zero_and_empty_stream():
    lib = fold_lib()
    assert folded(lib, [1.0], [0], 0) == (-1, 0, 0, 0)
    assert folded(lib, [], [], 3) == (-1, 0, 0, 1)


SANITIZED_MAIN = r"""
#include <cstdio>
#include <vector>
#include "csi_limit.h"
// every stream of length <= 7 over {positive option, non-positive option, nil}, limits 1 to 4:
// prints winner, seen, consumed, ended_nil per case
int main() {
    const double sc[3] = {1.0, 0.0, 0.0};
    const unsigned kd[3] = {pe::kCsiOption, pe::kCsiOption, pe::kCsiNil};
    unsigned long cases = 0;
    for (int n = 0; n <= 7; n++) {
        long total = 1;
        for (int i = 0; i < n; i++) total *= 3;
        for (long code = 0; code < total; code++) {
            std::vector<int> ev((size_t)n);
            long c = code;
            for (int i = n - 1; i >= 0; i--) { ev[(size_t)i] = (int)(c % 3); c /= 3; }
            for (unsigned limit = 1; limit <= 4; limit++) {
                pe::CsiLimit L;
                bool done = pe::csi_limit_init(L, limit);
                unsigned used = 0;
                while (!done && used < (unsigned)n) {
                    done = pe::csi_limit_step(L, kd[ev[used]], sc[ev[used]], (int)used);
                    used++;
                }
                for (int t = 0; t < pe::kCsiTailEvents && !done; t++) done = pe::csi_limit_step(L, pe::kCsiNil, 0.0, -1);
                if (!done) { std::printf("unbounded\n"); return 2; }
                std::printf("%d %u %u %u\n", L.best_id, L.seen, used, L.ended_nil);
                cases++;
            }
        }
    }
    std::fprintf(stderr, "%lu cases\n", cases);
    return 0;
}
"""


def test_fold_header_under_sanitizers(tmp_path):
    """csi_limit.h and a small main of its own, built with AddressSanitizer and
    UBSan as a stand-alone host program, over the exhaustive set."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "fold_main.cpp"
    src.write_text(SANITIZED_MAIN)
    exe = tmp_path / "fold_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    lines = out.stdout.decode().split("\n")[:-1]
    want = []
    for scores, kinds in exhaustive_streams():
        for limit in (1, 2, 3, 4):
            want.append("%d %d %d %d" % restated(scores, kinds, limit)[0])
    assert lines == want
    assert b"runtime error" not in out.stderr and b"AddressSanitizer" not in out.stderr


# ---- the reference run for the engine tests --------------------------------------------

class Ref:
    """The count loop by the restatement. `unavailable(i)` -> the set of rows the
    CSI checker fails for placement i; `known` maps a computed class to True once
    its task-group status is memoised eligible (every node of these clusters
    passes the job's and the group's checks)."""

    def __init__(self, nodes, perm, job, allocs, limit, cursor=0, known=None, job_fail=()):
        from oracle.oracle import OracleGenericStack
        self.nodes, self.perm, self.limit, self.cursor = nodes, list(perm), limit, cursor
        self.o = OracleGenericStack()
        self.o.SetState(nodes, list(allocs))
        self.o.SetJob(plain(job))
        self.known = dict(known or {})
        self.job_seen = set(self.known)
        self.traces, self.stops = [], []
        # rows that fail the checks of a job with escaped constraints: they run per node, before the
        # group's entry of the class is looked at, and write no job-level entry (feasible.go:1075-1096)
        self.job_fail = set(job_fail)

    def option(self, row):
        self.o.SetNodes([row])
        return self.o.SelectRaw(0)

    def select(self, unavailable):
        n = len(self.perm)
        st = {"k": 0, "filtered": 0, "exhausted": 0, "stops": 0}
        recs = {}

        def stream():
            while st["k"] < n:
                row = self.perm[(self.cursor + st["k"]) % n]
                st["k"] += 1
                cls = self.nodes[row].computed_class
                if row in self.job_fail:
                    st["filtered"] += 1
                    continue
                self.job_seen.add(cls)
                if row in unavailable:
                    st["filtered"] += 1
                    if self.known.get(cls):
                        st["stops"] += 1
                        return None
                    self.known[cls] = True
                    continue
                self.known[cls] = True
                r = self.option(row)
                if r.row < 0:
                    st["filtered"] += r.nodes_filtered
                    st["exhausted"] += r.nodes_exhausted
                    continue
                recs[row] = r
                return ("opt", row, r.final_score)
            return None

        best, trace, _, _, _ = limit_max(stream, self.limit)
        self.traces.append(trace)
        self.stops.append(st["stops"])
        self.cursor = (self.cursor + st["k"]) % n
        want = dict(row=-1, final_score=0.0, scores=[], nodes_evaluated=st["k"], nodes_filtered=st["filtered"],
                    nodes_exhausted=st["exhausted"], new_offset=self.cursor)
        if best is not None:
            r = recs[best[1]]
            want.update(row=r.row, final_score=r.final_score, scores=list(r.scores))
            self.o.Commit(0, r.row)
        return want

    def run(self, count, unavailable):
        out = []
        for i in range(count):
            out.append(self.select(unavailable(i) if callable(unavailable) else unavailable))
            if out[-1]["row"] < 0:
                break
        return out

    def eligibility(self, tg="web"):
        decided = {c: True for c, v in self.known.items() if v}
        return {"job": {c: True for c in self.job_seen}, "tgs": {tg: decided} if decided else {}, "escaped": False}


def assert_records(got, want):
    assert len(got) == len(want), ([g.row for g in got], [w["row"] for w in want])
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.row == w["row"], (k, g.row, w)
        if w["row"] >= 0:
            assert g.final_score == w["final_score"] and list(g.scores) == w["scores"], k
        assert (g.nodes_evaluated, g.nodes_filtered, g.nodes_exhausted, g.new_offset) == \
            (w["nodes_evaluated"], w["nodes_filtered"], w["nodes_exhausted"], w["new_offset"]), (k, w)


def same_record(g, w):
    same_option(g, w)
    assert (g.nodes_evaluated, g.nodes_filtered, g.nodes_exhausted, g.new_offset) == \
        (w.nodes_evaluated, w.nodes_filtered, w.nodes_exhausted, w.new_offset)


def job_allocs(nodes, perm, job, positions):
    return [Allocation(nodes[perm[p]].id, job.id, "web", cpu_shares=500, memory_mb=256) for p in positions]


def class_elig(nodes, tg="web"):
    classes = {nd.computed_class for nd in nodes}
    return {"job": {c: True for c in classes}, "tgs": {tg: {c: True for c in classes}}}


def two_group_job(count):
    return csi_job(STOP_REQS, count=count, extra_group=True)


def assert_plan_matches(e, nodes, volumes, node_volumes, job, perm, allocs, rows):
    """The plan, through a following Select of the plain second group against a
    handle that committed the same rows one by one."""
    f = engine_with(nodes, volumes, node_volumes, job, perm, allocs=allocs)
    for r in rows:
        f.Commit(0, r)
    e.SetNodes(perm)
    f.SetNodes(perm)
    same_record(e.SelectRaw(1), f.SelectRaw(1))


# ---- GPU: parity with the restatement where pe_select gives up ---------------------------

PARITY_CASES = [
    ((5, 8, 11), (1, 9, 13)),                 # a nil in the skip loop, then a pop with a duplicate append
    ((1, 2, 4, 5, 9, 13), (6, 8, 14)),        # two stops and two pops in one Select
    ((0, 4, 7, 9, 12), (2, 14)),              # a pop and a duplicate in two consecutive Selects
    ((0, 3, 4, 5, 6, 10), (7, 9, 11)),        # a failed second Select: one position, one stop
]


def parity_setup(P, U, count=4, memo="put"):
    nodes, perm, volumes, node_volumes = stop_cluster(unavailable=U)
    job = two_group_job(count)
    allocs = job_allocs(nodes, perm, job, P)
    e = engine_with(nodes, volumes, node_volumes, job, perm, allocs=allocs)
    if memo == "put":
        e.PutEligibility(class_elig(nodes))
    known = {nodes[0].computed_class: True}
    ref = Ref(nodes, perm, job, allocs, e.limit, known=known)
    return nodes, perm, volumes, node_volumes, job, allocs, e, ref


def run_parity(P, U, count=4):
    nodes, perm, volumes, node_volumes, job, allocs, e, ref = parity_setup(P, U, count)
    lacking = {perm[p] for p in U}
    want = ref.run(count, lacking)
    got = e.PlaceCSI(0, count)
    assert_records(got, want)
    assert_after_call(e, ref, want, nodes, volumes, node_volumes, job, perm, allocs)
    return ref, want


def assert_after_call(e, ref, want, nodes, volumes, node_volumes, job, perm, allocs):
    """Cursor, Eligibility() and the plan after a PlaceCSI that `ref` restated."""
    assert e.GetCursor() == (ref.cursor, e.limit)
    ee = e.Eligibility()
    assert ee["job"] == ref.eligibility()["job"] and ee["tgs"] == ref.eligibility()["tgs"]
    assert_plan_matches(e, nodes, volumes, node_volumes, job, perm, allocs, [w["row"] for w in want if w["row"] >= 0])


@pytest.mark.gpu
def test_parity_with_restatement_where_select_gives_up():
    kinds, two_stops, nil_option, resumed = set(), False, False, False
    for P, U in PARITY_CASES:
        ref, want = run_parity(P, U)
        for trace, stops in zip(ref.traces, ref.stops):
            kinds |= set(trace)
            two_stops = two_stops or stops >= 2
            resumed = resumed or ('pop' in trace and stops >= 1)
        nil_option = nil_option or want[-1]["row"] < 0
    # every event kind is reached (a changed synth cannot empty the test silently)
    assert kinds == {'pop', 'dup', 'nilD'}
    assert two_stops and nil_option and resumed


@pytest.mark.gpu
def test_popped_option_wins_against_a_later_equal_score():
    """Allocs of the job on every node of the first window (two on position 3):
    every option of the Select is non-positive. Positions 0 to 2 are set aside,
    position 3 is returned, the stop at position 4 pops position 0, which then
    precedes the bit-equal options returned after it and wins."""
    U = (4,)
    P = tuple(p for p in range(0, 14) if p not in U) + (3,)
    nodes, perm, volumes, node_volumes, job, allocs, e, ref = parity_setup(P, U, count=4)
    want = ref.run(2, {perm[4]})
    assert ref.traces[0] == ['pop'] and want[0]["row"] == perm[0] and want[0]["final_score"] <= 0.0
    later = [ref.option(perm[p]).final_score for p in (5, 6, 7)]
    assert want[0]["final_score"] in later          # (position 0 now holds the placement; 5 to 7 are as they were)
    got = e.PlaceCSI(0, 2)
    assert_records(got, want)
    assert_after_call(e, ref, want, nodes, volumes, node_volumes, job, perm, allocs)


# ---- GPU: agreement with the existing per-placement path -----------------------------------

def per_placement(e, count, alloc_idx=None):
    """CSIAllocIndex / SelectRaw / Commit per placement; None where pe_select hands the Select back."""
    from nomad_amd.stack import Unsupported
    out = []
    for i in range(count):
        if alloc_idx is not None:
            e.CSIAllocIndex(0, alloc_idx[i])
        try:
            r = e.SelectRaw(0)
        except Unsupported:
            out.append(None)
            break
        out.append(r)
        if r.row < 0:
            break
        e.Commit(0, r.row)
    return out


@pytest.mark.gpu
def test_agreement_with_per_placement_sequence():
    handed_back, whole_runs = 0, 0
    cases = PARITY_CASES + [((), (0, 5)), ((), (2, 3, 30))]
    for P, U in cases:
        nodes, perm, volumes, node_volumes, job, allocs, e, _ = parity_setup(P, U)
        _, _, _, _, _, _, e2, _ = parity_setup(P, U)
        got = e.PlaceCSI(0, 4)
        seq = per_placement(e2, 4)
        for k, r in enumerate(seq):
            if r is None:
                handed_back += 1
                break
            same_record(got[k], r)
            assert list(got[k].scores) == list(r.scores)
        else:
            whole_runs += 1
            assert len(seq) == len(got)
            assert e.GetCursor() == e2.GetCursor() and e.Eligibility() == e2.Eligibility()
    assert handed_back >= 1 and whole_runs >= 1


# ---- GPU: two classes --------------------------------------------------------------------

@pytest.mark.gpu
def test_two_classes_one_decided_during_the_call():
    """Plugin nodes carry meta.csi (class A), the nodes without the plugin form
    class B. A is memoised at call start, B is decided during the second Select:
    an unavailable node of B before its deciding position is a skip, the ones
    after it are stops."""
    U = (7, 9, 12, 20)
    nodes, perm, volumes, node_volumes = stop_cluster(unavailable=U, meta_on_plugin_nodes=True)
    cls_a, cls_b = nodes[perm[0]].computed_class, nodes[perm[7]].computed_class
    assert cls_a != cls_b and {nodes[perm[p]].computed_class for p in U} == {cls_b}
    job = two_group_job(6)
    allocs = job_allocs(nodes, perm, job, (8, 10))
    e = engine_with(nodes, volumes, node_volumes, job, perm, allocs=allocs)
    e.PutEligibility({"job": {cls_a: True}, "tgs": {"web": {cls_a: True}}})
    ref = Ref(nodes, perm, job, allocs, e.limit, known={cls_a: True})
    want = ref.run(6, {perm[p] for p in U})
    assert want[0]["nodes_evaluated"] <= 7 < want[0]["nodes_evaluated"] + want[1]["nodes_evaluated"]
    assert ref.stops[0] == 0 and sum(ref.stops) >= 1          # position 7 a skip, a later one a stop
    assert sum(w["nodes_filtered"] for w in want) > sum(ref.stops)
    got = e.PlaceCSI(0, 6)
    assert_records(got, want)
    assert e.GetCursor() == (ref.cursor, e.limit)
    ee = e.Eligibility()
    assert ee["tgs"] == {"web": {cls_a: True, cls_b: True}} and ee["job"] == {cls_a: True, cls_b: True}


@pytest.mark.gpu
def test_escaped_job_node_before_the_deciding_position():
    """A job constraint on node.unique.id escapes the class: the job checks run
    per node. The node at position 0 fails them (and lacks the plugin): it is
    filtered and decides nothing. Position 1 lacks the plugin and passes: it is
    F[c], a skip that decides the class. Position 5 is then a stop. If F[c]
    counted position 0, position 1 would end the first Select at once."""
    from nomad_amd.structs import Constraint
    U = (0, 1, 5)
    nodes, perm, volumes, node_volumes = stop_cluster(unavailable=U)
    job = csi_job(STOP_REQS, count=4, extra_group=True,
                  constraints=[Constraint("${node.unique.id}", nodes[perm[0]].id, "!=")])
    allocs = job_allocs(nodes, perm, job, (2, 3))
    e = engine_with(nodes, volumes, node_volumes, job, perm, allocs=allocs)
    ref = Ref(nodes, perm, job, allocs, e.limit, job_fail={perm[0]})
    want = ref.run(3, {perm[p] for p in U})
    assert want[0]["row"] >= 0 and want[0]["nodes_filtered"] >= 3 and ref.stops[0] == 1
    got = e.PlaceCSI(0, 3)
    assert_records(got, want)
    assert e.GetCursor() == (ref.cursor, e.limit)
    ee = e.Eligibility()
    assert ee["escaped"] and ee["tgs"] == ref.eligibility()["tgs"]
    assert_plan_matches(e, nodes, volumes, node_volumes, job, perm, allocs, [w["row"] for w in want if w["row"] >= 0])


# ---- GPU: per_alloc -------------------------------------------------------------------------

PER_ALLOC_REQS = [CSIVolumeRequest("vol", per_alloc=True)]


def per_alloc_cluster(n_extra_sets=0):
    """vol[0] and vol[3] on plugin foo (every node), vol[1] on plugin bar (the
    nodes at even visit positions), vol[2] absent; `n_extra_sets` further
    volumes vol[10 + k] on plugins of their own that no node runs."""
    nodes, _ = synth.cluster_c1(64, seed=9)
    perm = [int(x) for x in synth.shuffle(64, 10)]
    for p, r in enumerate(perm):
        nodes[r].csi_node_plugins = {"foo": CSINodePlugin(True)}
        if p % 2 == 0:
            nodes[r].csi_node_plugins["bar"] = CSINodePlugin(True)
    volumes = [CSIVolume("vol[0]", NS, "foo"), CSIVolume("vol[1]", NS, "bar"), CSIVolume("vol[3]", NS, "foo")]
    volumes += [CSIVolume("vol[%d]" % (10 + k), NS, "plugin-%d" % k) for k in range(n_extra_sets)]
    return nodes, perm, volumes, {}


def per_alloc_unavailable(perm, idx):
    if idx in (0, 3):
        return set()
    if idx == 1:
        return {r for p, r in enumerate(perm) if p % 2}
    return set(perm)


@pytest.mark.gpu
def test_per_alloc_indices_and_columns():
    nodes, perm, volumes, node_volumes = per_alloc_cluster()
    job = csi_job(PER_ALLOC_REQS, count=4, extra_group=True)
    allocs = job_allocs(nodes, perm, job, (1, 4))

    def fresh():
        e = engine_with(nodes, volumes, node_volumes, job, perm, allocs=allocs)
        e.PutEligibility(class_elig(nodes))
        return e

    known = {nodes[0].computed_class: True}
    for idx in ([0, 1, 3], [0, 1, 2, 3]):
        e = fresh()
        ref = Ref(nodes, perm, job, allocs, e.limit, known=known)
        want = ref.run(len(idx), lambda i: per_alloc_unavailable(perm, idx[i]))
        got = e.PlaceCSI(0, len(idx), alloc_idx=idx)
        assert_records(got, want)
        assert e.GetCursor() == (ref.cursor, e.limit)
        if len(idx) == 4:      # vol[2] does not exist: the third Select is nil at its first position
            assert len(got) == 3 and got[2].row < 0 and got[2].nodes_evaluated == 1
        seq = per_placement(fresh(), len(idx), idx)
        for g, r in zip(got, seq):
            if r is None:
                break
            same_record(g, r)
    # one k_csi_avail launch per distinct set of resolved records
    for idx, launches in (([0, 1, 0, 1], 2), ([0, 3, 0, 3], 1), ([1, 1, 1, 1], 1), ([0, 1, 3, 2], 3)):
        e = fresh()
        e.CSICheck(0)              # the group's own column is up to date
        before = e.csi_avail_launches()
        e.PlaceCSI(0, 4, alloc_idx=idx)
        assert e.csi_avail_launches() - before == launches, idx


@pytest.mark.gpu
def test_one_record_set_beyond_the_cap_is_refused_untouched():
    from nomad_amd.stack import Unsupported
    nodes, perm, volumes, node_volumes = per_alloc_cluster(n_extra_sets=abi.PE_MAX_CSI_SETS)
    job = csi_job(PER_ALLOC_REQS, count=12, extra_group=True)
    e = engine_with(nodes, volumes, node_volumes, job, perm)
    f = engine_with(nodes, volumes, node_volumes, job, perm)
    cursor, elig = e.GetCursor(), e.Eligibility()
    idx = [0] + [10 + k for k in range(abi.PE_MAX_CSI_SETS)]       # foo + 8 plugins of their own: 9 sets
    with pytest.raises(Unsupported, match="distinct CSI record sets"):
        e.PlaceCSI(0, len(idx), alloc_idx=idx)
    assert_untouched(e, f, cursor, elig)
    got = e.PlaceCSI(0, len(idx) - 1, alloc_idx=idx[:-1])           # 8 sets are placed
    assert got[0].row >= 0 and got[1].row < 0


def assert_untouched(e, fresh, cursor, elig, tg=1):
    assert e.GetCursor() == cursor
    assert e.Eligibility() == elig
    same_record(e.SelectRaw(tg), fresh.SelectRaw(tg))


# ---- GPU: shapes ------------------------------------------------------------------------------

def shape_cluster(n, U, seed=31):
    nodes, _ = synth.cluster_c1(n, seed=seed)
    perm = [int(x) for x in synth.shuffle(n, seed + 1)]
    lacking = {perm[p] for p in U}
    for r, nd in enumerate(nodes):
        if r not in lacking:
            nd.csi_node_plugins = {"foo": CSINodePlugin(True)}
    return nodes, perm, [CSIVolume("vol", NS, "foo")], {}, lacking


def run_shape(n, U, count, cursor=0, P=(), memo=True):
    nodes, perm, volumes, node_volumes, lacking = shape_cluster(n, U)
    job = csi_job(STOP_REQS, count=4)
    allocs = job_allocs(nodes, perm, job, P)
    e = engine_with(nodes, volumes, node_volumes, job, perm, allocs=allocs)
    known = {}
    if memo:
        e.PutEligibility(class_elig(nodes))
        known = {nodes[0].computed_class: True}
    if cursor:
        e.SetCursor(cursor, e.limit)
    ref = Ref(nodes, perm, job, allocs, e.limit, cursor=cursor, known=known)
    want = ref.run(count, lacking)
    got = e.PlaceCSI(0, count)
    assert_records(got, want)
    assert e.GetCursor() == (ref.cursor, e.limit)
    ee, re_ = e.Eligibility(), ref.eligibility()
    assert ee["job"] == re_["job"] and ee["tgs"] == re_["tgs"]
    return ref, want


P65 = (6, 17, 19, 29, 31, 37, 50, 60, 61)
P130 = (8, 11, 17, 30, 50, 58, 62, 73, 87, 110, 116)


@pytest.mark.gpu
@pytest.mark.parametrize("n,U,count,cursor,P,memo", [
    (1, (), 3, 0, (), True),
    (1, (0,), 2, 0, (), True),
    (2, (1,), 4, 0, (), True),
    (2, (), 5, 1, (0,), True),
    (63, (1, 62), 6, 0, (3, 4), True),
    (65, (1, 63, 64), 6, 60, (61, 62, 2), True),
    (65, (32, 35), 40, 0, P65, True),               # 384 positions: more than twice round a 65-node ring
    (130, (63, 64, 129), 40, 0, P130, True),        # stops at lanes 63 and 0 of a chunk and at the last position; the ring wraps
    (130, (128,), 6, 127, (127, 129, 0, 1), True),  # the cursor three before the end of the list
    (65, tuple(range(65)), 2, 0, (), True),         # every node unavailable: a stop at the first position
    (65, tuple(range(65)), 2, 0, (), False),        # the same, not memoised: a skip, then a stop
])
def test_shapes(n, U, count, cursor, P, memo):
    ref, want = run_shape(n, U, count, cursor=cursor, P=P, memo=memo)
    if count == 40:
        assert len(want) == 40 and sum(w["nodes_evaluated"] for w in want) > 2 * n and sum(ref.stops) >= 9


@pytest.mark.gpu
def test_unmemoised_class_is_decided_by_the_walk():
    """No memo at call start: the first unavailable node is a skip and decides
    the class (F[c] = its position), the next one is a stop."""
    ref, want = run_shape(65, (0, 3, 9), 5, memo=False, P=(1, 2))
    assert ref.stops[0] >= 1 and want[0]["nodes_filtered"] >= 2


# ---- GPU: refusals ------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals_leave_the_handle_untouched():
    from nomad_amd.stack import Unsupported
    nodes, perm, volumes, node_volumes = stop_cluster()
    job = two_group_job(3)

    def pair(j=job, stack=engine_generic, **kw):
        return (engine_with(nodes, volumes, node_volumes, j, perm, stack=stack, **kw),
                engine_with(nodes, volumes, node_volumes, j, perm, stack=stack, **kw))

    def refused(e, f, match, count=3, tg=1):
        cursor, elig = e.GetCursor(), e.Eligibility()
        with pytest.raises(Unsupported, match=match):
            if count > 64:      # refused before anything is written: no record buffer of that size
                out, placed = (abi.pe_ranked_node * 1)(), C.c_uint32(0)
                e._check(e._lib.pe_place_csi(e._h, 0, count, None, out, C.byref(placed)))
            else:
                e.PlaceCSI(0, count)
        assert_untouched(e, f, cursor, elig, tg=tg)

    # metrics on
    e, f = pair()
    e.EnableMetrics(True)
    cursor, elig = e.GetCursor(), e.Eligibility()
    with pytest.raises(Unsupported, match="pe_set_metrics"):
        e.PlaceCSI(0, 3)
    e.EnableMetrics(False)
    assert_untouched(e, f, cursor, elig)
    # several devices
    m, mf = pair(devices=[0, 0])
    cursor, elig = m.GetCursor(), m.Eligibility()
    with pytest.raises(Unsupported, match="several devices"):
        m.PlaceCSI(0, 3)
    assert_untouched(m, mf, cursor, elig)
    # a system stack
    sysjob = synth.mock_system_job("csi-system")
    sysjob.task_groups[0].csi_volumes = list(STOP_REQS)
    sysjob.task_groups.append(TaskGroup(name="plain", count=1, tasks=[Task(name="plain", cpu=300, memory_mb=128)]))
    se, sf = pair(sysjob, stack=engine_system)
    for h in (se, sf):
        h.SetNodes([perm[3]])
    cursor, elig = se.GetCursor(), se.Eligibility()
    with pytest.raises(Unsupported, match="system stack"):
        se.PlaceCSI(0, 1)
    assert_untouched(se, sf, cursor, elig)
    # a preempting stack: the loop would retry a nil Select with Preempt
    e, f = pair(config=SchedulerConfig(preempt_service=True))
    refused(e, f, "preempting stack")
    # a case pe_place itself refuses (the group's `unsupported` route of prepare_tg)
    dev = two_group_job(3)
    dev.task_groups[0].tasks[0].devices = [RequestedDevice("gpu", count=300)]
    e, f = pair(dev)
    refused(e, f, "device request count above 255")
    # a full-pass group (a spread)
    spr = two_group_job(3)
    spr.task_groups[0].spreads = [Spread("${node.datacenter}", 50, [SpreadTarget("dc1", 100)])]
    e, f = pair(spr)
    refused(e, f, "full passes")
    # a full-pass group (an affinity)
    aff = two_group_job(3)
    aff.task_groups[0].affinities = [Affinity("${meta.database}", "mysql", "=", 50)]
    e, f = pair(aff)
    refused(e, f, "full passes")
    # a latched limit: a Select of a full-pass sibling group latched it (stack.go:165-167)
    lat = two_group_job(3)
    lat.task_groups[1].affinities = [Affinity("${meta.database}", "mysql", "=", 50)]
    e, f = pair(lat)
    e.SelectRaw(1)
    f.SelectRaw(1)
    assert e.GetCursor()[1] >= 0x7FFFFFFF
    refused(e, f, "full passes")
    # count beyond the overlay of one launch
    e, f = pair()
    refused(e, f, "overlay", count=1 << 20)
    refused(e, f, "overlay", count=(1 << 31) + 5)    # (a count whose doubling wraps 32 bits)
    # a group without a table is refused as pe_select refuses it
    e, f = pair(csi=False)
    refused(e, f, "CSI volumes")


@pytest.mark.gpu
def test_non_uniform_class_is_refused_untouched():
    from nomad_amd.stack import Unsupported
    from nomad_amd.structs import DriverInfo
    nodes, perm, volumes, node_volumes = stop_cluster()
    nodes[perm[10]].drivers = dict(nodes[perm[10]].drivers, exec=DriverInfo(detected=True, healthy=False))
    job = two_group_job(3)
    job.task_groups[1].tasks[0].driver = "mock_driver"
    e = engine_with(nodes, volumes, node_volumes, job, perm)
    f = engine_with(nodes, volumes, node_volumes, job, perm)
    cursor, elig = e.GetCursor(), e.Eligibility()
    with pytest.raises(Unsupported, match="CSI volumes with computed classes"):
        e.PlaceCSI(0, 3)
    assert_untouched(e, f, cursor, elig)


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
    job.task_groups.append(TaskGroup(name="plain", count=1, tasks=[Task(name="plain", cpu=300, memory_mb=128)]))
    e = engine_with(nodes, volumes, {}, job, perm, allocs=allocs)
    f = engine_with(nodes, volumes, {}, job, perm, allocs=allocs)
    cursor, elig = e.GetCursor(), e.Eligibility()
    with pytest.raises(Unsupported, match="multi-device nodes"):
        e.PlaceCSI(0, 3)
    assert_untouched(e, f, cursor, elig)


@pytest.mark.gpu
def test_group_without_csi_requests_is_place():
    nodes, perm, volumes, node_volumes = stop_cluster()
    job = two_group_job(3)
    e = engine_with(nodes, volumes, node_volumes, job, perm)
    f = engine_with(nodes, volumes, node_volumes, job, perm)
    got, want = e.PlaceCSI(1, 3), f.Place(1, 3)
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        same_record(g, w)
    assert e.GetCursor() == f.GetCursor() and e.Eligibility() == f.Eligibility()
