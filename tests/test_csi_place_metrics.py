"""pe_place_csi_metrics / pe_place_csi_maps: the count loop of a task group with
CSI requests with AllocMetric kept (k_csi_loop<true>'s trace log, the host walk
with the reference memo shadow, one batched trace against the checkpoint), the
reason texts of CSIVolumeChecker.Feasible (csi_reason.h, pe_csi_reason_text)
and the log byte's pack / unpack.

Reference for the records: `test_csi_place.Ref`, the restatement of the loop.

Reference for record k's maps: a second oracle stack with metrics on and the
same commits. Its node list is record k's consumed window minus the rows that
reach the CSI checker and fail it (the restatement `test_csi.csi_code` for the
placement's alloc index; a row that fails the job's or the group's checks never
reaches the checker, so it stays in the list and the oracle records its
constraint, as the reference does). The limit is MaxInt32, so every row is
pulled through the rank chain as the reference pulls every row of its window.
Each removed row adds FilterNode(node, reason): ClassFiltered[NodeClass] when
the node has a class, ConstraintFiltered[text], the text restated here from
feasible.go:19-26. Maps and ScoreMetaData are compared with `==` on the dicts.
"""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from nomad_amd import abi, synth
from nomad_amd.structs import (Allocation, CSINodePlugin, CSIVolume, Constraint, DeviceGroup,
                               NetworkResource, RequestedDevice, Task, TaskGroup)

from test_csi import NS, RANDOM_INDICES, RANDOM_REQS, STOP_REQS, csi_code, csi_job, engine_with, plain, random_cluster, \
    stop_cluster
from test_csi_place import (P65, P130, PARITY_CASES, PER_ALLOC_REQS, Ref, assert_after_call, assert_records,
                            assert_untouched, class_elig, job_allocs, per_alloc_cluster, same_record, shape_cluster,
                            two_group_job)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nomad_amd", "libnomadpe.so")
CSRC = os.path.join(ROOT, "nomad_amd", "csrc")

TEMPLATES = {
    abi.PE_CSI_NOT_FOUND: "missing CSI Volume %s",
    abi.PE_CSI_NO_PLUGIN: "CSI plugin %s is missing from client %s",
    abi.PE_CSI_UNHEALTHY: "CSI plugin %s is unhealthy on client %s",
    abi.PE_CSI_MAX_VOLUMES: "CSI plugin %s has the maximum number of volumes on client %s",
    abi.PE_CSI_NO_READ: "CSI volume %s is unschedulable or has exhausted its available reader claims",
    abi.PE_CSI_NO_WRITE: "CSI volume %s is unschedulable or is read-only",
    abi.PE_CSI_IN_USE: "CSI volume %s has exhausted its available writer claims",
}
NODE_REASONS = (abi.PE_CSI_NO_PLUGIN, abi.PE_CSI_UNHEALTHY, abi.PE_CSI_MAX_VOLUMES)


def template_text(reason, plugin, volume, node_id):
    return TEMPLATES[reason] % ((plugin, node_id) if reason in NODE_REASONS else (volume,))


# ---- CPU: the formatter and the log byte --------------------------------------------------

def reason_lib():
    return abi.bind_csi_reason_text(C.CDLL(LIB))


def reason_text(lib, reason, plugin, volume, node_id, cap=None):
    need = lib.pe_csi_reason_text(reason, plugin, volume, node_id, None, 0)
    if need < 0:
        return need, None
    buf = C.create_string_buffer(need if cap is None else cap)
    assert lib.pe_csi_reason_text(reason, plugin, volume, node_id, buf, len(buf)) == need
    return need, buf.value.decode()


def test_reason_text_templates_sizes_and_einval():
    lib = reason_lib()
    plugin, volume, node = "ebs-plugin", "data[3]", "8f2c0b7e-node"
    for reason in range(1, 8):
        want = template_text(reason, plugin, volume, node)
        need, got = reason_text(lib, reason, plugin.encode(), volume.encode(), node.encode())
        assert got == want and need == len(want.encode()) + 1
        # a short buffer: the bytes needed all the same, the text cut and NUL-terminated
        need2, cut = reason_text(lib, reason, plugin.encode(), volume.encode(), node.encode(), cap=10)
        assert need2 == need and cut == want[:9]
        need1, one = reason_text(lib, reason, plugin.encode(), volume.encode(), node.encode(), cap=1)
        assert need1 == need and one == ""
        # a text that fills its buffer exactly
        assert reason_text(lib, reason, plugin.encode(), volume.encode(), node.encode(), cap=need)[1] == want
    # NULL strings read as ""
    assert reason_text(lib, abi.PE_CSI_NOT_FOUND, None, None, None)[1] == "missing CSI Volume "
    assert reason_text(lib, abi.PE_CSI_NO_PLUGIN, None, None, None)[1] == "CSI plugin  is missing from client "
    # the plugin reasons do not read the volume, the others neither plugin nor node
    assert reason_text(lib, 2, b"p", b"IGNORED", b"n")[1] == "CSI plugin p is missing from client n"
    assert reason_text(lib, 7, b"IGNORED", b"v", b"IGNORED")[1] == "CSI volume v has exhausted its available writer claims"
    # a long id needs what it needs
    long_id = "x" * 3000
    assert reason_text(lib, 1, None, long_id.encode(), None) == (len("missing CSI Volume ") + 3001,
                                                               "missing CSI Volume " + long_id)
    for reason in (0, 8, 9, 255, 0xFFFFFFFF):
        assert lib.pe_csi_reason_text(reason, b"p", b"v", b"n", None, 0) == abi.PE_EINVAL
        buf = C.create_string_buffer(b"untouched", 16)
        assert lib.pe_csi_reason_text(reason, b"p", b"v", b"n", buf, 16) == abi.PE_EINVAL
        assert buf.value == b"untouched"


def log_byte(code, stop):
    """The trace log byte, restated: 0, or request << 3 | reason with bit 7 = the node was a stop."""
    c = code & 0x7F
    return (c | (0x80 if stop else 0)) if c else 0


REASON_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "csi_reason.h"
// the log byte over every (request < 16, reason 0..7, stop), then every reason's text through
// buffers of every size up to the bytes needed plus two, each allocated at its exact size
int main() {
    for (unsigned q = 0; q < 16; q++)
        for (unsigned reason = 0; reason < 8; reason++)
            for (int stop = 0; stop < 2; stop++) {
                const unsigned code = reason ? (q << 3 | reason) : 0u;
                const uint8_t b = pe::csi_log_pack(code, stop != 0);
                std::printf("%u %u %d %u %u %u %d\n", q, reason, stop, (unsigned)b, pe::csi_log_request(b),
                            pe::csi_log_reason(b), (int)pe::csi_log_stop(b));
            }
    const char* plugin = "ebs-plugin";
    const char* volume = "data[3]";
    const char* node = "8f2c0b7e-node";
    for (unsigned reason = 0; reason <= 8; reason++) {
        const long long need = pe::csi_reason_text(reason, plugin, volume, node, nullptr, 0);
        std::printf("need %u %lld\n", reason, need);
        if (need < 0) continue;
        for (size_t cap = 1; cap <= (size_t)need + 2; cap++) {
            std::vector<char> buf(cap, 'x');
            if (pe::csi_reason_text(reason, plugin, volume, node, buf.data(), cap) != need) return 3;
            if (std::strlen(buf.data()) != (cap < (size_t)need ? cap - 1 : (size_t)need - 1)) return 4;
            if (cap >= (size_t)need) std::printf("text %u %s\n", reason, buf.data());
        }
        if (pe::csi_reason_text(reason, nullptr, nullptr, nullptr, nullptr, 0) <= 0) return 5;
    }
    return 0;
}
"""


def reason_main_lines(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "reason_main.cpp"
    src.write_text(REASON_MAIN)
    exe = tmp_path / "reason_main"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", *flags, "-I", CSRC, "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    assert b"runtime error" not in out.stderr and b"AddressSanitizer" not in out.stderr
    return out.stdout.decode().split("\n")[:-1]


def test_log_byte_pack_unpack_every_combination(tmp_path):
    """csi_reason.h's pack / unpack (the lines the kernel and the host both run)
    against the restatement, over every request < 16, reason and stop bit."""
    lines = reason_main_lines(tmp_path, sanitize=False)
    rows = [tuple(int(x) for x in ln.split()) for ln in lines if ln[0].isdigit()]
    assert len(rows) == 16 * 8 * 2
    seen = set()
    for q, reason, stop, b, uq, ur, us in rows:
        code = (q << 3 | reason) if reason else 0
        assert b == log_byte(code, bool(stop)) and 0 <= b < 256
        if reason:
            assert (uq, ur, us) == (q, reason, stop) and b != 0
            assert b not in seen          # the byte names its (request, reason, stop)
            seen.add(b)
        else:
            assert b == 0 and (uq, ur, us) == (0, 0, 0)
    assert len(seen) == 16 * 7 * 2


def test_reason_header_under_sanitizers(tmp_path):
    """csi_reason.h and a small main of its own, built with AddressSanitizer and
    UBSan as a stand-alone host program: every buffer size at its exact allocation."""
    lines = reason_main_lines(tmp_path, sanitize=True)
    texts = [ln.split(" ", 2) for ln in lines if ln.startswith("text ")]
    needs = {int(ln.split()[1]): int(ln.split()[2]) for ln in lines if ln.startswith("need ")}
    assert needs[0] == -1 and needs[8] == -1
    for reason in range(1, 8):
        want = template_text(reason, "ebs-plugin", "data[3]", "8f2c0b7e-node")
        assert needs[reason] == len(want) + 1
        assert [t[2] for t in texts if int(t[1]) == reason] == [want] * 3      # cap = need, need + 1, need + 2


# ---- the cases ------------------------------------------------------------------------------

class NeverKnown(dict):
    """Ref's memo for a group that escapes its class: no entry, so never a stop."""

    def __setitem__(self, k, v):
        pass


class Case:
    def __init__(self, name, nodes, perm, volumes, node_volumes, job, allocs=(), count=4, cursor=0, memo=True,
                 alloc_idx=None, job_fail=(), escaped_tg=False, ref_elig=True):
        self.name, self.nodes, self.perm, self.volumes, self.node_volumes = name, nodes, list(perm), volumes, node_volumes
        self.job, self.allocs, self.count, self.cursor, self.memo = job, list(allocs), count, cursor, memo
        self.alloc_idx, self.job_fail, self.escaped_tg, self.ref_elig = alloc_idx, set(job_fail), escaped_tg, ref_elig
        self._codes = {}

    def codes(self, i):
        """row -> availability code for placement i's alloc index (failing rows only)."""
        idx = self.alloc_idx[i] if self.alloc_idx else 0
        if idx not in self._codes:
            reqs = self.job.task_groups[0].csi_volumes
            self._codes[idx] = {r: c for r, nd in enumerate(self.nodes)
                                for c in [csi_code(nd, reqs, "[%d]" % idx, self.volumes, self.node_volumes, NS, self.job.id)]
                                if c}
        return self._codes[idx]

    def text(self, i, row):
        code = self.codes(i)[row]
        q, reason = code >> 3, code & 7
        r = self.job.task_groups[0].csi_volumes[q]
        idx = self.alloc_idx[i] if self.alloc_idx else 0
        src = r.source + ("[%d]" % idx if r.per_alloc else "")
        vol = {(v.namespace, v.id): v for v in self.volumes}.get((NS, src))
        return template_text(reason, vol.plugin_id if vol else None, src, self.nodes[row].id)

    def engine(self, metrics):
        e = engine_with(self.nodes, self.volumes, self.node_volumes, self.job, self.perm, allocs=self.allocs)
        e.CSICheck(0)              # the group's own column is up to date: the launches counted are the call's
        if metrics:
            e.EnableMetrics(True)
        if self.memo:
            e.PutEligibility(class_elig(self.nodes))
        if self.cursor:
            e.SetCursor(self.cursor, e.limit)
        return e


def mixed_node_class(nodes):
    """No NodeClass on every third node (a computed class of its own)."""
    for r, nd in enumerate(nodes):
        if r % 3 == 0:
            nd.node_class = ""
            nd.compute_class()
    return nodes


def parity_case(k):
    P, U = PARITY_CASES[k]
    nodes, perm, volumes, node_volumes = stop_cluster(unavailable=U)
    mixed_node_class(nodes)
    job = two_group_job(4)
    return Case("parity%d" % k, nodes, perm, volumes, node_volumes, job, job_allocs(nodes, perm, job, P))


SHAPES = [
    (1, (), 3, 0, (), True),
    (1, (0,), 2, 0, (), True),
    (2, (1,), 4, 0, (), True),
    (2, (), 5, 1, (0,), True),
    (63, (1, 62), 6, 0, (3, 4), True),
    (65, (1, 63, 64), 6, 60, (61, 62, 2), True),
    (65, (32, 35), 40, 0, P65, True),               # more than twice round a 65-node ring
    (130, (63, 64, 129), 40, 0, P130, True),        # stops at lanes 63 and 0 of a chunk and at the last position
    (130, (128,), 6, 127, (127, 129, 0, 1), True),  # the cursor three before the end of the list
    (65, tuple(range(65)), 2, 0, (), True),         # every node unavailable, memoised: a stop at once
    (65, tuple(range(65)), 2, 0, (), False),        # the same, not memoised: a skip, then a stop
]


def shape_case(k):
    n, U, count, cursor, P, memo = SHAPES[k]
    nodes, perm, volumes, node_volumes, _ = shape_cluster(n, U)
    job = csi_job(STOP_REQS, count=4, extra_group=True)
    return Case("shape%d" % k, nodes, perm, volumes, node_volumes, job, job_allocs(nodes, perm, job, P), count=count,
                cursor=cursor, memo=memo)


def per_alloc_case():
    """Indices whose records fail for different reasons: vol[1] lacks its plugin on
    the odd positions, vol[2] does not exist (the loop ends there)."""
    nodes, perm, volumes, node_volumes = per_alloc_cluster()
    job = csi_job(PER_ALLOC_REQS, count=5, extra_group=True)
    return Case("per_alloc", nodes, perm, volumes, node_volumes, job, job_allocs(nodes, perm, job, (1, 4)), count=5,
                alloc_idx=[0, 1, 3, 1, 2])


def escaped_case():
    """test_escaped_job_node_before_the_deciding_position's job: position 0 fails
    the job's escaped constraint and lacks the plugin; its key is the constraint's."""
    U = (0, 1, 5)
    nodes, perm, volumes, node_volumes = stop_cluster(unavailable=U)
    job = csi_job(STOP_REQS, count=4, extra_group=True,
                  constraints=[Constraint("${node.unique.id}", nodes[perm[0]].id, "!=")])
    return Case("escaped", nodes, perm, volumes, node_volumes, job, job_allocs(nodes, perm, job, (2, 3)), count=3,
                memo=False, job_fail={perm[0]})


def full_nodes_case():
    """Foreign allocs fill the CPU of some nodes and the bandwidth of others; the
    task asks for 100 MBits: DimensionExhausted 'cpu' and 'network: bandwidth exceeded'."""
    U = (7, 16)
    nodes, perm, volumes, node_volumes = stop_cluster(unavailable=U)
    mixed_node_class(nodes)
    job = two_group_job(5)
    job.task_groups[0].tasks[0].network = NetworkResource(mbits=100, dynamic_ports=1)
    allocs = [Allocation(nodes[perm[p]].id, "other-job", "cache", cpu_shares=3700, memory_mb=256) for p in (1, 4, 11)]
    allocs += [Allocation(nodes[perm[p]].id, "other-job", "cache", cpu_shares=100, memory_mb=64, net_mbits=950)
               for p in (3, 6, 13)]
    return Case("full_nodes", nodes, perm, volumes, node_volumes, job, allocs, count=5)


def device_case():
    """One healthy GPU on the nodes at even rows (a computed class of their own;
    the others fail DeviceChecker), some already held: 'devices: no devices match request'."""
    U = (20, 33)
    nodes, perm, volumes, node_volumes = stop_cluster(unavailable=U)
    for r, nd in enumerate(nodes):
        if r % 2 == 0:
            nd.devices = [DeviceGroup("nvidia", "gpu", "1080ti", healthy=1)]
            nd.compute_class()
    job = two_group_job(5)
    job.task_groups[0].tasks[0].devices = [RequestedDevice("nvidia/gpu", count=1)]
    held = [perm[p] for p in range(12) if perm[p] % 2 == 0][:2]
    allocs = [Allocation(nodes[r].id, "other-job", "cache", cpu_shares=100, memory_mb=64, devices=[(0, 1)]) for r in held]
    return Case("device", nodes, perm, volumes, node_volumes, job, allocs, count=5, memo=False,
                job_fail={r for r in range(len(nodes)) if r % 2}, ref_elig=False)


def random_case(n, idx):
    """test_csi.random_cluster with a group that escapes its class (never a stop),
    so a Select walks past every unavailable node: all seven reasons."""
    nodes, volumes, node_volumes, job_id = random_cluster(n, seed=100 + n)
    perm = [int(x) for x in synth.shuffle(n, 7 + n)]
    job = csi_job(RANDOM_REQS, count=3, job_id=job_id, extra_group=True)
    job.task_groups[0].constraints = [Constraint("${node.unique.id}", "no-such-node", "!=")]
    return Case("random%d_%d" % (n, idx), nodes, perm, volumes, node_volumes, job, count=3, memo=False,
                alloc_idx=[idx, 5, idx], escaped_tg=True, ref_elig=False)


RANDOM_PARAMS = [(n, idx) for n in (63, 130) for idx in RANDOM_INDICES]
BUILDERS = {}
for _k in range(len(PARITY_CASES)):
    BUILDERS["parity%d" % _k] = (parity_case, _k)
for _k in range(len(SHAPES)):
    BUILDERS["shape%d" % _k] = (shape_case, _k)
for _n, _i in RANDOM_PARAMS:
    BUILDERS["random%d_%d" % (_n, _i)] = (random_case, _n, _i)
BUILDERS.update(per_alloc=(per_alloc_case,), escaped=(escaped_case,), full_nodes=(full_nodes_case,),
                device=(device_case,))
_REFS = {}


def passes_checks(probe, cache, row):
    """Whether the node passes the job's and the group's checks: a Select over it
    alone on a stack without allocs filters it or not."""
    if row not in cache:
        probe.SetNodes([row])
        cache[row] = probe.SelectRaw(0).nodes_filtered == 0
    return cache[row]


def reference(name):
    """(case, Ref, want records, want maps), computed once per case."""
    if name in _REFS:
        return _REFS[name]
    from oracle.oracle import OracleGenericStack
    b = BUILDERS[name]
    case = b[0](*b[1:])
    sizing = OracleGenericStack()
    sizing.SetState(case.nodes, [])
    sizing.SetJob(plain(case.job))
    sizing.SetNodes(case.perm)
    limit = sizing.limit
    classes = {nd.computed_class for nd in case.nodes}
    known = {c: True for c in classes} if case.memo else {}
    ref = Ref(case.nodes, case.perm, case.job, case.allocs, limit, cursor=case.cursor, known=known,
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
    probe, reaches = sizing, {}
    n, cur, maps = len(case.perm), case.cursor, []
    for k, w in enumerate(want):
        window = [case.perm[(cur + j) % n] for j in range(w["nodes_evaluated"])]
        failing = case.codes(k)
        removed = [r for r in window if r in failing and r not in case.job_fail and passes_checks(probe, reaches, r)]
        o.SetNodes([r for r in window if r not in removed])
        o.SetCursor(0, 0x7FFFFFFF)
        o.SelectRaw(0)
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


def csi_keys(maps):
    return {k for m in maps for k in m["ConstraintFiltered"] if k.startswith(("CSI ", "missing CSI "))}


# ---- CPU: the inputs reach every case the GPU tests rely on -------------------------------------

def test_reference_reaches_every_case():
    reasons, evicts, tie, exhausted, popped, final_nil, dims = set(), False, False, False, False, False, set()
    classed, unclassed = False, False
    for name in BUILDERS:
        case, ref, want, maps = reference(name)
        assert len(maps) == len(want)
        for k, (w, m) in enumerate(zip(want, maps)):
            for r, code in case.codes(k).items():
                if case.text(k, r) in m["ConstraintFiltered"]:
                    reasons.add(code & 7)
                    classed = classed or bool(case.nodes[r].node_class)
                    unclassed = unclassed or not case.nodes[r].node_class
            options = w["nodes_evaluated"] - w["nodes_filtered"] - w["nodes_exhausted"]
            evicts = evicts or (options > 5 and len(m["ScoreMetaData"]) == 5)
            norms = [x[1] for x in m["ScoreMetaData"]]
            tie = tie or len(set(norms)) < len(norms)
            exhausted = exhausted or w["nodes_exhausted"] > 0
            dims |= set(m["DimensionExhausted"])
            assert sum(m["DimensionExhausted"].values()) == w["nodes_exhausted"]
        popped = popped or any('pop' in t for t in ref.traces)
        final_nil = final_nil or want[-1]["row"] < 0
    assert reasons == {1, 2, 3, 4, 5, 6, 7}
    assert evicts and tie and exhausted and popped and final_nil and classed and unclassed
    assert {"cpu", "network: bandwidth exceeded", "devices: no devices match request"} <= dims
    # the escaped job's failing row keeps the constraint's key; a record past its class's first row
    # holds the memoised text of the device case's ineligible class
    case, _, want, maps = reference("escaped")
    assert want[0]["nodes_filtered"] >= 3
    assert any(k.startswith("${node.unique.id}") for k in maps[0]["ConstraintFiltered"])
    assert len(csi_keys(maps[:1])) == 2            # positions 1 and 5; never position 0
    assert case.nodes[case.perm[0]].id not in " ".join(csi_keys(maps))
    _, _, dwant, dmaps = reference("device")
    assert sum(w["row"] >= 0 for w in dwant) >= 2 and sum(w["row"] >= 0 for w in reference("full_nodes")[2]) >= 2
    assert any("missing devices" in m["ConstraintFiltered"] for m in dmaps)
    assert any("computed class ineligible" in m["ConstraintFiltered"] for m in dmaps)
    # per_alloc: different reasons per record, the missing volume among them
    _, _, pwant, pmaps = reference("per_alloc")
    assert pwant[-1]["row"] < 0 and len(pwant) == 5
    assert "missing CSI Volume vol[2]" in pmaps[4]["ConstraintFiltered"]
    assert any(k.startswith("CSI plugin bar is missing from client") for k in csi_keys(pmaps[1:2] + pmaps[3:4]))
    assert not csi_keys(pmaps[0:1]) and not csi_keys(pmaps[2:3])


# ---- GPU: parity ------------------------------------------------------------------------------------

def run_case(name):
    case, ref, want, maps = reference(name)
    e, f = case.engine(True), case.engine(False)
    before = e.csi_avail_launches()
    got = e.PlaceCSIMetrics(0, case.count, alloc_idx=case.alloc_idx)
    launches = e.csi_avail_launches() - before
    got_maps = e.PlaceCSIMaps()
    assert_records(got, want)
    assert len(got_maps) == len(want)
    for k, (gm, wm) in enumerate(zip(got_maps, maps)):
        assert gm == wm, (name, k)
    # as after the other batched metrics calls
    from nomad_amd.stack import EngineError
    with pytest.raises(EngineError):
        e.LastMetrics()
    # ... and everything else is pe_place_csi's with metrics off
    plain_got = f.PlaceCSI(0, case.count, alloc_idx=case.alloc_idx)
    assert len(plain_got) == len(got)
    for g, p in zip(got, plain_got):
        same_record(g, p)
        assert list(g.scores) == list(p.scores)
    assert e.GetCursor() == f.GetCursor() and e.Eligibility() == f.Eligibility()
    if case.ref_elig and not case.escaped_tg:
        assert e.GetCursor() == (ref.cursor, e.limit)
        ee, re_ = e.Eligibility(), ref.eligibility()
        assert ee["tgs"] == re_["tgs"] and (case.job_fail or ee["job"] == re_["job"])
    e.SetNodes(case.perm)
    f.SetNodes(case.perm)
    same_record(e.SelectRaw(1), f.SelectRaw(1))      # the plan, through the plain group's next Select
    return case, launches, got_maps


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(PARITY_CASES)))
def test_parity_where_select_gives_up(k):
    case, _, maps = run_case("parity%d" % k)
    _, ref, want, _ = reference(case.name)
    assert_after_call_like(case, ref, want)


def assert_after_call_like(case, ref, want):
    """assert_after_call on a fresh metrics handle (cursor, Eligibility(), plan against per-row commits)."""
    e = case.engine(True)
    e.PlaceCSIMetrics(0, case.count, alloc_idx=case.alloc_idx)
    assert_after_call(e, ref, want, case.nodes, case.volumes, case.node_volumes, case.job, case.perm, case.allocs)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_shapes(k):
    case, _, maps = run_case("shape%d" % k)
    _, ref, want, _ = reference(case.name)
    if case.count == 40:
        assert len(want) == 40 and sum(w["nodes_evaluated"] for w in want) > 2 * len(case.nodes)


@pytest.mark.gpu
def test_per_alloc_reasons_differ_per_record():
    case, launches, maps = run_case("per_alloc")
    assert launches == 3                 # vol[0] and vol[3] share a column; vol[1]; vol[2]
    assert "missing CSI Volume vol[2]" in maps[4]["ConstraintFiltered"]


@pytest.mark.gpu
def test_escaped_job_rows_keep_the_constraint_key():
    case, _, maps = run_case("escaped")
    assert any(k.startswith("${node.unique.id}") for k in maps[0]["ConstraintFiltered"])
    assert case.nodes[case.perm[0]].id not in " ".join(csi_keys(maps))


@pytest.mark.gpu
def test_full_nodes_and_network_ask():
    _, _, maps = run_case("full_nodes")
    dims = {k for m in maps for k in m["DimensionExhausted"]}
    assert {"cpu", "network: bandwidth exceeded"} <= dims


@pytest.mark.gpu
def test_device_ask():
    _, _, maps = run_case("device")
    assert any("devices: no devices match request" in m["DimensionExhausted"] for m in maps)


@pytest.mark.gpu
@pytest.mark.parametrize("n,idx", RANDOM_PARAMS)
def test_random_clusters_every_reason(n, idx):
    case, launches, maps = run_case("random%d_%d" % (n, idx))
    assert launches <= 2                 # the distinct record sets of [idx, 5, idx], and no more


@pytest.mark.gpu
def test_launch_count_is_the_distinct_record_sets():
    nodes, perm, volumes, node_volumes = per_alloc_cluster()
    job = csi_job(PER_ALLOC_REQS, count=4, extra_group=True)
    allocs = job_allocs(nodes, perm, job, (1, 4))
    for idx, launches in (([0, 1, 0, 1], 2), ([0, 3, 0, 3], 1), ([1, 1, 1, 1], 1), ([0, 1, 3, 2], 3)):
        for metrics in (True, False):
            e = engine_with(nodes, volumes, node_volumes, job, perm, allocs=allocs)
            e.CSICheck(0)              # the group's own column is up to date
            e.EnableMetrics(metrics)
            e.PutEligibility(class_elig(nodes))
            before = e.csi_avail_launches()
            e.PlaceCSIMetrics(0, 4, alloc_idx=idx)
            assert e.csi_avail_launches() - before == launches, (idx, metrics)


# ---- GPU: metrics off, refusals ------------------------------------------------------------------

@pytest.mark.gpu
def test_metrics_off_is_place_csi_and_has_no_maps():
    from nomad_amd.stack import EngineError
    case, _, want, _ = reference("parity1")
    e, f = case.engine(False), case.engine(False)
    got, plain_got = e.PlaceCSIMetrics(0, case.count), f.PlaceCSI(0, case.count)
    assert_records(got, want)
    for g, p in zip(got, plain_got):
        same_record(g, p)
    assert e.GetCursor() == f.GetCursor() and e.Eligibility() == f.Eligibility()
    with pytest.raises(EngineError) as err:
        e.PlaceCSIMaps()
    assert err.value.code == abi.PE_ESTATE
    # the maps of a metrics call go with the next placing or state call
    m = case.engine(True)
    m.PlaceCSIMetrics(0, case.count)
    assert len(m.PlaceCSIMaps()) == len(want)
    m.SetNodes(case.perm)
    with pytest.raises(EngineError):
        m.PlaceCSIMaps()


@pytest.mark.gpu
def test_new_refusals_leave_the_handle_untouched():
    from nomad_amd.stack import Unsupported
    nodes, perm, volumes, node_volumes = stop_cluster()

    def pair(job):
        out = []
        for metrics in (True, False):
            e = engine_with(nodes, volumes, node_volumes, job, perm)
            e.EnableMetrics(metrics)
            out.append(e)
        return out

    def refused(job, match, count=3, tg=0, other=1):
        e, f = pair(job)
        cursor, elig = e.GetCursor(), e.Eligibility()
        with pytest.raises(Unsupported, match=match):
            if count > 64:      # refused before anything is written: no record buffer of that size
                out, placed = (abi.pe_ranked_node * 1)(), C.c_uint32(0)
                e._check(e._lib.pe_place_csi_metrics(e._h, tg, count, None, out, C.byref(placed)))
            else:
                e.PlaceCSIMetrics(tg, count)
        e.EnableMetrics(False)           # (the next Select of the plain group, on both handles alike)
        assert_untouched(e, f, cursor, elig, tg=other)
        # the metrics shadow of the memo did not move either: the call is answered afterwards
        e.EnableMetrics(True)
        return e

    job = two_group_job(3)
    # a group without CSI requests while metrics are on
    refused(job, "without CSI requests", tg=1, other=1)
    # the size cap: count * len(list) above 2^24, compared in 64 bits
    refused(job, "trace log", count=abi.PE_CSI_LOG_CAP // 64 + 1)
    refused(job, "trace log", count=(1 << 31) + 5)
    e = refused(job, "trace log", count=0xFFFFFFFF)
    got = e.PlaceCSIMetrics(0, 3)
    assert len(e.PlaceCSIMaps()) == len(got) >= 1
    # static port asks
    st = two_group_job(3)
    st.task_groups[0].network = NetworkResource(mode="host", dynamic_ports=1, reserved_ports=[8080],
                                                port_labels=["http"], host_network="default")
    refused(st, "static port")
    # reserved cores: the trace would read the cores in use after the loop's write-back
    cores = two_group_job(3)
    cores.task_groups[0].tasks[0].cores = 2
    refused(cores, "reserved cores")
    # two task groups of one name: the checkpoint holds one group's collision column
    twins = two_group_job(3)
    twins.task_groups.append(TaskGroup(name="web", count=1, tasks=[Task(name="web", cpu=300, memory_mb=128)]))
    refused(twins, "one name")
    # pe_place_csi's own list still holds with metrics on (a spread: full passes)
    from nomad_amd.structs import Spread, SpreadTarget
    spr = two_group_job(3)
    spr.task_groups[0].spreads = [Spread("${node.datacenter}", 50, [SpreadTarget("dc1", 100)])]
    refused(spr, "full passes")
    refused(job, "overlay", count=1 << 18)      # (below the log's cap for 64 nodes, beyond one launch's overlay)


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
    e.EnableMetrics(True)
    cursor, elig = e.GetCursor(), e.Eligibility()
    with pytest.raises(Unsupported, match="multi-device nodes"):
        e.PlaceCSIMetrics(0, 3)
    e.EnableMetrics(False)
    assert_untouched(e, f, cursor, elig)


@pytest.mark.gpu
def test_place_csi_and_select_still_refuse_with_metrics_on():
    from nomad_amd.stack import Unsupported
    case, _, _, _ = reference("parity0")
    e = case.engine(True)
    cursor, elig = e.GetCursor(), e.Eligibility()
    with pytest.raises(Unsupported, match="pe_set_metrics"):
        e.PlaceCSI(0, 3)
    with pytest.raises(Unsupported, match="pe_set_metrics"):
        e.SelectRaw(0)
    assert e.GetCursor() == cursor and e.Eligibility() == elig
