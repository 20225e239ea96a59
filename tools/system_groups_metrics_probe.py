"""Multi-group system placement with AllocMetric on, probe:
pe_system_place_groups_metrics on a preempting system stack for a system job
with G task groups on cluster_c5(50000, busy=0.5), every max_parallel set to
0 (the shape and protocol of tools/system_groups_preempt_probe.py), timed
through the C ABI:

  (on)  one call with pe_set_metrics on, null arrays; the results are read in
        the staging (pe_system_groups_results, pe_system_groups_preempted,
        pe_system_groups_metrics)
  (off) the same call on a second handle with pe_set_metrics off

for G = 1, 2, 3: the groups gpu (500 MHz, 256 MB, two nvidia/gpu with
affinities, so that the named scores are produced), big (7200 MHz, 14000 MB)
and net (1500 MHz, 2048 MB, a task network of 50 MBits and one dynamic port).
Every repetition starts from the snapshot again (pe_reset_plan + pe_set_job +
pe_set_nodes, not timed); one warm-up; the two alternate; their statuses and
scores must agree bit for bit in every repetition. (on) minus (off) is the cost
of the maps. The kernel time is the engine's HIP events (pe_last_kernel_ms).

On a cut of the first 3000 nodes the batched call with metrics on is also
timed against what a caller with metrics on has without it: the node-major
per-Select loop (system_place_groups_metrics_by_select, Python around
pe_set_nodes / pe_select / pe_last_metrics / pe_commit_preempt), whose results
must equal the call's.

    python tools/system_groups_metrics_probe.py [--reps 9] [--small] [--out probe.json]
"""
import argparse
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from nomad_amd import abi, synth  # noqa: E402
from nomad_amd.stack import SystemStack, system_place_groups_metrics_by_select, unpack_status2  # noqa: E402
from nomad_amd.structs import (Affinity, NetworkResource, RequestedDevice, SchedulerConfig, Task,  # noqa: E402
                               TaskGroup)


def _tg(name, cpu, mem, net=None, devices=()):
    return TaskGroup(name=name, count=1, ephemeral_disk_mb=50,
                     tasks=[Task(name=name, driver="exec", cpu=cpu, memory_mb=mem, network=net,
                                 devices=list(devices))])


def job_of(G):
    aff = [Affinity("${device.attr.cuda_cores}", "6000", ">", 60)]
    job = synth.mock_system_job("sys-groups-metrics")
    job.task_groups = [_tg("gpu", 500, 256, devices=[RequestedDevice("nvidia/gpu", 2, affinities=aff)]),
                       _tg("big", 7200, 14000),
                       _tg("net", 1500, 2048, net=NetworkResource(mbits=50, dynamic_ports=1))][:G]
    return job


def call(st, G, n, metrics):
    """One pe_system_place_groups_metrics call; (status[n, G], score[n, G], call us, kernel us, failures)."""
    lib, h = st._lib, st._h
    tgs = np.arange(G, dtype=np.uint32)
    placed = C.c_uint32(0)
    t0 = time.perf_counter()
    rc = lib.pe_system_place_groups_metrics(h, tgs.ctypes.data_as(abi.u32p), G, None, None, None, C.byref(placed))
    us = (time.perf_counter() - t0) * 1e6
    st._check(rc)
    kus = st.last_kernel_ms() * 1e3
    sc, ss, cn = abi.f64p(), abi.u8p(), abi.u32p()
    rn, rg, rp = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    st._check(lib.pe_system_groups_results(h, C.byref(sc), C.byref(ss), C.byref(cn), C.byref(rn), C.byref(rg),
                                           C.byref(rp)))
    E, p = n * G, placed.value
    status = unpack_status2(np.ctypeslib.as_array(ss, shape=((E + 3) // 4,)), E)
    score = np.full(E, np.nan)
    score[status == 0] = np.ctypeslib.as_array(sc, shape=(max(p, 1),))[:p]
    maps = st.SystemGroupsMetrics(G) if metrics else None
    return status.reshape(n, G), score.reshape(n, G), us, kus, maps


def make(nodes, allocs, metrics):
    st = SystemStack(config=SchedulerConfig(preempt_system=True))
    st.SetState(nodes, allocs)
    st._lib.pe_flush.restype = C.c_int
    st._lib.pe_flush.argtypes = [C.c_void_p]
    st.EnableMetrics(metrics)
    return st


def fresh(st, job, rows):
    st.ResetPlan()
    st.SetJob(job)
    st.SetNodes(rows)
    st._check(st._lib.pe_flush(st._h))


def same(sa, ca, sb, cb):
    assert np.array_equal(sa, sb), "the statuses disagree"
    assert np.array_equal(ca.view(np.uint64)[sa == 0], cb.view(np.uint64)[sb == 0]), "the scores disagree"


def stats(x):
    return float(np.median(x)), [float(min(x)), float(max(x))]


def measure(G, nodes, allocs, reps):
    n = len(nodes)
    on, off = make(nodes, allocs, True), make(nodes, allocs, False)
    job, rows = job_of(G), synth.shuffle(n, 5)
    t = {"on": [], "off": []}
    k = {"on": [], "off": []}
    maps = None
    for rep in range(reps + 1):   # the first repetition warms both up
        out = {}
        for name, st in (("on", on), ("off", off)):
            fresh(st, job, rows)
            out[name] = call(st, G, n, name == "on")
            if rep:
                t[name].append(out[name][2])
                k[name].append(out[name][3])
        same(out["on"][0], out["on"][1], out["off"][0], out["off"][1])
        maps = out["on"][4]
        print("# G=%d: repetition %d of %d done" % (G, rep, reps), file=sys.stderr, flush=True)
    sb = out["on"][0]
    a, b = stats(t["on"]), stats(t["off"])
    ka, kb = stats(k["on"]), stats(k["off"])
    res = {"groups": G, "nodes": n, "entries": n * G, "reps": reps,
           "status_counts": [int((sb == v).sum()) for v in (0, 1, 2)],
           "first_failures": {str(g): list(v) for g, v in maps["failed"].items()},
           "named_score_entries": len(maps["scores"]),
           "metrics_on_call_us": a[0], "metrics_on_call_us_min_max": a[1],
           "metrics_off_call_us": b[0], "metrics_off_call_us_min_max": b[1],
           "ratio_on_over_off": a[0] / b[0],
           "metrics_on_kernel_us": ka[0], "metrics_on_kernel_us_min_max": ka[1],
           "metrics_off_kernel_us": kb[0], "metrics_off_kernel_us_min_max": kb[1],
           "kernel_share_of_metrics_on_call": ka[0] / a[0]}
    on.close()
    off.close()
    return res


def measure_cut(G, nodes, allocs, reps):
    """The batched call against the per-Select loop, both with metrics on."""
    n = len(nodes)
    a, b = make(nodes, allocs, True), make(nodes, allocs, True)
    job, rows = job_of(G), synth.shuffle(n, 5)
    ta, tb = [], []
    for rep in range(reps + 1):
        fresh(a, job, rows)
        sa, ca, us, _, maps = call(a, G, n, True)
        fresh(b, job, rows)
        t0 = time.perf_counter()
        rb = system_place_groups_metrics_by_select(b, list(range(G)))
        ub = (time.perf_counter() - t0) * 1e6
        same(sa, ca, rb[1], rb[0])
        assert maps["failed"] == rb[5]["failed"], "the first failures disagree"
        for key, named in maps["scores"].items():
            assert named == rb[5]["scores"][key], "the named scores disagree"
        if rep:
            ta.append(us)
            tb.append(ub)
        print("# cut G=%d: repetition %d of %d done" % (G, rep, reps), file=sys.stderr, flush=True)
    x, y = stats(ta), stats(tb)
    a.close()
    b.close()
    return {"groups": G, "nodes": n, "entries": n * G, "reps": reps,
            "batched_call_us": x[0], "batched_call_us_min_max": x[1],
            "per_select_loop_us": y[0], "per_select_loop_us_min_max": y[1],
            "ratio_loop_over_batched": y[0] / x[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="toy size (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nodes, allocs = synth.cluster_c5(3000 if args.small else 50000, seed=5, busy=0.5)
    for a in allocs:
        a.max_parallel = 0
    results, cut = [], []
    for G in (1, 2, 3):
        r = measure(G, nodes, allocs, args.reps)
        results.append(r)
        print(json.dumps(r), flush=True)
    cn = nodes[:300 if args.small else 3000]
    ids = {nd.id for nd in cn}
    ca = [a for a in allocs if a.node_id in ids]
    for G in (1, 2, 3):
        r = measure_cut(G, cn, ca, args.reps)
        cut.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/system_groups_metrics_probe.py", "small": args.small, "results": results,
                       "cut_3000": cut}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
