"""Multi-group system placement on a preempting stack, probe:
SystemScheduler.computePlacements (scheduler_system.go:283-425) with
PreemptionConfig.SystemSchedulerEnabled for a system job with G task groups on
cluster_c5(50000, busy=0.5), every max_parallel set to 0, timed two ways
through the C ABI on one handle per shape:

  (a) G sequential pe_system_place calls with null arrays (results read in the
      engine's staging through pe_system_results); each call evicts in its
      second pass
  (b) one pe_system_place_groups_preempt call with null arrays
      (pe_system_groups_results, pe_system_groups_preempted)

for G = 1, 2, 3: the groups gpu (500 MHz, 256 MB, two nvidia/gpu), big (7200
MHz, 14000 MB) and net (1500 MHz, 2048 MB, a task network of 50 MBits and one
dynamic port) in that order, job priority 100. Every repetition starts from
the snapshot again (pe_reset_plan + pe_set_job + pe_set_nodes, not timed); one
warm-up; the two paths alternate; their statuses and scores must agree in every
repetition. Host clock around the calls (each ends in a device synchronise);
the kernel time is the engine's HIP events (pe_last_kernel_ms; for (a) both
passes of each call, summed). (a) hands back no preempted lists, so there is
nothing to compare (b)'s lists with; their totals are reported. After the
timed repetitions one more (b) run with the per-kernel events on
(pe_set_kernel_split) gives the share of the device time in the eviction
walk.

(b) counts as slower than (a) at a given G only if its median lies above (a)'s
maximum in the same run.

    python tools/system_groups_preempt_probe.py [--reps 9] [--small] [--out probe.json]
"""
import argparse
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from nomad_amd import abi, synth  # noqa: E402
from nomad_amd.stack import SystemStack, unpack_status2  # noqa: E402
from nomad_amd.structs import (NetworkResource, RequestedDevice, SchedulerConfig, Task,  # noqa: E402
                               TaskGroup)


def _tg(name, cpu, mem, net=None, devices=()):
    return TaskGroup(name=name, count=1, ephemeral_disk_mb=50,
                     tasks=[Task(name=name, driver="exec", cpu=cpu, memory_mb=mem, network=net,
                                 devices=list(devices))])


def job_of(G):
    job = synth.mock_system_job("sys-groups-pre")
    job.task_groups = [_tg("gpu", 500, 256, devices=[RequestedDevice("nvidia/gpu", 2)]),
                       _tg("big", 7200, 14000),
                       _tg("net", 1500, 2048, net=NetworkResource(mbits=50, dynamic_ports=1))][:G]
    return job


def path_a(st, G, n):
    """G pe_system_place calls; returns (status[n, G], score[n, G], call us, kernel us)."""
    lib, h = st._lib, st._h
    status, score = np.empty((n, G), dtype=np.uint8), np.empty((n, G))
    sc, ss, rn, placed = abi.f64p(), abi.u8p(), C.c_uint32(0), C.c_uint32(0)
    us = kus = 0.0
    for g in range(G):
        t0 = time.perf_counter()
        rc = lib.pe_system_place(h, g, None, None, C.byref(placed))
        us += (time.perf_counter() - t0) * 1e6
        st._check(rc)
        kus += st.last_kernel_ms() * 1e3
        st._check(lib.pe_system_results(h, C.byref(sc), C.byref(ss), C.byref(rn)))
        status[:, g] = np.ctypeslib.as_array(ss, shape=(n,))
        score[:, g] = np.ctypeslib.as_array(sc, shape=(n,))
    return status, score, us, kus


def path_b(st, G, n):
    """One pe_system_place_groups_preempt call; the same shape, the placed
    count, the evicting entries and the preempted allocs."""
    lib, h = st._lib, st._h
    tgs = np.arange(G, dtype=np.uint32)
    placed = C.c_uint32(0)
    t0 = time.perf_counter()
    rc = lib.pe_system_place_groups_preempt(h, tgs.ctypes.data_as(abi.u32p), G, None, None, None, C.byref(placed))
    us = (time.perf_counter() - t0) * 1e6
    st._check(rc)
    kus = st.last_kernel_ms() * 1e3
    sc, ss, cn = abi.f64p(), abi.u8p(), abi.u32p()
    rn, rg, rp = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    st._check(lib.pe_system_groups_results(h, C.byref(sc), C.byref(ss), C.byref(cn), C.byref(rn), C.byref(rg),
                                           C.byref(rp)))
    en, of, al, ne = abi.u32p(), abi.u32p(), abi.u32p(), C.c_uint32(0)
    st._check(lib.pe_system_groups_preempted(h, C.byref(en), C.byref(of), C.byref(al), C.byref(ne)))
    n_alloc = int(of[ne.value]) if ne.value else 0
    E, p = n * G, placed.value
    status = unpack_status2(np.ctypeslib.as_array(ss, shape=((E + 3) // 4,)), E)
    score = np.full(E, np.nan)
    score[status == 0] = np.ctypeslib.as_array(sc, shape=(max(p, 1),))[:p]
    return status.reshape(n, G), score.reshape(n, G), us, kus, p, ne.value, n_alloc


def measure(G, nodes, allocs, reps):
    n = len(nodes)
    st = SystemStack(config=SchedulerConfig(preempt_system=True))
    st.SetState(nodes, allocs)
    st._lib.pe_flush.restype = C.c_int
    st._lib.pe_flush.argtypes = [C.c_void_p]
    st._lib.pe_system_results.restype = C.c_int
    st._lib.pe_system_results.argtypes = [C.c_void_p, C.POINTER(abi.f64p), C.POINTER(abi.u8p), abi.u32p]
    job = job_of(G)
    rows = synth.shuffle(n, 5)

    def fresh():
        st.ResetPlan()
        st.SetJob(job)
        st.SetNodes(rows)
        st._check(st._lib.pe_flush(st._h))

    ta, tb, ka, kb = [], [], [], []
    placed = evicting = n_alloc = 0
    for rep in range(reps + 1):   # the first repetition warms both paths up
        for path in ("a", "b"):
            fresh()
            if path == "a":
                sa, ca, us, kus = path_a(st, G, n)
            else:
                sb, cb, us, kus, placed, evicting, n_alloc = path_b(st, G, n)
            if rep:
                (ta if path == "a" else tb).append(us)
                (ka if path == "a" else kb).append(kus)
        assert np.array_equal(sa, sb), "the two paths' statuses disagree"
        assert np.array_equal(ca.view(np.uint64)[sa == 0], cb.view(np.uint64)[sb == 0]), "the scores disagree"
        print("# G=%d: repetition %d of %d done" % (G, rep, reps), file=sys.stderr, flush=True)
    # the share of the eviction walk: one more (b) run with the per-kernel events on
    st._check(st._lib.pe_set_kernel_split(st._h, 1))
    fresh()
    path_b(st, G, n)
    ms4 = (C.c_double * 4)()
    st._check(st._lib.pe_last_kernel_split(st._h, C.cast(ms4, abi.f64p)))
    split = [x * 1e3 for x in ms4][:3]
    st._check(st._lib.pe_set_kernel_split(st._h, 0))
    a, b = float(np.median(ta)), float(np.median(tb))
    res = {"groups": G, "nodes": n, "entries": n * G, "placed": int(placed), "reps": reps,
           "status_counts": [int((sb == v).sum()) for v in (0, 1, 2)],
           "evicting_entries": int(evicting), "preempted_allocs": int(n_alloc),
           "sequential_call_us": a, "sequential_call_us_min_max": [min(ta), max(ta)],
           "batched_call_us": b, "batched_call_us_min_max": [min(tb), max(tb)],
           "ratio_sequential_over_batched": a / b,
           "batched_slower": bool(b > max(ta)),
           "sequential_kernel_us": float(np.median(ka)), "sequential_kernel_us_min_max": [min(ka), max(ka)],
           "batched_kernel_us": float(np.median(kb)), "batched_kernel_us_min_max": [min(kb), max(kb)],
           "batched_split_us": {"stopping_pass": split[0], "eviction_walk": split[1], "compaction": split[2]},
           "eviction_walk_share_of_kernel_time": split[1] / sum(split) if sum(split) else 0.0}
    st.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="toy size (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nodes, allocs = synth.cluster_c5(3000 if args.small else 50000, seed=5, busy=0.5)
    for a in allocs:
        a.max_parallel = 0
    results = []
    for G in (1, 2, 3):
        r = measure(G, nodes, allocs, args.reps)
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/system_groups_preempt_probe.py", "small": args.small, "results": results}, f,
                      indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
