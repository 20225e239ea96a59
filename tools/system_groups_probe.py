"""Multi-group system placement probe: SystemScheduler.computePlacements
(scheduler_system.go:283-425) for a system job with G task groups on
cluster_c4, timed two ways through the C ABI on one handle per shape:

  (a) G sequential pe_system_place calls with null arrays (results read in the
      engine's staging through pe_system_results)
  (b) one pe_system_place_groups call with null arrays
      (pe_system_groups_results)

for G = 1, 2, 4. The groups are copies of mock.SystemJob's group under
different names with asks small enough that several fit on a node. Every
repetition starts from the snapshot again (pe_reset_plan + pe_set_job +
pe_set_nodes, not timed); one warm-up; the two paths alternate; their statuses
and scores must agree before a time is printed. Host clock around the calls
(each ends in a device synchronise); the kernel time is the engine's HIP
events (pe_last_kernel_ms), summed over (a)'s calls. Bytes downloaded are
counted from the layouts: (a) per call 8 n scores + n outcome bytes (padded
to 4) + 256 counter bytes; (b) the packed outcome bytes (padded to 8) + 8
bytes per placed entry by DMA and 4 (1 + 3 G) header bytes through mapped
host memory.

    python tools/system_groups_probe.py [--reps 9] [--small] [--out probe.json]
"""
import argparse
import copy
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from nomad_amd import abi, synth  # noqa: E402
from nomad_amd.stack import SystemStack, unpack_status2  # noqa: E402


def job_of(G):
    job = synth.mock_system_job()
    base = job.task_groups[0]
    base.tasks[0].cpu, base.tasks[0].memory_mb, base.ephemeral_disk_mb = 200, 128, 100
    job.task_groups = []
    for k in range(G):
        g = copy.deepcopy(base)
        g.name = "agent-%d" % k
        g.tasks[0].name = g.name
        job.task_groups.append(g)
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
    """One pe_system_place_groups call; the same shape, and the placed count."""
    lib, h = st._lib, st._h
    tgs = np.arange(G, dtype=np.uint32)
    placed = C.c_uint32(0)
    t0 = time.perf_counter()
    rc = lib.pe_system_place_groups(h, tgs.ctypes.data_as(abi.u32p), G, None, None, None, C.byref(placed))
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
    return status.reshape(n, G), score.reshape(n, G), us, kus, p


def measure(G, nodes, allocs, reps):
    n = len(nodes)
    st = SystemStack()
    st.SetState(nodes, allocs)
    st._lib.pe_flush.restype = C.c_int
    st._lib.pe_flush.argtypes = [C.c_void_p]
    st._lib.pe_system_results.restype = C.c_int
    st._lib.pe_system_results.argtypes = [C.c_void_p, C.POINTER(abi.f64p), C.POINTER(abi.u8p), abi.u32p]
    job = job_of(G)
    rows = synth.shuffle(n, 5)
    ta, tb, ka, kb = [], [], [], []
    placed = 0
    for rep in range(reps + 1):   # the first repetition warms both paths up
        for path in ("a", "b"):
            st.ResetPlan()
            st.SetJob(job)
            st.SetNodes(rows)
            st._check(st._lib.pe_flush(st._h))
            if path == "a":
                sa, ca, us, kus = path_a(st, G, n)
            else:
                sb, cb, us, kus, placed = path_b(st, G, n)
            if rep:
                (ta if path == "a" else tb).append(us)
                (ka if path == "a" else kb).append(kus)
        assert np.array_equal(sa, sb), "the two paths' statuses disagree"
        assert np.array_equal(ca.view(np.uint64)[sa == 0], cb.view(np.uint64)[sb == 0]), "the scores disagree"
        print("# G=%d: repetition %d of %d done" % (G, rep, reps), file=sys.stderr, flush=True)
    E = n * G
    a, b = float(np.median(ta)), float(np.median(tb))
    res = {"groups": G, "nodes": n, "entries": E, "placed": int(placed), "reps": reps,
           "status_counts": [int((sb == v).sum()) for v in (0, 1, 2)],
           "sequential_call_us": a, "sequential_call_us_min_max": [min(ta), max(ta)],
           "batched_call_us": b, "batched_call_us_min_max": [min(tb), max(tb)],
           "ratio_sequential_over_batched": a / b,
           "sequential_kernel_us": float(np.median(ka)), "sequential_kernel_us_min_max": [min(ka), max(ka)],
           "batched_kernel_us": float(np.median(kb)), "batched_kernel_us_min_max": [min(kb), max(kb)],
           "sequential_bytes_downloaded": G * (8 * n + ((n + 3) & ~3) + 256),
           "batched_bytes_downloaded": (((E + 3) // 4 + 7) & ~7) + 8 * int(placed) + 4 * (1 + 3 * G)}
    st.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="toy size (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nodes, allocs = synth.cluster_c4(3000 if args.small else 100000, seed=11)
    results = []
    for G in (1, 2, 4):
        r = measure(G, nodes, allocs, args.reps)
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/system_groups_probe.py", "small": args.small, "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
