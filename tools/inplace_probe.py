"""In-place update probe: inplaceUpdate's loop (scheduler/util.go:692-806) on
one handle and state, timed two ways through the C ABI:

  (a) the per-call sequence: pe_plan_stop, pe_set_nodes (one row), pe_select,
      pe_plan_pop_update and, on an option, pe_plan_stop + pe_commit per alloc
  (b) pe_inplace_update, one call for the whole list

at three shapes: 1000 updates of a job_c2 service on cluster_c2(10000), an
updated system job holding one alloc on each of 100k cluster_c4 nodes, and
that system shape on a stack with preemption enabled (the reference's default
for system jobs), where (a)'s pe_select evicts and (b) is
pe_inplace_update_preempt. Every
repetition starts from the snapshot again (pe_reset_plan + pe_set_job, not
timed); the two paths alternate; both must return the same statuses before a
time is printed. Where every node is listed once (the system shape) the
updates are independent, and (a) runs the first --per-call-cap of them per
repetition (its cost per update does not depend on the list's length; a whole
pass takes minutes); its statuses are compared with that prefix of (b)'s.
Host clock around calls that end in a device synchronise; the kernel time of
(b) is the engine's HIP events (pe_last_kernel_ms).

--metrics: pe_inplace_update_metrics with AllocMetric on, on one
handle, against the same call with the maps off on a second handle of the same
build, alternating, at the same shapes: the call and its kernels (HIP events),
and the difference. Beside them the per-call sequence with the maps on over the
--per-call-cap prefix on the first handle, which is what a caller that keeps
AllocMetric runs without the call. Statuses are compared before a time is
printed.

--spread: the service shape with a target spread on
${node.class}, three paths alternating on one handle: the per-call sequence
(the only answer the other in-place calls leave such a job),
pe_inplace_update_spread with records, and pe_inplace_update on the same job
without the spread, which shows what the second stage costs; beside them the
HIP-event times of the walk and of the second stage (pe_inplace_spread_ms).

    python tools/inplace_probe.py [--reps 5] [--small] [--shapes service,system,preempt] [--metrics | --spread]
                                  [--out probe.json]
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
from nomad_amd.stack import GenericStack, SystemStack  # noqa: E402
from nomad_amd.structs import Allocation, SchedulerConfig, Spread, SpreadTarget  # noqa: E402


def service_shape(n_nodes, n_upd):
    nodes, allocs = synth.cluster_c2(n_nodes, seed=42)
    rng = np.random.Generator(np.random.PCG64(43))
    base = len(allocs)
    for k in rng.integers(0, n_nodes, size=n_upd):
        allocs.append(Allocation(node_id=nodes[int(k)].id, job_id="svc-c2", task_group="web",
                                 cpu_shares=500, memory_mb=256, disk_mb=150, priority=50))
    job = synth.job_c2(n_upd)
    job.version = 2
    job.task_groups[0].tasks[0].cpu = 600
    upd = base + rng.permutation(n_upd)
    return GenericStack(), nodes, allocs, job, upd.astype(np.uint32)


def system_shape(n_nodes, preempt=False):
    nodes, allocs = synth.cluster_c4(n_nodes, seed=11)
    base = len(allocs)
    for nd in nodes:
        allocs.append(Allocation(node_id=nd.id, job_id="mock-system-0", task_group="web", cpu_shares=500,
                                 memory_mb=256, disk_mb=300, net_mbits=50, dyn_ports=1, priority=100))
    job = synth.mock_system_job()
    job.version = 2
    job.task_groups[0].tasks[0].cpu = 600
    upd = base + np.random.Generator(np.random.PCG64(12)).permutation(n_nodes)
    # (preempting: the ~5 % pre-filled nodes' filler, priority 50 under the job's 100, is evicted)
    st = SystemStack(config=SchedulerConfig(preempt_system=True)) if preempt else SystemStack()
    return st, nodes, allocs, job, upd.astype(np.uint32)


def per_call(st, upd, node_row):
    """(a): the statuses of the per-call sequence, straight through ctypes."""
    lib, h = st._lib, st._h
    out, opts = abi.pe_ranked_node(), abi.pe_select_options()
    one, row = (C.c_uint32 * 1)(), (C.c_uint32 * 1)()
    status = np.empty(len(upd), dtype=np.uint8)
    for i, ai in enumerate(upd):
        one[0], row[0] = int(ai), int(node_row[ai])
        rc = lib.pe_plan_stop(h, one, 1) or lib.pe_set_nodes(h, row, 1, None) or \
            lib.pe_select(h, 0, C.byref(opts), C.byref(out)) or lib.pe_plan_pop_update(h, one[0])
        if rc == 0 and out.row >= 0:
            rc = lib.pe_plan_stop(h, one, 1) or lib.pe_commit(h, 0, out.row)
        st._check(rc)
        status[i] = 0 if out.row >= 0 else (1 if out.nodes_filtered else 2)
    return status


def batched(st, upd, recs, status, entry="pe_inplace_update"):
    """(b): one pe_inplace_update (or pe_inplace_update_preempt)."""
    updated = C.c_uint32(0)
    st._check(getattr(st._lib, entry)(st._h, 0, upd.ctypes.data_as(abi.u32p), len(upd), recs,
                                        status.ctypes.data_as(abi.u8p), C.byref(updated)))
    return updated.value


def measure(name, shape, reps, cap, entry="pe_inplace_update"):
    st, nodes, allocs, job, upd = shape
    st.SetState(nodes, allocs)
    st._lib.pe_flush.restype = C.c_int
    st._lib.pe_flush.argtypes = [C.c_void_p]
    node_row = np.ctypeslib.as_array(st.state.alloc_table.node_row, shape=(len(allocs),)).copy()
    n = len(upd)
    # (a) over the first `cap` updates only when no node is listed twice: the
    # updates are independent then, so the prefix costs and answers the same
    # inside the whole list, and a whole pass of (a) would take minutes
    na = n
    if cap and n > cap and len(np.unique(node_row[upd])) == n:
        na = cap
    recs = (abi.pe_ranked_node * n)()
    sb = np.empty(n, dtype=np.uint8)
    ta, tb, tk = [], [], []
    for rep in range(reps + 1):   # the first repetition warms both paths up
        for path in ("a", "b"):
            st.ResetPlan()
            st.SetJob(job)
            st._check(st._lib.pe_flush(st._h))
            t0 = time.perf_counter()
            if path == "a":
                sa = per_call(st, upd[:na], node_row)
            else:
                batched(st, upd, recs, sb, entry)
            dt = (time.perf_counter() - t0) * 1e6
            if rep:
                (ta if path == "a" else tb).append(dt)
                if path == "b":
                    tk.append(st.last_kernel_ms() * 1e3)
        assert np.array_equal(sa, sb[:na]), "the two paths disagree"
        print("# %s: repetition %d of %d done" % (name, rep, reps), file=sys.stderr, flush=True)
    a, b, k = np.median(ta) * (n / na), np.median(tb), np.median(tk)
    ta = [x * (n / na) for x in ta]   # per-update figures below divide by n
    res = {"shape": name, "entry": entry, "updates": n, "per_call_updates_timed": na, "nodes": len(nodes), "reps": reps,
           "status_counts": [int((sb == v).sum()) for v in (0, 1, 2)],
           "per_call_us_per_update": a / n, "per_call_us_min_max": [min(ta) / n, max(ta) / n],
           "batched_us_per_update": b / n, "batched_us_min_max": [min(tb) / n, max(tb) / n],
           "batched_call_us": b, "ratio_per_call_over_batched": a / b,
           "k_inplace_us": k, "k_inplace_us_min_max": [min(tk), max(tk)]}
    st.close()
    return res


def measure_metrics(name, make, reps, cap):
    """The metrics leg: the new call with the maps on (handle `on`) and off
    (handle `off`), alternating; the per-call sequence with the maps on."""
    on, nodes, allocs, job, upd = make()
    off = SystemStack(config=SchedulerConfig(preempt_system=bool(on._cfg.preempt))) \
        if isinstance(on, SystemStack) else GenericStack()
    for st in (on, off):
        st.SetState(nodes, allocs)
        st._lib.pe_flush.restype = C.c_int
        st._lib.pe_flush.argtypes = [C.c_void_p]
    on.EnableMetrics(True)
    node_row = np.ctypeslib.as_array(on.state.alloc_table.node_row, shape=(len(allocs),)).copy()
    n = len(upd)
    na = n
    if cap and n > cap and len(np.unique(node_row[upd])) == n:
        na = cap
    recs = (abi.pe_ranked_node * n)()
    s_on, s_off = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint8)
    t = {"a": [], "on": [], "off": [], "k_on": [], "k_off": []}
    n_scores = 0
    for rep in range(reps + 1):   # the first repetition warms the paths up
        for path in ("a", "on", "off"):
            st = off if path == "off" else on
            st.ResetPlan()
            st.SetJob(job)
            st._check(st._lib.pe_flush(st._h))
            t0 = time.perf_counter()
            if path == "a":
                sa = per_call(st, upd[:na], node_row)
            else:
                batched(st, upd, recs, s_on if path == "on" else s_off, "pe_inplace_update_metrics")
            dt = (time.perf_counter() - t0) * 1e6
            if rep:
                t[path].append(dt)
                if path != "a":
                    t["k_" + path].append(st.last_kernel_ms() * 1e3)
            if path == "on":
                mp, sp = C.POINTER(abi.pe_inplace_metric)(), C.POINTER(abi.pe_metric_score)()
                nm, ns = C.c_uint32(0), C.c_uint32(0)
                st._check(st._lib.pe_inplace_metrics(st._h, C.byref(mp), C.byref(nm), C.byref(sp), C.byref(ns)))
                assert nm.value == n
                n_scores = ns.value
        assert np.array_equal(s_on, s_off) and np.array_equal(sa, s_on[:na]), "the paths disagree"
        assert n_scores == int((s_on == 0).sum())
        print("# %s (metrics): repetition %d of %d done" % (name, rep, reps), file=sys.stderr, flush=True)
    med = {k: float(np.median(v)) for k, v in t.items()}
    a = med["a"] * (n / na)
    res = {"shape": name, "entry": "pe_inplace_update_metrics", "updates": n, "per_call_updates_timed": na,
           "nodes": len(nodes), "reps": reps, "status_counts": [int((s_on == v).sum()) for v in (0, 1, 2)],
           "score_items": n_scores,
           "metrics_on_call_us": med["on"], "metrics_on_call_us_min_max": [min(t["on"]), max(t["on"])],
           "metrics_off_call_us": med["off"], "metrics_off_call_us_min_max": [min(t["off"]), max(t["off"])],
           "call_us_difference": med["on"] - med["off"],
           "metrics_on_kernels_us": med["k_on"], "metrics_on_kernels_us_min_max": [min(t["k_on"]), max(t["k_on"])],
           "metrics_off_kernels_us": med["k_off"], "metrics_off_kernels_us_min_max": [min(t["k_off"]), max(t["k_off"])],
           "kernels_us_difference": med["k_on"] - med["k_off"],
           "metrics_on_us_per_update": med["on"] / n,
           "per_call_metrics_on_us_per_update": a / n,
           "per_call_metrics_on_us_min_max": [min(t["a"]) / na, max(t["a"]) / na],
           "ratio_per_call_over_call": a / med["on"]}
    on.close()
    off.close()
    return res


def measure_spread(n_nodes, n_upd, reps):
    """The spread leg: the service shape with a target spread on
    ${node.class}, three paths alternating on one handle: (a) the per-call
    sequence, (b) pe_inplace_update_spread with records, (c) pe_inplace_update
    on the same job without the spread. Statuses do not depend on the spread:
    all three must agree on every repetition."""
    st, nodes, allocs, job, upd = service_shape(n_nodes, n_upd)
    plain = copy.deepcopy(job)
    job.task_groups[0].spreads = [Spread("${node.class}", 60, [SpreadTarget("class-1", 40), SpreadTarget("class-2", 30)])]
    st.SetState(nodes, allocs)
    st._lib.pe_flush.restype = C.c_int
    st._lib.pe_flush.argtypes = [C.c_void_p]
    node_row = np.ctypeslib.as_array(st.state.alloc_table.node_row, shape=(len(allocs),)).copy()
    n = len(upd)
    recs = (abi.pe_ranked_node * n)()
    s = {"b": np.empty(n, dtype=np.uint8), "c": np.empty(n, dtype=np.uint8)}
    t = {"a": [], "b": [], "c": [], "stage1": [], "stage2": [], "k_c": []}
    with_part = 0
    for rep in range(reps + 1):   # the first repetition warms the paths up
        for path in ("a", "b", "c"):
            st.ResetPlan()
            st.SetJob(plain if path == "c" else job)
            st._check(st._lib.pe_flush(st._h))
            t0 = time.perf_counter()
            if path == "a":
                sa = per_call(st, upd, node_row)
            else:
                batched(st, upd, recs, s[path], "pe_inplace_update_spread" if path == "b" else "pe_inplace_update")
            dt = (time.perf_counter() - t0) * 1e6
            if path == "b":
                with_part = sum(1 for i in range(n) if s["b"][i] == 0 and recs[i].n_scores >= 2)
            if rep:
                t[path].append(dt)
                if path == "b":
                    ms = st.inplace_stage_ms()
                    t["stage1"].append(ms[0] * 1e3)
                    t["stage2"].append(ms[1] * 1e3)
                elif path == "c":
                    t["k_c"].append(st.last_kernel_ms() * 1e3)
        assert np.array_equal(sa, s["b"]) and np.array_equal(s["b"], s["c"]), "the paths disagree"
        print("# spread: repetition %d of %d done" % (rep, reps), file=sys.stderr, flush=True)
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {"shape": "service with a target spread: %d updates" % n, "entry": "pe_inplace_update_spread", "updates": n,
           "nodes": len(nodes), "reps": reps, "status_counts": [int((s["b"] == v).sum()) for v in (0, 1, 2)],
           "records_with_a_spread_part": with_part}
    for k, label in (("a", "per_call"), ("b", "spread_call"), ("c", "plain_call_without_spread")):
        res[label + "_us"] = med[k]
        res[label + "_us_min_max"] = [min(t[k]), max(t[k])]
        res[label + "_us_per_update"] = med[k] / n
    res["ratio_per_call_over_spread_call"] = med["a"] / med["b"]
    res["spread_call_minus_plain_call_us"] = med["b"] - med["c"]
    res["stage1_us"] = med["stage1"]
    res["stage1_us_min_max"] = [min(t["stage1"]), max(t["stage1"])]
    res["stage2_us"] = med["stage2"]
    res["stage2_us_min_max"] = [min(t["stage2"]), max(t["stage2"])]
    res["plain_call_kernel_us"] = med["k_c"]
    st.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="toy sizes (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--per-call-cap", type=int, default=2000,
                    help="updates path (a) runs per repetition when every node is listed once (0: all)")
    ap.add_argument("--shapes", default="service,system,preempt", help="comma-separated: service, system, preempt")
    ap.add_argument("--metrics", action="store_true",
                    help="the AllocMetric leg: pe_inplace_update_metrics, maps on against maps off")
    ap.add_argument("--spread", action="store_true",
                    help="the spread leg: pe_inplace_update_spread on the service shape with a target spread")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n_sys = 2000 if args.small else 100000
    shapes = {"service": ("service: %d updates" % (50 if args.small else 1000),
                          lambda: service_shape(500 if args.small else 10000, 50 if args.small else 1000),
                          "pe_inplace_update"),
              "system": ("system: one alloc per node", lambda: system_shape(n_sys), "pe_inplace_update"),
              "preempt": ("system, preemption enabled: one alloc per node", lambda: system_shape(n_sys, True),
                          "pe_inplace_update_preempt")}
    results = []
    if args.spread:
        r = measure_spread(500 if args.small else 10000, 50 if args.small else 1000, args.reps)
        results.append(r)
        print(json.dumps(r), flush=True)
    for key in ([] if args.spread else args.shapes.split(",")):
        name, make, entry = shapes[key]
        if args.metrics:
            r = measure_metrics(name, make, args.reps, args.per_call_cap)
        else:
            r = measure(name, make(), args.reps, args.per_call_cap, entry)
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/inplace_probe.py", "small": args.small, "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
