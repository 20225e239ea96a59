"""Destructive-update probe: what pe_place_destructive costs
against the per-call sequence it replaces.

  (default) The C2 cluster of bench.py at its default node count (10k nodes,
      seed 42), where an older version of svc-c2 already holds 600 allocs on
      distinct random nodes; all 600 are updated, in shuffled order. Two
      handles of one build and one type (GenericStack, metrics off):
        call      pe_place_destructive(tg, allocs, 600)
        sequence  per update pe_plan_stop(&alloc, 1), pe_select(tg, NULL), then
                  pe_commit, or pe_plan_pop_update and a break
      Every repetition starts from pe_reset_plan, pe_set_job and pe_set_nodes
      followed by pe_flush (not timed), so both timed sections begin on an idle
      device; both end with pe_flush (queued device work) and a device
      synchronise (the call's own synchronisation has already drained its
      stream). Three warm-up pairs, then the two versions alternate in one
      process, the order swapping every pair. The host clock runs around the ctypes calls alone; the sequence's
      arguments are built before it starts. The records are compared. The
      call's own counters (pe_place_destructive_stats) give its launches,
      synchronisations and uploads.

          python tools/destructive_probe.py [--pairs 8] [--small] [--out profiles/place_destructive/probe.json]

  --metrics  The same comparison with pe_set_metrics on in both handles
      (DESIGN.md §47): the call is pe_place_destructive_metrics followed by
      pe_place_destructive_maps; the sequence reads pe_last_metrics_bin after
      each pe_select, as a caller that keeps AllocMetric does. With
      PE_METRICS_PROF set in the environment the call's host split (walk,
      trace, maps) is read back from the engine's stderr lines.

          PE_METRICS_PROF=1 python tools/destructive_probe.py --metrics [--out profiles/place_destructive_metrics/probe.json]

  --full  The same comparison for a group that runs full passes (DESIGN.md
      §48): the C3 cluster (10k nodes, seed 7) and job_c3 (a node affinity and
      a datacenter target spread), where an older version of svc-c3 holds 600
      allocs on distinct random nodes, all 600 updated. The call is
      pe_place_destructive_full; the sequence is the same per-call sequence.

          python tools/destructive_probe.py --full [--out profiles/place_destructive_full/probe.json]

  --full-metrics  --full's shape and protocol with pe_set_metrics on in both
      handles: the call is pe_place_destructive_full_metrics
      followed by pe_place_destructive_maps, the sequence reads
      pe_last_metrics_bin after each pe_select; both legs copy the maps' bytes
      out, and records and maps are compared in every pair (the maps after the
      clock has stopped). A third handle with metrics off runs
      pe_place_destructive_full once per pair, from an idle device as well: what
      keeping the maps costs. With PE_METRICS_PROF set the call's host split
      is read back from the engine's stderr lines, with the records walked on
      the host, the traced entries and k_trace_top's path.

          PE_METRICS_PROF=1 python tools/destructive_probe.py --full-metrics [--out profiles/place_destructive_full_metrics/probe.json]

  --headline PARENT_LIB  `bench.py --gpus 1 --steps N --warmup 20` in fresh
      processes, the parent commit's library (PE_ENGINE_LIB) and this tree's
      alternating, the order swapping every leg.

          python tools/destructive_probe.py --headline /path/to/parent/libnomadpe.so [--legs 6] [--steps 40000]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nomad_amd import abi, synth  # noqa: E402
from nomad_amd.structs import Allocation  # noqa: E402


def shape(n, own, seed=42):
    """bench.py's cluster_c2 where an older version of svc-c2 holds `own` allocs on distinct nodes."""
    nodes, allocs = synth.cluster_c2(n, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    for k in rng.choice(n, size=own, replace=False):
        allocs.append(Allocation(node_id=nodes[int(k)].id, job_id="svc-c2", task_group="web",
                                 cpu_shares=500, memory_mb=256, disk_mb=150, priority=50))
    job = synth.job_c2(own)
    job.version = 7
    own_idx = [i for i, a in enumerate(allocs) if a.job_id == "svc-c2"]
    upd = [own_idx[int(k)] for k in rng.permutation(len(own_idx))]
    return nodes, allocs, job, upd


def shape_full(n, own, seed=7):
    """cluster_c3 and job_c3 where an older version of svc-c3 holds `own` allocs on distinct nodes."""
    nodes, allocs = synth.cluster_c3(n, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    for k in rng.choice(n, size=own, replace=False):
        allocs.append(Allocation(node_id=nodes[int(k)].id, job_id="svc-c3", task_group="web",
                                 cpu_shares=250, memory_mb=128, disk_mb=150, priority=50))
    job = synth.job_c3(own)
    job.version = 7
    own_idx = [i for i, a in enumerate(allocs) if a.job_id == "svc-c3"]
    upd = [own_idx[int(k)] for k in rng.permutation(len(own_idx))]
    return nodes, allocs, job, upd


def hip_runtime():
    """The HIP runtime the engine library is linked against (the process holds one copy)."""
    for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            hip = C.CDLL(name)
        except OSError:
            continue
        hip.hipDeviceSynchronize.restype = C.c_int
        hip.hipDeviceSynchronize.argtypes = []
        return hip
    raise RuntimeError("libamdhip64.so not found")


def rec_key(r):
    return (r.row, r.final_score, r.nodes_evaluated, r.nodes_filtered, r.nodes_exhausted, r.new_offset)


def call_vs_sequence(args):
    from nomad_amd.stack import GenericStack
    n, own = (2000, 200) if args.small else (10000, 600)
    nodes, allocs, job, upd = shape_full(n, own) if args.full else shape(n, own)
    perm = synth.shuffle(n, 7)

    def handle():
        st = GenericStack()
        st.SetState(nodes, allocs)
        st.SetJob(job)
        if args.metrics:
            st.EnableMetrics(True)
        return st
    a, b = handle(), handle()
    fm = args.full_metrics
    plain = None
    if fm:   # the third handle: metrics off
        plain = GenericStack()
        plain.SetState(nodes, allocs)
        plain.SetJob(job)
        plain_recs = (abi.pe_ranked_node * len(upd))()
    lib = a._lib
    lib.pe_flush.restype = C.c_int
    lib.pe_flush.argtypes = [C.c_void_p]
    length = len(upd)
    arr = np.ascontiguousarray(np.asarray(upd, dtype=np.uint32))
    recs = (abi.pe_ranked_node * length)()
    placed = C.c_uint32(0)
    one = [(C.c_uint32 * 1)(int(x)) for x in upd]
    seq = (abi.pe_ranked_node * length)()

    hip = hip_runtime()

    def settle(st):
        return lib.pe_flush(st._h) or hip.hipDeviceSynchronize()

    def prepare(st):
        st.ResetPlan()
        st.SetJob(job)
        if args.metrics and st is not plain:
            st.EnableMetrics(True)
        st.SetNodes(perm)
        assert settle(st) == 0

    place = lib.pe_place_destructive_metrics if args.metrics else lib.pe_place_destructive
    if args.full:
        place = lib.pe_place_destructive_full_metrics if fm else lib.pe_place_destructive_full
    mc, ms = C.POINTER(abi.pe_metric_count)(), C.POINTER(abi.pe_metric_score)()
    mco, mso, mn = abi.u32p(), abi.u32p(), C.c_uint32(0)
    lib.pe_last_metrics_bin.restype = C.c_int
    lib.pe_last_metrics_bin.argtypes = [C.c_void_p, C.POINTER(C.POINTER(abi.pe_metric_count)), abi.u32p,
                                        C.POINTER(C.POINTER(abi.pe_metric_score)), abi.u32p]
    nc, ns = C.c_uint32(0), C.c_uint32(0)
    map_sizes = {}
    csz, ssz = C.sizeof(abi.pe_metric_count), C.sizeof(abi.pe_metric_score)
    kept = {"call": None, "sequence": []}     # --full-metrics: the maps' bytes, copied out inside the timed sections

    def run_call():
        prepare(a)
        t0 = time.perf_counter()
        rc = place(a._h, 0, arr.ctypes.data_as(abi.u32p), length, recs, C.byref(placed))
        if args.metrics:
            rc = rc or lib.pe_place_destructive_maps(a._h, C.byref(mc), C.byref(mco), C.byref(ms), C.byref(mso),
                                                     C.byref(mn))
        if fm and rc == 0:
            k = mn.value
            kept["call"] = (k, [mco[i] for i in range(k + 1)], [mso[i] for i in range(k + 1)],
                            C.string_at(mc, csz * mco[k]), C.string_at(ms, ssz * mso[k]))
        rc = rc or settle(a)
        t1 = time.perf_counter()
        assert rc == 0, rc
        if args.metrics:
            map_sizes["call"] = (int(mn.value), int(mco[mn.value]), int(mso[mn.value]))
        return (t1 - t0) * 1e6

    def run_sequence():
        prepare(b)
        done = 0
        sizes = [0, 0]
        map_sizes["sequence"] = sizes
        kept["sequence"] = []
        t0 = time.perf_counter()
        for k in range(length):
            rc = lib.pe_plan_stop(b._h, one[k], 1) or lib.pe_select(b._h, 0, None, C.byref(seq[k]))
            if args.metrics:
                rc = rc or lib.pe_last_metrics_bin(b._h, C.byref(mc), C.byref(nc), C.byref(ms), C.byref(ns))
                sizes[0] += nc.value
                sizes[1] += ns.value
                if fm and rc == 0:
                    kept["sequence"].append((C.string_at(mc, csz * nc.value), C.string_at(ms, ssz * ns.value)))
            assert rc == 0, rc
            done = k + 1
            if seq[k].row < 0:
                lib.pe_plan_pop_update(b._h, int(upd[k]))
                break
            rc = lib.pe_commit(b._h, 0, seq[k].row)
            assert rc == 0, rc
        rc = settle(b)
        t1 = time.perf_counter()
        assert rc == 0, rc
        return (t1 - t0) * 1e6, done

    def run_plain():
        prepare(plain)
        t0 = time.perf_counter()
        rc = lib.pe_place_destructive_full(plain._h, 0, arr.ctypes.data_as(abi.u32p), length, plain_recs,
                                           C.byref(placed_plain))
        rc = rc or settle(plain)
        t1 = time.perf_counter()
        assert rc == 0, rc
        return (t1 - t0) * 1e6

    placed_plain = C.c_uint32(0)
    cdt, sdt = np.dtype(abi.pe_metric_count), np.dtype(abi.pe_metric_score)

    def maps_equal():
        """Record by record: the counts as (kind, key text, count) sets, the score items field by field."""
        k, co, so, cb, sb = kept["call"]
        if k != len(kept["sequence"]):
            return False
        cc, cs = np.frombuffer(cb, dtype=cdt), np.frombuffer(sb, dtype=sdt)
        for r in range(k):
            qb, tb = kept["sequence"][r]
            qc, qs = np.frombuffer(qb, dtype=cdt), np.frombuffer(tb, dtype=sdt)
            mine, theirs = cc[co[r]:co[r + 1]], cs[so[r]:so[r + 1]]
            if len(mine) != len(qc) or len(theirs) != len(qs):
                return False
            if sorted((int(e["kind"]), a.MetricString(int(e["key"])), int(e["count"])) for e in mine) != \
                    sorted((int(e["kind"]), b.MetricString(int(e["key"])), int(e["count"])) for e in qc):
                return False
            for x, y in zip(theirs, qs):
                n_sc = int(x["n_scores"])
                if (int(x["row"]), n_sc, float(x["norm"])) != (int(y["row"]), int(y["n_scores"]), float(y["norm"])) or \
                        list(x["scorer"][:n_sc]) != list(y["scorer"][:n_sc]) or \
                        list(x["score"][:n_sc]) != list(y["score"][:n_sc]):
                    return False
        return True

    pairs, same, counters = [], True, set()
    maps_same = True if fm else None
    # PE_METRICS_PROF: the engine writes the call's host split to stderr; keep the process's stderr in a file
    prof = args.metrics and bool(os.environ.get("PE_METRICS_PROF"))
    saved_err = None
    if prof:
        sys.stderr.flush()
        err_file = tempfile.TemporaryFile(mode="w+b")
        saved_err = os.dup(2)
        os.dup2(err_file.fileno(), 2)
    for r in range(args.pairs + 3):
        order = ("call", "sequence") if r % 2 == 0 else ("sequence", "call")
        t = {}
        for who in order:
            if who == "call":
                t["call"] = run_call()
                counters.add(a.place_destructive_stats())
            else:
                t["sequence"], done = run_sequence()
        got = min(length, placed.value + 1)
        same = same and got == done and all(rec_key(recs[k]) == rec_key(seq[k]) for k in range(got))
        if fm:
            maps_same = maps_same and maps_equal()
            t["plain"] = run_plain()
            same = same and placed_plain.value == placed.value and \
                all(rec_key(recs[k]) == rec_key(plain_recs[k]) for k in range(got))
        if r >= 3:
            pairs.append({"pair": r - 2, "order": order[0] + " first", "call_us": t["call"], "sequence_us": t["sequence"],
                          "difference_us": t["sequence"] - t["call"]})
            if fm:
                pairs[-1]["metrics_off_call_us"] = t["plain"]
    split = None
    if prof:
        C.CDLL(None).fflush(None)
        os.dup2(saved_err, 2)
        os.close(saved_err)
        err_file.seek(0)
        lines = [ln for ln in err_file.read().decode(errors="replace").splitlines()
                 if ln.startswith("place_destructive_full_metrics:" if fm else "place_destructive_metrics:")]
        rows = [[float(x) for x in re.search(r"walk ([\d.]+) us, trace ([\d.]+) us, maps ([\d.]+) us", ln).groups()]
                for ln in lines][3:]                           # (the warm-ups' lines dropped)
        if rows:
            arr3 = np.asarray(rows)
            split = {"calls": len(rows), "line": lines[-1],
                     "median_us": dict(zip(("walk", "trace", "maps"), (float(x) for x in np.median(arr3, axis=0)))),
                     "min_us": dict(zip(("walk", "trace", "maps"), (float(x) for x in arr3.min(axis=0)))),
                     "max_us": dict(zip(("walk", "trace", "maps"), (float(x) for x in arr3.max(axis=0))))}
    diff = np.asarray([p["difference_us"] for p in pairs])
    call = np.asarray([p["call_us"] for p in pairs])
    sequ = np.asarray([p["sequence_us"] for p in pairs])
    extra = {}
    if args.metrics:
        same = same and map_sizes["call"][1:] == tuple(map_sizes["sequence"])
        extra = {"metrics": True, "call_records_counts_scores": list(map_sizes["call"]),
                 "sequence_counts_scores": list(map_sizes["sequence"]),
                 "call_host_split_PE_METRICS_PROF": split}
    if fm:
        off = np.asarray([p["metrics_off_call_us"] for p in pairs])
        extra["maps_equal"] = bool(maps_same)
        extra["metrics_off_call_us"] = {"min": float(off.min()), "median": float(np.median(off)), "max": float(off.max())}
        extra["factor_between_medians"] = float(np.median(sequ) / np.median(call))
        extra["call_below_sequence_in_every_pair_and_range"] = bool(call.max() < sequ.min())
    if args.full:
        opts = [r.nodes_evaluated - r.nodes_filtered - r.nodes_exhausted for r in recs[:min(length, placed.value + 1)]]
        extra["full"] = True
        extra["options_per_select"] = {"min": int(min(opts)), "max": int(max(opts))}
    return {"tool": "tools/destructive_probe.py" + (" --full-metrics" if fm else (" --metrics" if args.metrics else "") +
                                                    (" --full" if args.full else "")), "nodes": n,
            "updates": length, "placed": int(placed.value), **extra,
            "records_equal": bool(same),
            "call_us": {"min": float(call.min()), "median": float(np.median(call)), "max": float(call.max())},
            "sequence_us": {"min": float(sequ.min()), "median": float(np.median(sequ)), "max": float(sequ.max())},
            "median_paired_difference_us": float(np.median(diff)),
            "paired_difference_range_us": [float(diff.min()), float(diff.max())],
            "ranges_overlap": bool(call.max() >= sequ.min()),
            "call_launches_synchronisations_uploads": sorted(counters),
            "pairs": pairs}


def run_json(cmd, lib):
    env = dict(os.environ)
    if lib:
        env["PE_ENGINE_LIB"] = lib
    else:
        env.pop("PE_ENGINE_LIB", None)
    out = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, check=True, timeout=900).stdout.decode()
    return json.loads([line for line in out.splitlines() if line.startswith("{")][-1])


def headline(args):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", "20"]
    legs = []
    for k in range(args.legs):
        order = ("parent", "change") if k % 2 == 0 else ("change", "parent")
        entry = {"leg": k + 1, "order": order[0] + " first"}
        for who in order:
            res = run_json(cmd, os.path.abspath(args.headline) if who == "parent" else None)
            entry[who] = {key: res[key] for key in ("value", "unit", "ms_per_step") if key in res}
        legs.append(entry)
    par = np.asarray([e["parent"]["value"] for e in legs]) / 1e6
    chg = np.asarray([e["change"]["value"] for e in legs]) / 1e6
    d = (chg / par - 1.0) * 100.0
    return {"tool": "tools/destructive_probe.py --headline", "what": " ".join(cmd[1:]),
            "note": "parent: the parent commit's engine build; change: this tree's; one process per leg and build",
            "summary": {"pairs": len(legs),
                        "parent_M_per_s": {"min": float(par.min()), "median": float(np.median(par)), "max": float(par.max())},
                        "change_M_per_s": {"min": float(chg.min()), "median": float(np.median(chg)), "max": float(chg.max())},
                        "change_faster_in_pairs": int((d > 0).sum()),
                        "median_paired_difference_percent": float(np.median(d)),
                        "paired_differences_percent": [float(x) for x in d]},
            "legs": legs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--legs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=40000)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--metrics", action="store_true")
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--full-metrics", action="store_true")
    ap.add_argument("--headline", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.full and args.metrics:
        ap.error("--full with metrics is --full-metrics")
    if args.full_metrics:
        args.full = args.metrics = True
    res = headline(args) if args.headline else call_vs_sequence(args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
