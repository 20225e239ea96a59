"""In-place CSI probe: what pe_inplace_update_csi costs against
the per-alloc sequence it replaces, and what the new arguments cost the
in-place calls that existed before.

  (default) The new call against the per-alloc sequence (pe_plan_stop,
      pe_set_nodes([row]), pe_csi_alloc_index, pe_select, pe_plan_pop_update
      and, on an option, pe_plan_stop + pe_commit) on two handles of one build
      with metrics off, over cluster_c2 (10k nodes) where an older version of
      the job holds allocs on nodes drawn with replacement. Three requests,
      one of them per_alloc; each node runs each of the three plugins with
      probability 0.97, healthy with probability 0.97, so about one node in
      six is unavailable. List lengths 1, 64 and 1024, alloc indices
      0 .. length - 1 (one record set: one k_csi_avail launch per call). Every
      repetition starts from pe_reset_plan and pe_set_job (not timed); the two
      handles alternate; the host clock runs around the ctypes calls alone, the
      sequence's arguments are built before it starts. Statuses are compared.

          python tools/inplace_csi_probe.py [--reps 24] [--small] [--out profiles/inplace_csi/probe.json]

  --leg  One leg of an A/B of pe_inplace_update_spread on the job without CSI
      (1000 updates), for the library PE_ENGINE_LIB names: prints one JSON line.
  --ab PARENT_LIB  Runs such legs in fresh processes, the parent commit's
      library and this tree's alternating (the order swaps every leg).
  --headline PARENT_LIB  The same for `bench.py --gpus 1 --steps 2000 --warmup 20` (--steps).

          python tools/inplace_csi_probe.py --ab /path/to/parent/libnomadpe.so [--legs 6] [--out ...]
"""
import argparse
import copy
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nomad_amd import abi, synth  # noqa: E402
from nomad_amd.structs import Allocation, CSINodePlugin, CSIVolume, CSIVolumeRequest  # noqa: E402

REQS = [CSIVolumeRequest("data"), CSIVolumeRequest("scratch", per_alloc=True), CSIVolumeRequest("conf", read_only=True)]


def shape(n, own, seed=71):
    """cluster_c2 where an older version of svc-c2 holds `own` allocs; the update list in shuffled order."""
    nodes, allocs = synth.cluster_c2(n, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    for k in rng.integers(0, n, size=own):
        allocs.append(Allocation(node_id=nodes[int(k)].id, job_id="svc-c2", task_group="web",
                                 cpu_shares=500, memory_mb=256, disk_mb=150, priority=50))
    job = synth.job_c2(own)
    job.version = 7
    job.task_groups[0].tasks[0].cpu = 900
    job.task_groups[0].tasks[0].memory_mb = 512
    own_idx = [i for i, a in enumerate(allocs) if a.job_id == "svc-c2"]
    upd = [own_idx[int(k)] for k in rng.permutation(len(own_idx))]
    return nodes, allocs, job, upd


def csi_state(nodes, n_alloc_names, seed=6):
    rng = np.random.Generator(np.random.PCG64(seed))
    volumes = [CSIVolume("data", "default", "p0"), CSIVolume("conf", "default", "p2")]
    volumes += [CSIVolume("scratch[%d]" % i, "default", "p1") for i in range(n_alloc_names)]
    node_volumes = {}
    for nd in nodes:
        for p in range(3):
            if rng.random() < 0.97:
                nd.csi_node_plugins["p%d" % p] = CSINodePlugin(bool(rng.random() < 0.97), 8)
    return volumes, node_volumes


def stats(us):
    a = np.asarray(us, dtype=np.float64)
    return {"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)),
            "p90_us": float(np.percentile(a, 90)), "reps": int(len(a))}


def call_vs_sequence(args):
    from nomad_amd.stack import GenericStack
    n = 2000 if args.small else 10000
    lengths = [1, 64, 1024]
    nodes, allocs, job, upd = shape(n, max(lengths))
    volumes, node_volumes = csi_state(nodes, max(lengths))
    csi = copy.deepcopy(job)
    csi.task_groups[0].csi_volumes = list(REQS)

    def handle():
        st = GenericStack()
        st.SetState(nodes, allocs)
        st.SetCSI(volumes, node_volumes)
        st.SetJob(csi)
        return st
    a, b = handle(), handle()
    lib = a._lib
    node_row = a.state.alloc_table.node_row
    out = {"tool": "tools/inplace_csi_probe.py", "nodes": n, "requests": 3, "results": []}
    for length in lengths:
        lst = upd[:length]
        arr = np.ascontiguousarray(np.asarray(lst, dtype=np.uint32))
        idx = np.ascontiguousarray(np.arange(length, dtype=np.uint32))
        recs = (abi.pe_ranked_node * length)()
        status = np.zeros(length, dtype=np.uint8)
        updated = C.c_uint32(0)
        # the sequence's arguments, built once
        one = [(C.c_uint32 * 1)(int(x)) for x in lst]
        row = [(C.c_uint32 * 1)(int(node_row[x])) for x in lst]
        lim = C.c_uint32(0)
        opts = abi.pe_select_options()
        rec = abi.pe_ranked_node()
        t_call, t_seq, launches, unavailable, same = [], [], [], None, True
        for r in range(args.reps + 3):
            for st in (a, b):
                st.ResetPlan()
                st.SetJob(csi)
            l0 = a.csi_avail_launches()
            t0 = time.perf_counter()
            rc = lib.pe_inplace_update_csi(a._h, 0, arr.ctypes.data_as(abi.u32p), idx.ctypes.data_as(abi.u32p), length,
                                           recs, status.ctypes.data_as(abi.u8p), C.byref(updated))
            t1 = time.perf_counter()
            assert rc == 0, rc
            seq_status = []
            t2 = time.perf_counter()
            for k in range(length):
                lib.pe_plan_stop(b._h, one[k], 1)
                lib.pe_set_nodes(b._h, row[k], 1, C.byref(lim))
                lib.pe_csi_alloc_index(b._h, 0, k)
                rc = lib.pe_select(b._h, 0, C.byref(opts), C.byref(rec))
                assert rc == 0, rc
                lib.pe_plan_pop_update(b._h, int(lst[k]))
                if rec.row >= 0:
                    lib.pe_plan_stop(b._h, one[k], 1)
                    lib.pe_commit(b._h, 0, rec.row)
                    seq_status.append(0)
                else:
                    seq_status.append(1 if rec.nodes_filtered else 2)
            t3 = time.perf_counter()
            same = same and seq_status == status.tolist()
            if r >= 3:
                t_call.append((t1 - t0) * 1e6)
                t_seq.append((t3 - t2) * 1e6)
                launches.append(a.csi_avail_launches() - l0)
        unavailable = float(np.count_nonzero(a.CSICheck(0))) / n
        out["results"].append({"list_length": length, "call": stats(t_call), "sequence": stats(t_seq),
                               "speedup_of_medians": float(np.median(t_seq) / np.median(t_call)),
                               "k_csi_avail_launches_per_call": sorted(set(launches)),
                               "status_counts": [int((status == c).sum()) for c in (0, 1, 2)],
                               "statuses_equal": bool(same), "unavailable_fraction_last_index": unavailable})
    return out


def leg(args):
    """pe_inplace_update_spread on the job without CSI, this process's library."""
    from nomad_amd import stack
    from nomad_amd.stack import GenericStack
    nodes, allocs, job, upd = shape(2000 if args.small else 10000, 1000)
    st = GenericStack()
    st.SetState(nodes, allocs)
    st.SetJob(job)
    arr = np.ascontiguousarray(np.asarray(upd, dtype=np.uint32))
    recs = (abi.pe_ranked_node * len(upd))()
    status = np.zeros(len(upd), dtype=np.uint8)
    updated = C.c_uint32(0)
    us, kernel = [], []
    for r in range(args.reps + 3):
        st.ResetPlan()
        st.SetJob(job)
        t0 = time.perf_counter()
        rc = st._lib.pe_inplace_update_spread(st._h, 0, arr.ctypes.data_as(abi.u32p), len(upd), recs,
                                              status.ctypes.data_as(abi.u8p), C.byref(updated))
        t1 = time.perf_counter()
        assert rc == 0, rc
        if r >= 3:
            us.append((t1 - t0) * 1e6)
            kernel.append(st.inplace_stage_ms()[0] * 1e3)
    res = dict(stats(us), min_us=float(min(us)), max_us=float(max(us)), k_inplace_us_median=float(np.median(kernel)),
               updates=len(upd), status_counts=[int((status == c).sum()) for c in (0, 1, 2)],
               library=os.path.relpath(stack.ENGINE_LIB, ROOT))
    print(json.dumps(res))


def run_json(cmd, lib):
    env = dict(os.environ)
    if lib:
        env["PE_ENGINE_LIB"] = lib
    else:
        env.pop("PE_ENGINE_LIB", None)
    out = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, check=True, timeout=900).stdout.decode()
    return json.loads([line for line in out.splitlines() if line.startswith("{")][-1])


def ab(args, cmd, what):
    legs = []
    for k in range(args.legs):
        order = ("parent", "change") if k % 2 == 0 else ("change", "parent")
        entry = {"leg": k + 1, "order": order[0] + " first"}
        for who in order:
            entry[who] = run_json(cmd, args.parent if who == "parent" else None)
        legs.append(entry)
    return {"tool": "tools/inplace_csi_probe.py", "what": what,
            "note": "parent: the parent commit's engine build; change: this tree's; one process per leg and build",
            "legs": legs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--legs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--ab", dest="parent", default=None)
    ap.add_argument("--headline", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    if args.headline:
        args.parent = args.headline
        res = ab(args, [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", "20"],
                 "bench.py --gpus 1 --steps %d --warmup 20" % args.steps)
        for e in res["legs"]:      # the result line's headline fields
            for who in ("parent", "change"):
                e[who] = {k: e[who][k] for k in ("value", "unit", "ms_per_step")}
    elif args.parent:
        cmd = [sys.executable, os.path.join("tools", "inplace_csi_probe.py"), "--leg", "--reps", str(args.reps)]
        res = ab(args, cmd + (["--small"] if args.small else []), "pe_inplace_update_spread, 1000 updates, no CSI")
    else:
        res = call_vs_sequence(args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
