"""CSI probe: what task groups with CSI volumes cost on the
device path, at 10k nodes (cluster_c2) and 100k nodes (cluster_c4) with three
requests, one of them per_alloc.

  (a) k_csi_avail alone, by the engine's HIP events (pe_csi_last_ms, recorded
      with PE_CSI_TIME=1, which the probe sets on the handle it times): every
      repetition changes the alloc index, so pe_csi_check launches the kernel
      again and waits for the code column;
  (b) per-Select time, host clock around pe_select (which ends in a device
      synchronise), on three handles of one build that alternate: the job
      without CSI, the job with CSI and a fixed alloc index (no k_csi_avail
      launch per Select), and the job with CSI and a new alloc index per
      Select (one launch per placement). Every Select is followed by its
      Commit (not timed). All three run the non-speculative path: the probe
      sets PE_SPECULATE=0 before it creates a handle.

Each node runs each of the three plugins with probability 0.97, healthy with
probability 0.97, so about one node in six is unavailable, most windows hold
unavailable nodes and some Selects take the second run of the stop rule; Selects that the
engine hands back (PE_EUNSUPPORTED, the resume corner) are counted, not timed.

    python tools/csi_probe.py [--reps 20] [--selects 200] [--small] [--out profiles/csi/probe.json]

--place: pe_place_csi against the per-placement sequence
(pe_csi_alloc_index, pe_select, pe_commit per placement: the code as it was
before pe_place_csi) on two handles of one build over cluster_c2, for counts
1, 8 and 64, alloc indices 0 .. count - 1. Every repetition starts from
pe_reset_plan and a cursor of its own; the two handles alternate. A Select the
sequence hands back is counted, left out of its time, and the cursor moved on
by one position (so its later placements differ from pe_place_csi's; the
records are compared up to there). k_csi_first and k_csi_loop by HIP events on
a third handle (PE_CSI_TIME=1).

    python tools/csi_probe.py --place [--reps 24] [--small] [--out profiles/csi_place/probe.json]

--place-metrics: pe_place_csi_metrics with AllocMetric on
against pe_place_csi with it off, on two handles of one build over the same
setup (counts 1, 8 and 64, 24 repetitions after 3 warm-up ones, each from
pe_reset_plan and a cursor of its own). Per count: both calls' host-clock time,
the metrics call's split into loop, host walk, trace and maps and the trace log
bytes written per call (pe_place_csi_metrics_stats on a third handle created
with PE_CSI_TIME=1), and whether the records are equal.

    python tools/csi_probe.py --place-metrics [--reps 24] [--small] [--out profiles/csi_place_metrics/probe.json]

--place-full: pe_place_csi_full over cluster_c2 with its nodes
dealt to three datacenters (50 / 30 / 20 %) and a target spread over them in
the job, counts 1, 8 and 64, alloc indices 0 .. count - 1, 24 repetitions after
3 warm-up ones, each from pe_reset_plan and a cursor of its own. Per count: the
call by the host clock, k_csi_first and k_csi_full by HIP events on a handle of
its own (PE_CSI_TIME=1), the placements a call made, pe_place of the same job
without its CSI requests on another handle (the full-pass loop without stops:
a cost reference, not an equal workload), and how many Selects of the
per-placement sequence (pe_csi_alloc_index, pe_select, pe_commit) pe_select
hands back on the same inputs; the sequence of a repetition ends at its first
hand-back, the records are compared up to there. One more leg at count 8
(measure_whole_list): both jobs with a group constraint that makes the group
escape its class, so that no node is a stop and every Select of either call
consumes the whole list. With a library that has no
pe_place_csi_full (PE_ENGINE_LIB: the parent commit's build) only the pe_place
leg runs.

    python tools/csi_probe.py --place-full [--reps 24] [--small] [--out profiles/csi_place_full/probe.json]

--place-full-metrics: pe_place_csi_full_metrics with AllocMetric
on against pe_place_csi_full with it off, on two handles of one build that
alternate, over --place-full's setup (counts 1, 8 and 64, 24 repetitions after
3 warm-up ones, each from pe_reset_plan and a cursor of its own). Per count:
both calls' host-clock time, the metrics call's split into loop, host walk,
trace and maps and the trace log bytes per call (pe_place_csi_metrics_stats on
a third handle created with PE_CSI_TIME=1), and whether the two handles'
records are equal. The same for --place-full's whole-list leg at count 8.

    python tools/csi_probe.py --place-full-metrics [--reps 24] [--small] [--out profiles/csi_place_full_metrics/probe.json]
"""
import argparse
import copy
import ctypes
import json
import os
import sys
import time

import numpy as np

os.environ["PE_SPECULATE"] = "0"
sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from nomad_amd import synth  # noqa: E402
from nomad_amd.stack import GenericStack, SelectOptions, Unsupported  # noqa: E402
from nomad_amd.structs import CSINodePlugin, CSIVolume, CSIVolumeRequest, Constraint, Spread, SpreadTarget  # noqa: E402

REQS = [CSIVolumeRequest("data"), CSIVolumeRequest("scratch", per_alloc=True), CSIVolumeRequest("conf", read_only=True)]


def csi_state(nodes, n_alloc_names, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    volumes = [CSIVolume("data", "default", "p0"), CSIVolume("conf", "default", "p2")]
    volumes += [CSIVolume("scratch[%d]" % i, "default", "p1") for i in range(n_alloc_names)]
    volumes += [CSIVolume("other-%d" % i, "default", "p%d" % (i % 3)) for i in range(6)]
    node_volumes = {}
    for nd in nodes:
        for p in range(3):
            if rng.random() < 0.97:
                nd.csi_node_plugins["p%d" % p] = CSINodePlugin(bool(rng.random() < 0.97), 8)
        k = int(rng.integers(0, 3))
        if k:
            node_volumes[nd.id] = ["other-%d" % int(i) for i in rng.integers(0, 6, k)]
    return volumes, node_volumes


def handle(nodes, allocs, job, perm, volumes=None, node_volumes=None):
    st = GenericStack()
    st.SetState(nodes, allocs)
    if volumes is not None:
        st.SetCSI(volumes, node_volumes)
    st.SetJob(job)
    st.SetNodes(perm)
    return st


def measure(name, nodes, allocs, job, reps, selects):
    perm = synth.shuffle(len(nodes), 5)
    volumes, node_volumes = csi_state(nodes, max(selects, reps) + 1, seed=6)
    csi = copy.deepcopy(job)
    csi.task_groups[0].csi_volumes = list(REQS)
    st_plain = handle(nodes, allocs, job, perm)
    os.environ["PE_CSI_TIME"] = "1"     # read at create: only st_time records the events
    st_time = handle(nodes, allocs, csi, perm, volumes, node_volumes)
    del os.environ["PE_CSI_TIME"]
    st_fixed = handle(nodes, allocs, csi, perm, volumes, node_volumes)
    st_alloc = handle(nodes, allocs, csi, perm, volumes, node_volumes)

    kernel_ms = []
    for r in range(reps + 2):
        st_time.CSIAllocIndex(0, r + 1)
        codes = st_time.CSICheck(0)
        if r >= 2:
            kernel_ms.append(st_time.csi_last_ms())
    st_time.close()
    unavailable = float(np.count_nonzero(codes)) / len(nodes)

    times = {"plain": [], "csi": [], "csi_per_alloc": []}
    handed_back = {"csi": 0, "csi_per_alloc": 0}
    for k in range(selects):
        for key, st, opts in (("plain", st_plain, None), ("csi", st_fixed, None),
                              ("csi_per_alloc", st_alloc, SelectOptions(alloc_index=k))):
            t0 = time.perf_counter()
            try:
                r = st.Select(0, opts)
            except Unsupported:
                handed_back[key] += 1
                st.SetCursor((st.GetCursor()[0] + 1) % len(nodes), st.GetCursor()[1])
                continue
            dt = time.perf_counter() - t0
            if k >= 5:
                times[key].append(dt * 1e6)
            if r is not None:
                st.Commit(0, r.row)

    def stats(v):
        a = np.asarray(v)
        return {"n": int(a.size), "median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)),
                "p90_us": float(np.percentile(a, 90))} if a.size else {"n": 0}
    out = {"nodes": len(nodes), "requests": len(REQS), "unavailable_fraction": unavailable,
           "k_csi_avail_ms": {"reps": len(kernel_ms), "median": float(np.median(kernel_ms)),
                              "min": float(np.min(kernel_ms)), "max": float(np.max(kernel_ms))},
           "select_us": {k: stats(v) for k, v in times.items()}, "handed_back": handed_back}
    print(name, json.dumps(out))
    return out


def measure_place(nodes, allocs, job, reps, counts=(1, 8, 64)):
    perm = synth.shuffle(len(nodes), 5)
    volumes, node_volumes = csi_state(nodes, max(counts) + 1, seed=6)
    csi = copy.deepcopy(job)
    csi.task_groups[0].csi_volumes = list(REQS)
    st_loop = handle(nodes, allocs, csi, perm, volumes, node_volumes)
    st_seq = handle(nodes, allocs, csi, perm, volumes, node_volumes)
    os.environ["PE_CSI_TIME"] = "1"
    st_time = handle(nodes, allocs, csi, perm, volumes, node_volumes)
    del os.environ["PE_CSI_TIME"]
    limit = st_loop.GetCursor()[1]
    n = len(nodes)
    for st in (st_loop, st_seq, st_time):   # (the handle is a 64-bit pointer: never call without argtypes)
        st._lib.pe_flush.restype = ctypes.c_int
        st._lib.pe_flush.argtypes = [ctypes.c_void_p]

    def stats(v):
        a = np.asarray(v, dtype=np.float64)
        return {"n": int(a.size), "median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)),
                "p90_us": float(np.percentile(a, 90))} if a.size else {"n": 0}
    out = {"nodes": n, "requests": len(REQS), "limit": limit, "counts": {}}
    for count in counts:
        idx = list(range(count))
        t_loop, t_seq, first_ms, loop_ms = [], [], [], []
        handed_back = placed_loop = placed_seq = same = compared = 0
        for rep in range(reps + 3):
            cursor = (rep * 977 + 13) % n
            for st in (st_loop, st_seq, st_time):
                st.ResetPlan()
                st.SetJob(csi)
                st.SetNodes(perm)
                st.SetCursor(cursor, limit)
                st._check(st._lib.pe_flush(st._h))
            t0 = time.perf_counter()
            recs = st_loop.PlaceCSI(0, count, alloc_idx=idx)
            dt_loop = (time.perf_counter() - t0) * 1e6
            dt_seq, seq, diverged = 0.0, [], False
            for i in range(count):
                t0 = time.perf_counter()
                try:
                    st_seq.CSIAllocIndex(0, idx[i])
                    r = st_seq.SelectRaw(0)
                except Unsupported:
                    handed_back += rep >= 3
                    diverged = True
                    st_seq.SetCursor((st_seq.GetCursor()[0] + 1) % n, limit)
                    continue
                if r.row >= 0:
                    st_seq.Commit(0, r.row)
                dt_seq += (time.perf_counter() - t0) * 1e6
                if not diverged:
                    seq.append(r)
                if r.row < 0:
                    break
            st_time.PlaceCSI(0, count, alloc_idx=idx)
            ms = st_time.csi_place_ms()
            if rep < 3:
                continue
            t_loop.append(dt_loop)
            t_seq.append(dt_seq)
            first_ms.append(ms[0])
            loop_ms.append(ms[1])
            placed_loop += sum(1 for r in recs if r.row >= 0)
            placed_seq += sum(1 for r in seq if r.row >= 0)
            compared += len(seq)
            same += sum(1 for a, b in zip(recs, seq) if (a.row, a.final_score, a.nodes_evaluated, a.new_offset) ==
                        (b.row, b.final_score, b.nodes_evaluated, b.new_offset))
        out["counts"][str(count)] = {
            "pe_place_csi_us": stats(t_loop), "per_placement_sequence_us": stats(t_seq),
            "k_csi_first_us": stats(np.asarray(first_ms) * 1e3), "k_csi_loop_us": stats(np.asarray(loop_ms) * 1e3),
            "sequence_selects_handed_back": int(handed_back), "placed_per_call": placed_loop / max(1, len(t_loop)),
            "records_compared": int(compared), "records_equal": int(same)}
        print("place", count, json.dumps(out["counts"][str(count)]))
    return out


def measure_place_metrics(nodes, allocs, job, reps, counts=(1, 8, 64)):
    """pe_place_csi_metrics with AllocMetric on against pe_place_csi with it off, on
    two handles of one build that alternate; §40's setup otherwise."""
    perm = synth.shuffle(len(nodes), 5)
    volumes, node_volumes = csi_state(nodes, max(counts) + 1, seed=6)
    csi = copy.deepcopy(job)
    csi.task_groups[0].csi_volumes = list(REQS)
    st_met = handle(nodes, allocs, csi, perm, volumes, node_volumes)
    st_met.EnableMetrics(True)
    st_off = handle(nodes, allocs, csi, perm, volumes, node_volumes)
    os.environ["PE_CSI_TIME"] = "1"     # read at create: only st_time reads the clock inside the call
    st_time = handle(nodes, allocs, csi, perm, volumes, node_volumes)
    del os.environ["PE_CSI_TIME"]
    st_time.EnableMetrics(True)
    limit = st_met.GetCursor()[1]
    n = len(nodes)
    for st in (st_met, st_off, st_time):   # (the handle is a 64-bit pointer: never call without argtypes)
        st._lib.pe_flush.restype = ctypes.c_int
        st._lib.pe_flush.argtypes = [ctypes.c_void_p]

    def stats(v):
        a = np.asarray(v, dtype=np.float64)
        return {"n": int(a.size), "median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)),
                "p90_us": float(np.percentile(a, 90))} if a.size else {"n": 0}
    out = {"nodes": n, "requests": len(REQS), "limit": limit, "counts": {}}
    for count in counts:
        idx = list(range(count))
        t_met, t_off, t_decode, log_bytes, keys = [], [], [], [], []
        split = {"loop": [], "walk": [], "trace": [], "maps": []}
        placed = same = compared = csi_filtered = 0
        for rep in range(reps + 3):
            cursor = (rep * 977 + 13) % n
            for st in (st_met, st_off, st_time):
                st.ResetPlan()
                st.SetJob(csi)
                st.SetNodes(perm)
                st.SetCursor(cursor, limit)
                st._check(st._lib.pe_flush(st._h))
            t0 = time.perf_counter()
            recs = st_met.PlaceCSIMetrics(0, count, alloc_idx=idx)
            dt_met = (time.perf_counter() - t0) * 1e6
            t0 = time.perf_counter()
            maps = st_met.PlaceCSIMaps()
            dt_decode = (time.perf_counter() - t0) * 1e6
            t0 = time.perf_counter()
            plain = st_off.PlaceCSI(0, count, alloc_idx=idx)
            dt_off = (time.perf_counter() - t0) * 1e6
            st_time.PlaceCSIMetrics(0, count, alloc_idx=idx)
            us, nb = st_time.place_csi_metrics_stats()
            if rep < 3:
                continue
            t_met.append(dt_met)
            t_off.append(dt_off)
            t_decode.append(dt_decode)
            log_bytes.append(nb)
            for k, v in zip(("loop", "walk", "trace", "maps"), us):
                split[k].append(v)
            placed += sum(1 for r in recs if r.row >= 0)
            compared += len(plain)
            same += sum(1 for a, b in zip(recs, plain) if (a.row, a.final_score, a.nodes_evaluated, a.nodes_filtered,
                                                            a.new_offset) ==
                        (b.row, b.final_score, b.nodes_evaluated, b.nodes_filtered, b.new_offset))
            assert len(maps) == len(recs)
            csi_filtered += sum(c for m in maps for k, c in m["ConstraintFiltered"].items()
                                if k.startswith(("CSI ", "missing CSI ")))
            keys.append(sum(len(m["ConstraintFiltered"]) for m in maps))
        out["counts"][str(count)] = {
            "pe_place_csi_metrics_on_us": stats(t_met), "pe_place_csi_metrics_off_us": stats(t_off),
            "split_us": {k: stats(v) for k, v in split.items()},
            "python_decode_of_maps_us": stats(t_decode),
            "log_bytes_per_call": {"median": float(np.median(log_bytes)), "min": int(np.min(log_bytes)),
                                   "max": int(np.max(log_bytes))}, "placed_per_call": placed / max(1, len(t_met)),
            "records_compared": int(compared), "records_equal": int(same),
            "csi_filter_entries": int(csi_filtered), "constraint_keys_per_call": float(np.mean(keys))}
        print("place-metrics", count, json.dumps(out["counts"][str(count)]))
    return out


def measure_place_full(nodes, allocs, job, reps, counts=(1, 8, 64)):
    rng = np.random.Generator(np.random.PCG64(17))
    for nd in nodes:
        u = rng.random()
        nd.datacenter = "dc1" if u < 0.5 else ("dc2" if u < 0.8 else "dc3")
        nd.compute_class()
    perm = synth.shuffle(len(nodes), 5)
    volumes, node_volumes = csi_state(nodes, max(counts) + 1, seed=6)
    job = copy.deepcopy(job)
    job.datacenters = ["dc1", "dc2", "dc3"]
    job.spreads = [Spread("${node.datacenter}", 100, [SpreadTarget("dc1", 50), SpreadTarget("dc2", 30)])]
    csi = copy.deepcopy(job)
    csi.task_groups[0].csi_volumes = list(REQS)
    st_plain = handle(nodes, allocs, job, perm)
    have_full = hasattr(st_plain._lib, "pe_place_csi_full")
    hs = [st_plain]
    if have_full:
        st_full = handle(nodes, allocs, csi, perm, volumes, node_volumes)
        st_seq = handle(nodes, allocs, csi, perm, volumes, node_volumes)
        os.environ["PE_CSI_TIME"] = "1"
        st_time = handle(nodes, allocs, csi, perm, volumes, node_volumes)
        del os.environ["PE_CSI_TIME"]
        hs += [st_full, st_seq, st_time]
    limit = st_plain.GetCursor()[1]
    n = len(nodes)
    for st in hs:   # (the handle is a 64-bit pointer: never call without argtypes)
        st._lib.pe_flush.restype = ctypes.c_int
        st._lib.pe_flush.argtypes = [ctypes.c_void_p]

    def stats(v):
        a = np.asarray(v, dtype=np.float64)
        return {"n": int(a.size), "median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)),
                "p90_us": float(np.percentile(a, 90))} if a.size else {"n": 0}
    out = {"nodes": n, "requests": len(REQS), "limit_at_set_nodes": limit, "library_has_pe_place_csi_full": have_full,
           "counts": {}}
    for count in counts:
        idx = list(range(count))
        t_full, t_plain, first_ms, full_ms, evaluated = [], [], [], [], []
        handed_back = answered = placed_full = placed_plain = same = compared = 0
        for rep in range(reps + 3):
            cursor = (rep * 977 + 13) % n
            for st in hs:
                st.ResetPlan()
                st.SetJob(csi if st is not st_plain else job)
                st.SetNodes(perm)
                st.SetCursor(cursor, limit)
                st._check(st._lib.pe_flush(st._h))
            t0 = time.perf_counter()
            plain = st_plain.Place(0, count)
            dt_plain = (time.perf_counter() - t0) * 1e6
            if rep >= 3:
                t_plain.append(dt_plain)
                placed_plain += sum(1 for r in plain if r.row >= 0)
            if not have_full:
                continue
            t0 = time.perf_counter()
            recs = st_full.PlaceCSIFull(0, count, alloc_idx=idx)
            dt_full = (time.perf_counter() - t0) * 1e6
            seq, back = [], 0
            for i in range(count):
                try:
                    st_seq.CSIAllocIndex(0, idx[i])
                    r = st_seq.SelectRaw(0)
                except Unsupported:
                    back = 1
                    break
                seq.append(r)
                if r.row < 0:
                    break
                st_seq.Commit(0, r.row)
            st_time.PlaceCSIFull(0, count, alloc_idx=idx)
            ms = st_time.csi_place_ms()
            if rep < 3:
                continue
            t_full.append(dt_full)
            first_ms.append(ms[0])
            full_ms.append(ms[1])
            handed_back += back
            answered += len(seq)
            placed_full += sum(1 for r in recs if r.row >= 0)
            evaluated.append(sum(r.nodes_evaluated for r in recs))
            compared += len(seq)
            same += sum(1 for a, b in zip(recs, seq) if (a.row, a.final_score, a.nodes_evaluated, a.new_offset) ==
                        (b.row, b.final_score, b.nodes_evaluated, b.new_offset))
        res = {"pe_place_without_csi_us": stats(t_plain), "pe_place_placed_per_call": placed_plain / max(1, len(t_plain))}
        if have_full:
            res.update({
                "pe_place_csi_full_us": stats(t_full), "k_csi_first_us": stats(np.asarray(first_ms) * 1e3),
                "k_csi_full_us": stats(np.asarray(full_ms) * 1e3), "placed_per_call": placed_full / max(1, len(t_full)),
                "positions_consumed_per_call": float(np.mean(evaluated)),
                "ratio_to_pe_place_median": float(np.median(t_full) / np.median(t_plain)),
                "sequence_selects_answered": int(answered), "sequence_repetitions_handed_back": int(handed_back),
                "records_compared": int(compared), "records_equal": int(same)})
        out["counts"][str(count)] = res
        print("place-full", count, json.dumps(res))
    if have_full:
        out["whole_list_count_8"] = measure_whole_list(nodes, allocs, job, csi, perm, volumes, node_volumes, reps)
        print("place-full whole list", json.dumps(out["whole_list_count_8"]))
    return out


def measure_whole_list(nodes, allocs, job, csi, perm, volumes, node_volumes, reps, count=8):
    """The same two jobs with a group constraint on node.unique.id that every
    node passes: the group escapes its class, so no unavailable node is a stop
    and every Select of pe_place_csi_full consumes the whole list, as every
    Select of pe_place does: the same number of positions per placement, the
    unavailable nodes filtered in one and options in the other."""
    job, csi = copy.deepcopy(job), copy.deepcopy(csi)
    for j in (job, csi):
        j.task_groups[0].constraints = list(j.task_groups[0].constraints) + [
            Constraint("${node.unique.id}", "no-such-node", "!=")]
    st_plain = handle(nodes, allocs, job, perm)
    st_full = handle(nodes, allocs, csi, perm, volumes, node_volumes)
    os.environ["PE_CSI_TIME"] = "1"
    st_time = handle(nodes, allocs, csi, perm, volumes, node_volumes)
    del os.environ["PE_CSI_TIME"]
    limit, n = st_plain.GetCursor()[1], len(nodes)
    for st in (st_plain, st_full, st_time):
        st._lib.pe_flush.restype = ctypes.c_int
        st._lib.pe_flush.argtypes = [ctypes.c_void_p]
    t_full, t_plain, full_ms, consumed, placed = [], [], [], [], 0
    for rep in range(reps + 3):
        for st in (st_plain, st_full, st_time):
            st.ResetPlan()
            st.SetJob(csi if st is not st_plain else job)
            st.SetNodes(perm)
            st.SetCursor((rep * 977 + 13) % n, limit)
            st._check(st._lib.pe_flush(st._h))
        t0 = time.perf_counter()
        st_plain.Place(0, count)
        dt_plain = (time.perf_counter() - t0) * 1e6
        t0 = time.perf_counter()
        recs = st_full.PlaceCSIFull(0, count, alloc_idx=list(range(count)))
        dt_full = (time.perf_counter() - t0) * 1e6
        st_time.PlaceCSIFull(0, count, alloc_idx=list(range(count)))
        ms = st_time.csi_place_ms()
        if rep < 3:
            continue
        t_plain.append(dt_plain)
        t_full.append(dt_full)
        full_ms.append(ms[1] * 1e3)
        consumed.append(sum(r.nodes_evaluated for r in recs))
        placed += sum(1 for r in recs if r.row >= 0)

    def stats(v):
        a = np.asarray(v, dtype=np.float64)
        return {"n": int(a.size), "median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)),
                "p90_us": float(np.percentile(a, 90))}
    return {"count": count, "pe_place_csi_full_us": stats(t_full), "pe_place_without_csi_us": stats(t_plain),
            "k_csi_full_us": stats(full_ms), "placed_per_call": placed / max(1, len(t_full)),
            "positions_consumed_per_call": float(np.mean(consumed)),
            "ratio_to_pe_place_median": float(np.median(t_full) / np.median(t_plain))}


def full_metrics_leg(nodes, allocs, csi, perm, volumes, node_volumes, reps, count):
    """One count of --place-full-metrics: metrics on against metrics off, alternating."""
    st_met = handle(nodes, allocs, csi, perm, volumes, node_volumes)
    st_met.EnableMetrics(True)
    st_off = handle(nodes, allocs, csi, perm, volumes, node_volumes)
    os.environ["PE_CSI_TIME"] = "1"     # read at create: only st_time reads the clock inside the call
    st_time = handle(nodes, allocs, csi, perm, volumes, node_volumes)
    del os.environ["PE_CSI_TIME"]
    st_time.EnableMetrics(True)
    limit, n = st_met.GetCursor()[1], len(nodes)
    for st in (st_met, st_off, st_time):   # (the handle is a 64-bit pointer: never call without argtypes)
        st._lib.pe_flush.restype = ctypes.c_int
        st._lib.pe_flush.argtypes = [ctypes.c_void_p]

    def stats(v):
        a = np.asarray(v, dtype=np.float64)
        return {"n": int(a.size), "median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)),
                "p90_us": float(np.percentile(a, 90))} if a.size else {"n": 0}
    idx = list(range(count))
    t_met, t_off, log_bytes, consumed, scored = [], [], [], [], []
    split = {"loop": [], "walk": [], "trace": [], "maps": []}
    placed = same = compared = csi_filtered = 0
    for rep in range(reps + 3):
        cursor = (rep * 977 + 13) % n
        for st in (st_met, st_off, st_time):
            st.ResetPlan()
            st.SetJob(csi)
            st.SetNodes(perm)
            st.SetCursor(cursor, limit)
            st._check(st._lib.pe_flush(st._h))
        t0 = time.perf_counter()
        recs = st_met.PlaceCSIFullMetrics(0, count, alloc_idx=idx)
        dt_met = (time.perf_counter() - t0) * 1e6
        maps = st_met.PlaceCSIMaps()
        t0 = time.perf_counter()
        plain = st_off.PlaceCSIFull(0, count, alloc_idx=idx)
        dt_off = (time.perf_counter() - t0) * 1e6
        st_time.PlaceCSIFullMetrics(0, count, alloc_idx=idx)
        us, nb = st_time.place_csi_metrics_stats()
        if rep < 3:
            continue
        t_met.append(dt_met)
        t_off.append(dt_off)
        log_bytes.append(nb)
        for k, v in zip(("loop", "walk", "trace", "maps"), us):
            split[k].append(v)
        placed += sum(1 for r in recs if r.row >= 0)
        consumed.append(sum(r.nodes_evaluated for r in recs))
        compared += max(len(plain), len(recs))
        same += sum(1 for a, b in zip(recs, plain)
                    if (a.row, a.final_score, list(a.scores), a.nodes_evaluated, a.nodes_filtered, a.nodes_exhausted,
                        a.new_offset) ==
                    (b.row, b.final_score, list(b.scores), b.nodes_evaluated, b.nodes_filtered, b.nodes_exhausted,
                     b.new_offset))
        assert len(maps) == len(recs)
        csi_filtered += sum(c for m in maps for k, c in m["ConstraintFiltered"].items()
                            if k.startswith(("CSI ", "missing CSI ")))
        scored.append(sum(len(m["ScoreMetaData"]) for m in maps))
    for st in (st_met, st_off, st_time):
        st.close()
    return {"count": count,
            "pe_place_csi_full_metrics_on_us": stats(t_met), "pe_place_csi_full_metrics_off_us": stats(t_off),
            "ratio_on_to_off_median": float(np.median(t_met) / np.median(t_off)),
            "split_us": {k: stats(v) for k, v in split.items()},
            "log_bytes_per_call": {"median": float(np.median(log_bytes)), "min": int(np.min(log_bytes)),
                                   "max": int(np.max(log_bytes))},
            "positions_consumed_per_call": float(np.mean(consumed)), "placed_per_call": placed / max(1, len(t_met)),
            "records_compared": int(compared), "records_equal": int(same),
            "csi_filter_entries": int(csi_filtered), "score_items_per_call": float(np.mean(scored))}


def measure_place_full_metrics(nodes, allocs, job, reps, counts=(1, 8, 64)):
    """--place-full's setup (three datacenters, a target spread at job level); the
    whole-list leg adds the group constraint that makes the group escape its class."""
    rng = np.random.Generator(np.random.PCG64(17))
    for nd in nodes:
        u = rng.random()
        nd.datacenter = "dc1" if u < 0.5 else ("dc2" if u < 0.8 else "dc3")
        nd.compute_class()
    perm = synth.shuffle(len(nodes), 5)
    volumes, node_volumes = csi_state(nodes, max(counts) + 1, seed=6)
    csi = copy.deepcopy(job)
    csi.datacenters = ["dc1", "dc2", "dc3"]
    csi.spreads = [Spread("${node.datacenter}", 100, [SpreadTarget("dc1", 50), SpreadTarget("dc2", 30)])]
    csi.task_groups[0].csi_volumes = list(REQS)
    out = {"nodes": len(nodes), "requests": len(REQS), "counts": {}}
    for count in counts:
        out["counts"][str(count)] = full_metrics_leg(nodes, allocs, csi, perm, volumes, node_volumes, reps, count)
        print("place-full-metrics", count, json.dumps(out["counts"][str(count)]))
    whole = copy.deepcopy(csi)
    whole.task_groups[0].constraints = list(whole.task_groups[0].constraints) + [
        Constraint("${node.unique.id}", "no-such-node", "!=")]
    out["whole_list_count_8"] = full_metrics_leg(nodes, allocs, whole, perm, volumes, node_volumes, reps, 8)
    print("place-full-metrics whole list", json.dumps(out["whole_list_count_8"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--place", action="store_true", help="the pe_place_csi leg (DESIGN.md §40)")
    ap.add_argument("--place-metrics", action="store_true", help="the pe_place_csi_metrics leg (DESIGN.md §41)")
    ap.add_argument("--place-full", action="store_true", help="the pe_place_csi_full leg (DESIGN.md §43)")
    ap.add_argument("--place-full-metrics", action="store_true", help="the pe_place_csi_full_metrics leg (DESIGN.md §45)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--selects", type=int, default=200)
    ap.add_argument("--small", action="store_true", help="1/10 of the node counts (rehearsal)")
    ap.add_argument("--out", default="profiles/csi/probe.json")
    a = ap.parse_args()
    scale = 10 if a.small else 1
    res = {"tool": "tools/csi_probe.py", "speculate": 0}
    if a.place_full_metrics:
        out = a.out if a.out != "profiles/csi/probe.json" else "profiles/csi_place_full_metrics/probe.json"
        nodes, allocs = synth.cluster_c2(10000 // scale, seed=42)
        res["tool"] += " --place-full-metrics"
        res["cluster_c2"] = measure_place_full_metrics(nodes, allocs, synth.job_c2(64), max(a.reps, 24))
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    if a.place_full:
        out = a.out if a.out != "profiles/csi/probe.json" else "profiles/csi_place_full/probe.json"
        nodes, allocs = synth.cluster_c2(10000 // scale, seed=42)
        res["tool"] += " --place-full"
        res["cluster_c2"] = measure_place_full(nodes, allocs, synth.job_c2(64), max(a.reps, 24))
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    if a.place_metrics:
        out = a.out if a.out != "profiles/csi/probe.json" else "profiles/csi_place_metrics/probe.json"
        nodes, allocs = synth.cluster_c2(10000 // scale, seed=42)
        res["tool"] += " --place-metrics"
        res["cluster_c2"] = measure_place_metrics(nodes, allocs, synth.job_c2(64), max(a.reps, 24))
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    if a.place:
        out = a.out if a.out != "profiles/csi/probe.json" else "profiles/csi_place/probe.json"
        nodes, allocs = synth.cluster_c2(10000 // scale, seed=42)
        res["tool"] += " --place"
        res["cluster_c2"] = measure_place(nodes, allocs, synth.job_c2(64), max(a.reps, 20))
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    nodes, allocs = synth.cluster_c2(10000 // scale, seed=42)
    res["cluster_c2"] = measure("cluster_c2", nodes, allocs, synth.job_c2(a.selects), a.reps, a.selects)
    nodes, allocs = synth.cluster_c4(100000 // scale, seed=11)
    res["cluster_c4"] = measure("cluster_c4", nodes, allocs, synth.job_c2(a.selects), a.reps, a.selects)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
