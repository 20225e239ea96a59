"""Host-side mirror of the reference `scheduler.Stack` interface over a C ABI.

`GenericStack` / `SystemStack` keep the reference's method names and argument
meaning (scheduler/stack.go:23-39): SetNodes, SetJob, Select. `Place` is the
fused count loop of GenericScheduler.computePlacements (generic_sched.go:493-649)
and `SystemPlace` the SystemScheduler one (scheduler_system.go:283-425).

The product backend is nomad_amd/libnomadpe.so (HIP, gfx950). There is no CPU
fallback: constructing an engine stack without the library or without a GPU
raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import abi
from .encode import EncodedCSI, EncodedJob, EncodedState, Interner, encode_csi_requests
from .structs import Allocation, Job, Node, SchedulerConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
# PE_ENGINE_LIB: an A/B build of the same sources (measurement runs only)
ENGINE_LIB = os.environ.get("PE_ENGINE_LIB") or os.path.join(_HERE, "libnomadpe.so")


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (code %d)" % (msg, code))
        self.code = code


class Unsupported(EngineError):
    pass


_engine = None


def load_engine():
    """Load the HIP engine library (fails loudly when it is missing)."""
    global _engine
    if _engine is None:
        if not os.path.exists(ENGINE_LIB):
            raise EngineError(-1, "nomad_amd/libnomadpe.so is not built: run __graft_entry__.build()")
        lib = C.CDLL(ENGINE_LIB)
        abi.bind(lib, "pe_", "pe_stack_create", "pe_stack_destroy", "pe_last_error")
        lib.pe_abi_version.restype = C.c_uint32
        lib.pe_last_kernel_ms.restype = C.c_double
        lib.pe_last_kernel_ms.argtypes = [C.c_void_p]
        lib.pe_last_sweep_bytes.restype = C.c_uint32
        lib.pe_last_sweep_bytes.argtypes = [C.c_void_p]
        lib.pe_set_kernel_split.restype = C.c_int
        lib.pe_set_kernel_split.argtypes = [C.c_void_p, C.c_int]
        lib.pe_last_kernel_split.restype = C.c_int
        lib.pe_last_kernel_split.argtypes = [C.c_void_p, abi.f64p]
        lib.pe_stage_orders.restype = C.c_int
        lib.pe_stage_orders.argtypes = [C.c_void_p, abi.u32p, C.c_uint32, C.c_uint32]
        lib.pe_place_batch.restype = C.c_int
        lib.pe_place_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(abi.pe_placement), abi.u32p]
        lib.pe_batch_results.restype = C.c_int
        lib.pe_batch_results.argtypes = [C.c_void_p, C.POINTER(C.POINTER(abi.pe_placement)),
                                         C.POINTER(abi.u32p), abi.u32p, abi.u32p]
        lib.pe_last_phase_ms.restype = None
        lib.pe_last_phase_ms.argtypes = [C.c_void_p, abi.f64p]
        lib.pe_select_shard.restype = C.c_int
        lib.pe_select_shard.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.POINTER(abi.pe_shard_rec)]
        lib.pe_inplace_update.restype = C.c_int
        lib.pe_inplace_update.argtypes = [C.c_void_p, C.c_uint32, abi.u32p, C.c_uint32,
                                          C.POINTER(abi.pe_ranked_node), abi.u8p, abi.u32p]
        if hasattr(lib, "pe_inplace_update_preempt"):
            lib.pe_inplace_update_preempt.restype = C.c_int
            lib.pe_inplace_update_preempt.argtypes = lib.pe_inplace_update.argtypes
            lib.pe_inplace_update_preempted.restype = C.c_int
            lib.pe_inplace_update_preempted.argtypes = [C.c_void_p, C.POINTER(abi.u32p), C.POINTER(abi.u32p),
                                                        C.POINTER(abi.u32p), abi.u32p]
        if hasattr(lib, "pe_inplace_update_metrics"):
            lib.pe_inplace_update_metrics.restype = C.c_int
            lib.pe_inplace_update_metrics.argtypes = lib.pe_inplace_update.argtypes
            lib.pe_inplace_metrics.restype = C.c_int
            lib.pe_inplace_metrics.argtypes = [C.c_void_p, C.POINTER(C.POINTER(abi.pe_inplace_metric)), abi.u32p,
                                               C.POINTER(C.POINTER(abi.pe_metric_score)), abi.u32p]
        if hasattr(lib, "pe_inplace_update_spread"):
            lib.pe_inplace_update_spread.restype = C.c_int
            lib.pe_inplace_update_spread.argtypes = lib.pe_inplace_update.argtypes
            lib.pe_inplace_spread_ms.restype = C.c_int
            lib.pe_inplace_spread_ms.argtypes = [C.c_void_p, abi.f64p]
        if hasattr(lib, "pe_inplace_update_csi"):
            lib.pe_inplace_update_csi.restype = C.c_int
            lib.pe_inplace_update_csi.argtypes = [C.c_void_p, C.c_uint32, abi.u32p, abi.u32p, C.c_uint32,
                                                  C.POINTER(abi.pe_ranked_node), abi.u8p, abi.u32p]
        if hasattr(lib, "pe_system_place_groups"):   # present or absent behind one ABI version
            lib.pe_system_place_groups.restype = C.c_int
            lib.pe_system_place_groups.argtypes = [C.c_void_p, abi.u32p, C.c_uint32, abi.f64p, abi.u8p, abi.u32p,
                                                   abi.u32p]
            lib.pe_system_groups_results.restype = C.c_int
            lib.pe_system_groups_results.argtypes = [C.c_void_p, C.POINTER(abi.f64p), C.POINTER(abi.u8p),
                                                     C.POINTER(abi.u32p), abi.u32p, abi.u32p, abi.u32p]
        if hasattr(lib, "pe_system_place_groups_preempt"):
            lib.pe_system_place_groups_preempt.restype = C.c_int
            lib.pe_system_place_groups_preempt.argtypes = [C.c_void_p, abi.u32p, C.c_uint32, abi.f64p, abi.u8p,
                                                           abi.u32p, abi.u32p]
            lib.pe_system_groups_preempted.restype = C.c_int
            lib.pe_system_groups_preempted.argtypes = [C.c_void_p, C.POINTER(abi.u32p), C.POINTER(abi.u32p),
                                                       C.POINTER(abi.u32p), abi.u32p]
        if hasattr(lib, "pe_system_place_groups_metrics"):
            lib.pe_system_place_groups_metrics.restype = C.c_int
            lib.pe_system_place_groups_metrics.argtypes = [C.c_void_p, abi.u32p, C.c_uint32, abi.f64p, abi.u8p,
                                                           abi.u32p, abi.u32p]
            lib.pe_system_groups_metrics.restype = C.c_int
            lib.pe_system_groups_metrics.argtypes = [C.c_void_p, C.POINTER(C.POINTER(abi.pe_sysg_failure)),
                                                     C.POINTER(C.c_int32), C.POINTER(abi.f64p), C.POINTER(abi.f64p),
                                                     abi.u32p]
        if hasattr(lib, "pe_set_csi"):
            abi.bind_csi(lib)
        lib.pe_speculation_stats.restype = C.c_int
        lib.pe_speculation_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.pe_chain_wide_stats.restype = C.c_int
        lib.pe_chain_wide_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        if hasattr(lib, "pe_chain_wide_launches"):
            lib.pe_chain_wide_launches.restype = C.c_int
            lib.pe_chain_wide_launches.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
            lib.pe_chain_wide_one_lds.restype = C.c_int
            lib.pe_chain_wide_one_lds.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        lib.pe_comm_unique_id.restype = C.c_int
        lib.pe_comm_unique_id.argtypes = [abi.u8p, C.c_size_t]
        lib.pe_comm_init.restype = C.c_int
        lib.pe_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, abi.u8p]
        lib.pe_place_sharded.restype = C.c_int
        lib.pe_place_sharded.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(abi.pe_ranked_node), abi.u32p]
        lib.pe_comm_init_host.restype = C.c_int
        lib.pe_comm_init_host.argtypes = [C.c_void_p, C.c_int, C.c_int, abi.pe_exchange_fn, C.c_void_p]
        lib.pe_last_exchange_us.restype = C.c_double
        lib.pe_last_exchange_us.argtypes = [C.c_void_p]
        lib.pe_select_merge.restype = C.c_int
        lib.pe_select_merge.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(abi.pe_shard_rec), C.c_uint32,
                                        C.POINTER(abi.pe_ranked_node)]
        _engine = lib
    return _engine


def parse_metrics(text: str) -> Dict:
    """pe_last_metrics' text (also a served record's maps in pe_spec_view) as
    {"ClassFiltered": {...}, "ConstraintFiltered": {...}, "ClassExhausted":
    {...}, "DimensionExhausted": {...}, "ScoreMetaData": [(node id, NormScore,
    {scorer: score}), ...]}."""
    names = {"CF": "ClassFiltered", "KF": "ConstraintFiltered", "CE": "ClassExhausted",
             "DE": "DimensionExhausted"}
    out = {v: {} for v in names.values()}
    out["ScoreMetaData"] = []
    for line in text.split("\n"):
        if not line:
            continue
        if line.startswith("SM\t"):   # PopulateScoreMetaData: top 5 by NormScore, descending
            _, _, node_id, norm, parts = line.split("\t")
            scores = dict((k, float(v)) for k, v in (p.split("=") for p in parts.split(",") if p))
            out["ScoreMetaData"].append((node_id, float(norm), scores))
            continue
        kind, key, cnt = line.split("\t")
        out[names[kind]][key] = int(cnt)
    return out


_KIND_NAMES = {abi.PE_METRIC_CLASS_FILTERED: "ClassFiltered", abi.PE_METRIC_CONSTRAINT_FILTERED: "ConstraintFiltered",
               abi.PE_METRIC_CLASS_EXHAUSTED: "ClassExhausted",
               abi.PE_METRIC_DIMENSION_EXHAUSTED: "DimensionExhausted"}


def decode_metrics(stack, counts, c0: int, c1: int, scores, s0: int, s1: int) -> Dict:
    """Binary AllocMetric maps (pe_metric_count[c0:c1], pe_metric_score[s0:s1])
    in parse_metrics' shape; keys resolved through pe_metric_string."""
    out = {v: {} for v in _KIND_NAMES.values()}
    out["ScoreMetaData"] = []
    cache = getattr(stack, "_mkey_cache", None)
    if cache is None:
        cache = stack._mkey_cache = {}
    for i in range(c0, c1):
        e = counts[i]
        k = cache.get(e.key)
        if k is None:
            k = cache[e.key] = stack.MetricString(e.key)
        out[_KIND_NAMES[e.kind]][k] = int(e.count)
    for i in range(s0, s1):
        m = scores[i]
        parts = {abi.SCORER_NAMES[m.scorer[j]]: float(m.score[j]) for j in range(m.n_scores)}
        nid = stack.nodes[m.row].id if stack.nodes is not None else stack.state.node_id(m.row)
        out["ScoreMetaData"].append((nid, float(m.norm), parts))
    return out


def view_metrics(stack, view, k: int) -> Dict:
    """Record k's maps from the served-Select view (pe_spec_view.mcounts / mscores)."""
    return decode_metrics(stack, view.mcounts, view.mcounts_off[k], view.mcounts_off[k + 1],
                          view.mscores, view.mscores_off[k], view.mscores_off[k + 1])


@dataclass
class SelectOptions:
    """SelectOptions (stack.go:34-39); nodes are given as node IDs or rows."""
    penalty_node_ids: Sequence[str] = ()
    preferred_nodes: Sequence[str] = ()
    preempt: bool = False
    alloc_name: str = ""
    # AllocSuffix of the alloc being placed: per_alloc CSI sources take "[alloc_index]"
    alloc_index: Optional[int] = None


def _core_ids(mask) -> List[int]:
    """Core ids of a 256-bit pe_ranked_node.reserved_cores mask, ascending."""
    out = []
    for w in range(4):
        m = int(mask[w])
        while m:
            low = m & -m
            out.append(64 * w + low.bit_length() - 1)
            m ^= low
    return out


@dataclass
class RankedNode:
    """RankedNode (rank.go:21-36) plus the AllocMetric counters."""
    row: int
    node: Optional[Node]
    final_score: float
    scores: List[float] = field(default_factory=list)
    nodes_evaluated: int = 0
    nodes_filtered: int = 0
    nodes_exhausted: int = 0
    new_offset: int = 0
    preempted: List[int] = field(default_factory=list)   # PreemptedAllocs: alloc-table rows
    device_offers: List[int] = field(default_factory=list)   # chosen device group per request
    reserved_cores: List[int] = field(default_factory=list)  # Cpu.ReservedCores of the tasks, ascending

    @classmethod
    def from_c(cls, r: abi.pe_ranked_node, nodes, full_preempted=None):
        """`full_preempted`: the whole PreemptedAllocs list when the record
        carries more than PE_MAX_PREEMPT (pe_preempted_of)."""
        pre = list(full_preempted) if full_preempted is not None else \
            [r.preempted[i] for i in range(min(r.n_preempted, abi.PE_MAX_PREEMPT))]
        return cls(row=r.row, node=nodes[r.row] if (nodes is not None and r.row >= 0) else None,
                   final_score=r.final_score,
                   scores=[r.scores[i] for i in range(r.n_scores)], nodes_evaluated=r.nodes_evaluated,
                   nodes_filtered=r.nodes_filtered, nodes_exhausted=r.nodes_exhausted,
                   new_offset=r.new_offset, preempted=pre,
                   device_offers=[r.device_offer_group[i] for i in range(r.n_device_offers)],
                   reserved_cores=_core_ids(r.reserved_cores))


class _Stack:
    """Stack over a C ABI with a given symbol prefix (engine: 'pe_')."""

    stack_kind = abi.PE_STACK_GENERIC

    def __init__(self, lib, prefix: str, batch: bool = False, config: SchedulerConfig = None,
                 device: int = 0, devices: Optional[Sequence[int]] = None):
        self._lib = lib
        self._p = prefix
        config = config or SchedulerConfig()
        cfg = abi.pe_config()
        cfg.stack_kind = self.stack_kind
        cfg.batch = int(batch)
        cfg.algorithm = abi.PE_ALGO_SPREAD if config.algorithm == "spread" else abi.PE_ALGO_BINPACK
        cfg.memory_oversubscription = int(config.memory_oversubscription)
        cfg.preempt = int(config.preempt_system if self.stack_kind == abi.PE_STACK_SYSTEM
                          else config.preempt_service)
        cfg.device = device
        if devices is not None and len(devices) > 1:   # one handle over several GPUs (pe_config.device_ids)
            if len(devices) > 8:
                raise ValueError("at most 8 devices per handle")
            cfg.device_count = len(devices)
            for k, d in enumerate(devices):
                cfg.device_ids[k] = int(d)
        self._cfg = cfg
        create = getattr(lib, prefix + ("stack_create" if prefix == "pe_" else "create"))
        self._h = create(C.byref(cfg))
        if not self._h:
            err = getattr(lib, prefix + "last_error")(None)
            raise EngineError(-1, (err or b"stack creation failed").decode())
        self.state: Optional[EncodedState] = None
        self.job: Optional[EncodedJob] = None
        self.nodes: List[Node] = []
        self.limit = None
        self.csi: Optional[EncodedCSI] = None

    def close(self):
        if self._h:
            destroy = getattr(self._lib, self._p + ("stack_destroy" if self._p == "pe_" else "destroy"))
            destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != abi.PE_OK:
            msg = getattr(self._lib, self._p + "last_error")(self._h).decode()
            raise (Unsupported if rc == abi.PE_EUNSUPPORTED else EngineError)(rc, msg)

    def _fn(self, name):
        return getattr(self._lib, self._p + name)

    # -- AllocMetric maps (structs.go:9826-10026) ------------------------------
    def EnableMetrics(self, on: bool = True):
        """Collect ClassFiltered / ConstraintFiltered / ClassExhausted /
        DimensionExhausted per Select (before the eval's first Select)."""
        if hasattr(self._lib, self._p + "set_metrics"):
            fn = self._fn("set_metrics")
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.c_int]
            self._check(fn(self._h, int(on)))
            self._metrics_on = bool(on)

    def LastMetrics(self) -> Dict[str, Dict[str, int]]:
        """The last Select's maps: {"ClassFiltered": {...}, "ConstraintFiltered": {...},
        "ClassExhausted": {...}, "DimensionExhausted": {...}, "ScoreMetaData":
        [(node id, NormScore, {scorer: score}), ...]}."""
        fn = self._fn("last_metrics")
        fn.restype = C.c_int64
        fn.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        need = fn(self._h, None, 0)
        if need < 0:
            self._check(int(need))
        buf = C.create_string_buffer(int(need) + 1)
        fn(self._h, buf, len(buf))
        return parse_metrics(buf.value.decode())

    def LastMetricsBin(self) -> Dict:
        """The last Select's maps from their binary form (pe_last_metrics_bin),
        in LastMetrics' shape: what the Go shim reads without parsing text."""
        lib = self._lib
        lib.pe_last_metrics_bin.restype = C.c_int
        lib.pe_last_metrics_bin.argtypes = [C.c_void_p, C.POINTER(C.POINTER(abi.pe_metric_count)), abi.u32p,
                                            C.POINTER(C.POINTER(abi.pe_metric_score)), abi.u32p]
        c, sc = C.POINTER(abi.pe_metric_count)(), C.POINTER(abi.pe_metric_score)()
        nc, ns = C.c_uint32(0), C.c_uint32(0)
        self._check(lib.pe_last_metrics_bin(self._h, C.byref(c), C.byref(nc), C.byref(sc), C.byref(ns)))
        return decode_metrics(self, c, 0, nc.value, sc, 0, ns.value)

    def MetricString(self, key: int) -> str:
        """pe_metric_string: the text of an AllocMetric key."""
        fn = self._lib.pe_metric_string
        fn.restype = C.c_int64
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t]
        need = fn(self._h, key, None, 0)
        if need < 0:
            self._check(int(need))
        buf = C.create_string_buffer(int(need) + 1)
        fn(self._h, key, buf, len(buf))
        return buf.value.decode()

    # -- EvalEligibility and iterator state (context.go:190-356) -------------
    def Eligibility(self, changed_only: bool = False) -> Dict:
        """The evaluation's EvalEligibility maps as the reference chain holds
        them: {"job": {class: eligible}, "tgs": {tg name: {class: eligible}},
        "escaped": HasEscaped()} (pe_get_eligibility)."""
        fn = self._fn("get_eligibility")
        n, flags = C.c_uint32(0), C.c_uint32(0)
        self._check(fn(self._h, int(changed_only), None, 0, C.byref(n), C.byref(flags)))
        buf = (abi.pe_class_feas * max(1, n.value))()
        self._check(fn(self._h, int(changed_only), buf, n.value, C.byref(n), C.byref(flags)))
        strs = self.state.interner.strs
        out = {"job": {}, "tgs": {}, "escaped": bool(flags.value & abi.PE_ELIG_ESCAPED)}
        for e in buf[:n.value]:
            cls, ok = strs[e.computed_class], e.status == abi.PE_CLASS_ELIGIBLE
            if e.task_group == abi.PE_NONE:
                out["job"][cls] = ok
            else:
                out["tgs"].setdefault(strs[e.task_group], {})[cls] = ok
        return out

    def PutEligibility(self, elig: Dict):
        """Load EvalEligibility maps ({"job": ..., "tgs": ...}) into this stack's memo."""
        it = self.state.interner
        ents = [(abi.PE_NONE, it.intern(c), ok) for c, ok in elig.get("job", {}).items()]
        for tg, m in elig.get("tgs", {}).items():
            ents += [(it.intern(tg), it.intern(c), ok) for c, ok in m.items()]
        buf = (abi.pe_class_feas * max(1, len(ents)))()
        for k, (tg, c, ok) in enumerate(ents):
            buf[k].task_group, buf[k].computed_class = tg, c
            buf[k].status = abi.PE_CLASS_ELIGIBLE if ok else abi.PE_CLASS_INELIGIBLE
        self._check(self._fn("put_eligibility")(self._h, buf, len(ents)))

    @staticmethod
    def GetClasses(elig: Dict) -> Dict[str, bool]:
        """EvalEligibility.GetClasses (context.go:253-290) over Eligibility()'s maps."""
        out: Dict[str, bool] = {}
        for classes in elig["tgs"].values():
            for cls, ok in classes.items():
                if ok:
                    out[cls] = True
                elif cls not in out:
                    out[cls] = False
        for cls, ok in elig["job"].items():
            if ok:
                out.setdefault(cls, True)
            else:
                out[cls] = False
        return out

    def GetCursor(self):
        """(StaticIterator offset, LimitIterator limit)."""
        off, lim = C.c_uint32(0), C.c_uint32(0)
        self._check(self._fn("get_cursor")(self._h, C.byref(off), C.byref(lim)))
        return off.value, lim.value

    def SetCursor(self, offset: int, limit: int, tg=None):
        """Adopt another chain's cursor and limit; `tg`: the task group it
        selected for (its SpreadIterator.SetTaskGroup ran)."""
        tgi = abi.PE_NONE if tg is None else self._tg_index(tg)
        self._check(self._fn("set_cursor")(self._h, tgi, int(offset), int(limit)))

    # -- scheduler.State snapshot -------------------------------------------
    def SetState(self, nodes: Sequence[Node], allocs: Sequence[Allocation] = ()):
        self.nodes = list(nodes)
        self.csi = None   # the table goes with the snapshot
        self.state = EncodedState(nodes, allocs, Interner())
        t = self.state.strtab()
        self._check(self._fn("set_state")(self._h, C.byref(t), C.byref(self.state.node_table),
                                          C.byref(self.state.alloc_table)))
        return self.state

    # -- CSI volumes (CSIVolumeChecker, feasible.go:209-337) ---------------------
    def SetCSI(self, volumes, node_volumes=None):
        """The snapshot's CSI state (pe_set_csi): `volumes` CSIVolume objects,
        `node_volumes` node id -> ids of the volumes CSIVolumesByNodeID yields;
        the plugins come from Node.csi_node_plugins. None drops the table.
        SetState, UpdateNodes and UpdateAllocs drop it too."""
        if volumes is None:
            self._check(self._lib.pe_set_csi(self._h, None, None))
            self.csi = None
            return None
        self.csi = EncodedCSI(self.state.nodes, list(volumes), node_volumes, self.state.interner)
        t = self.csi.strtab()
        self._check(self._lib.pe_set_csi(self._h, C.byref(t), C.byref(self.csi.table)))
        return self.csi

    def CSICheck(self, tg) -> np.ndarray:
        """pe_csi_check: the availability code of every snapshot row for `tg`
        (0, or request index << 3 | reason)."""
        out = np.zeros(max(1, len(self.state.nodes)), dtype=np.uint16)
        self._check(self._lib.pe_csi_check(self._h, self._tg_index(tg), out.ctypes.data_as(abi.u16p)))
        return out[:len(self.state.nodes)]

    def CSIAllocIndex(self, tg, idx: int):
        self._check(self._lib.pe_csi_alloc_index(self._h, self._tg_index(tg), int(idx)))

    def csi_last_ms(self) -> float:
        return float(self._lib.pe_csi_last_ms(self._h))

    def PlaceCSI(self, tg, count: int, alloc_idx=None) -> List[RankedNode]:
        """pe_place_csi: computePlacements' loop for `count` fresh placements of
        a group with CSI requests in one launch; `alloc_idx[i]` is the name index
        of placement i's alloc (per_alloc sources), None: the index CSIAllocIndex
        holds. The records of the placements and, if the loop ended early, of the
        failed Select. A group without CSI requests: Place."""
        out = (abi.pe_ranked_node * max(1, count))()
        placed = C.c_uint32(0)
        idx = None
        if alloc_idx is not None:
            if len(alloc_idx) != count:
                raise ValueError("alloc_idx needs one index per placement")
            idx = (C.c_uint32 * max(1, count))(*[int(i) for i in alloc_idx])
        self._check(self._lib.pe_place_csi(self._h, self._tg_index(tg), count, idx, out, C.byref(placed)))
        n = min(count, placed.value + 1)
        return [RankedNode.from_c(out[i], self.nodes, self._full_preempted(i, out[i])) for i in range(n)]

    def PlaceCSIFull(self, tg, count: int, alloc_idx=None) -> List[RankedNode]:
        """pe_place_csi_full: PlaceCSI for a group that runs full passes (node
        affinities, spreads, or a limit latched to MaxInt32 by a sibling group's
        Select). Arguments and records as PlaceCSI; on every other group the
        call is PlaceCSI."""
        out = (abi.pe_ranked_node * max(1, count))()
        placed = C.c_uint32(0)
        idx = None
        if alloc_idx is not None:
            if len(alloc_idx) != count:
                raise ValueError("alloc_idx needs one index per placement")
            idx = (C.c_uint32 * max(1, count))(*[int(i) for i in alloc_idx])
        self._check(self._lib.pe_place_csi_full(self._h, self._tg_index(tg), count, idx, out, C.byref(placed)))
        n = min(count, placed.value + 1)
        return [RankedNode.from_c(out[i], self.nodes, self._full_preempted(i, out[i])) for i in range(n)]

    def PlaceCSIMetrics(self, tg, count: int, alloc_idx=None) -> List[RankedNode]:
        """pe_place_csi_metrics: PlaceCSI with AllocMetric kept. The records are
        PlaceCSI's; with EnableMetrics on, PlaceCSIMaps() then gives each
        record's maps, the failed Select's included."""
        out = (abi.pe_ranked_node * max(1, count))()
        placed = C.c_uint32(0)
        idx = None
        if alloc_idx is not None:
            if len(alloc_idx) != count:
                raise ValueError("alloc_idx needs one index per placement")
            idx = (C.c_uint32 * max(1, count))(*[int(i) for i in alloc_idx])
        self._check(self._lib.pe_place_csi_metrics(self._h, self._tg_index(tg), count, idx, out, C.byref(placed)))
        n = min(count, placed.value + 1)
        return [RankedNode.from_c(out[i], self.nodes, self._full_preempted(i, out[i])) for i in range(n)]

    def PlaceCSIFullMetrics(self, tg, count: int, alloc_idx=None) -> List[RankedNode]:
        """pe_place_csi_full_metrics: PlaceCSIFull with AllocMetric kept. The
        records are PlaceCSIFull's; with EnableMetrics on, PlaceCSIMaps() then
        gives each record's maps, the failed Select's included. A group that
        runs no full passes: PlaceCSIMetrics; metrics off: PlaceCSIFull."""
        out = (abi.pe_ranked_node * max(1, count))()
        placed = C.c_uint32(0)
        idx = None
        if alloc_idx is not None:
            if len(alloc_idx) != count:
                raise ValueError("alloc_idx needs one index per placement")
            idx = (C.c_uint32 * max(1, count))(*[int(i) for i in alloc_idx])
        self._check(self._lib.pe_place_csi_full_metrics(self._h, self._tg_index(tg), count, idx, out,
                                                        C.byref(placed)))
        n = min(count, placed.value + 1)
        return [RankedNode.from_c(out[i], self.nodes, self._full_preempted(i, out[i])) for i in range(n)]

    def PlaceCSIMaps(self) -> List[Dict]:
        """pe_place_csi_maps: the maps of the last PlaceCSIMetrics' or
        PlaceCSIFullMetrics' records, one dict per record in LastMetrics' shape."""
        c, sc = C.POINTER(abi.pe_metric_count)(), C.POINTER(abi.pe_metric_score)()
        co, so, n = abi.u32p(), abi.u32p(), C.c_uint32(0)
        self._check(self._lib.pe_place_csi_maps(self._h, C.byref(c), C.byref(co), C.byref(sc), C.byref(so),
                                                C.byref(n)))
        return [decode_metrics(self, c, co[k], co[k + 1], sc, so[k], so[k + 1]) for k in range(n.value)]

    def place_csi_metrics_stats(self):
        """([loop, walk, trace, maps] in us by the host clock, trace log bytes) of the last PlaceCSIMetrics."""
        us, nb = (C.c_double * 4)(), C.c_uint64(0)
        self._check(self._lib.pe_place_csi_metrics_stats(self._h, us, C.byref(nb)))
        return [float(x) for x in us], int(nb.value)

    def csi_avail_launches(self) -> int:
        return int(self._lib.pe_csi_avail_launches(self._h))

    def csi_place_ms(self):
        """(k_csi_first, k_csi_loop) device ms of the last PlaceCSI, or (k_csi_first,
        k_csi_full) of the last PlaceCSIFull of a full-pass group; PE_CSI_TIME=1 only."""
        ms = (C.c_double * 2)()
        self._check(self._lib.pe_csi_place_ms(self._h, ms))
        return float(ms[0]), float(ms[1])

    def SetStateColumnar(self, cs):
        """Snapshot from a synth_columnar.ColumnarState (no per-node Python objects)."""
        self.nodes = None
        self.state = cs
        t = cs.strtab()
        self._check(self._fn("set_state")(self._h, C.byref(t), C.byref(cs.node_table), C.byref(cs.alloc_table)))
        return cs

    def UpdateAllocs(self, allocs: Sequence[Allocation], index: Optional[Sequence[int]] = None):
        """State delta without a node reload (pe_update_allocs): allocs[i]
        replaces snapshot alloc index[i] (None / -1: appended)."""
        fn = self._fn("update_allocs")
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.pe_strtab), C.POINTER(abi.pe_alloc_table), abi.u32p]
        at = self.state.encode_alloc_table(allocs)
        idx = np.asarray([abi.PE_NONE if (index is None or index[i] is None or index[i] < 0) else index[i]
                          for i in range(len(allocs))] or [0], dtype=np.uint32)
        t = self.state.strtab()
        self._check(fn(self._h, C.byref(t), C.byref(at), idx.ctypes.data_as(abi.u32p)))
        self._job = None

    def UpdateNodes(self, nodes: Sequence[Node], index: Optional[Sequence[int]] = None):
        """Node upserts without a reload (pe_update_nodes): nodes[i] replaces
        snapshot row index[i] (None / -1: appended)."""
        fn = self._fn("update_nodes")
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.pe_strtab), C.POINTER(abi.pe_node_table), abi.u32p]
        nt, idx = self.state.update_nodes(nodes, index)
        if self.nodes is not None:
            self.nodes = list(self.state.nodes)
        t = self.state.strtab()
        self._check(fn(self._h, C.byref(t), C.byref(nt), idx.ctypes.data_as(abi.u32p)))
        self._job = None

    def ResetPlan(self):
        """New evaluation on the resident snapshot (fresh EvalContext)."""
        self._check(self._fn("reset_plan")(self._h))

    def row(self, node_or_id) -> int:
        nid = node_or_id if isinstance(node_or_id, str) else node_or_id.id
        return self.state.row_of[nid]

    # -- Stack interface -------------------------------------------------------
    def SetJob(self, job: Job):
        self.job = EncodedJob(job, self.state.interner)
        self._job = job
        t = self.job.strtab()
        self._check(self._fn("set_job")(self._h, C.byref(t), C.byref(self.job.job)))
        if self._p == "pe_":   # the groups' CSI requests follow the job (pe_set_csi_requests)
            for i, g in enumerate(job.task_groups):
                if g.csi_volumes:
                    reqs = encode_csi_requests(g.csi_volumes, self.state.interner)   # (sources interned with the job)
                    self._check(self._lib.pe_set_csi_requests(self._h, i, reqs, len(g.csi_volumes)))

    def SetNodes(self, nodes_in_visit_order) -> int:
        """`nodes_in_visit_order`: Node objects / IDs / rows, already shuffled."""
        if isinstance(nodes_in_visit_order, np.ndarray) and nodes_in_visit_order.dtype.kind in "iu":
            rows = np.ascontiguousarray(nodes_in_visit_order, dtype=np.uint32)
        else:
            rows = np.asarray([x if isinstance(x, (int, np.integer)) else self.row(x)
                               for x in nodes_in_visit_order], dtype=np.uint32)
        self._visit = rows
        lim = C.c_uint32(0)
        self._check(self._fn("set_nodes")(self._h, rows.ctypes.data_as(abi.u32p), len(rows), C.byref(lim)))
        self.limit = lim.value
        return self.limit

    def _tg_index(self, tg):
        if isinstance(tg, int):
            return tg
        for i, g in enumerate(self._job.task_groups):
            if g is tg or g.name == tg:
                return i
        raise KeyError(tg)

    def Select(self, tg, options: SelectOptions = None) -> Optional[RankedNode]:
        opts = abi.pe_select_options()
        keep = []
        if options is not None:
            if options.penalty_node_ids:
                pen = np.asarray([self.row(x) for x in options.penalty_node_ids], dtype=np.uint32)
                keep.append(pen)
                opts.penalty_rows, opts.penalty_count = pen.ctypes.data_as(abi.u32p), len(pen)
            if options.preferred_nodes:
                pref = np.asarray([self.row(x) for x in options.preferred_nodes], dtype=np.uint32)
                keep.append(pref)
                opts.preferred_rows, opts.preferred_count = pref.ctypes.data_as(abi.u32p), len(pref)
            opts.preempt = int(options.preempt)
        if options is not None and options.alloc_index is not None and self._p == "pe_":
            self._check(self._lib.pe_csi_alloc_index(self._h, self._tg_index(tg), int(options.alloc_index)))
        out = abi.pe_ranked_node()
        self._check(self._fn("select")(self._h, self._tg_index(tg), C.byref(opts), C.byref(out)))
        r = RankedNode.from_c(out, self.nodes, self._full_preempted(0, out))
        return r if r.row >= 0 else None

    def _full_preempted(self, record, r):
        """PreemptedAllocs of record `record` of the last call when the record
        holds more than PE_MAX_PREEMPT inline (else None)."""
        if r.n_preempted <= abi.PE_MAX_PREEMPT:
            return None
        buf = (C.c_uint32 * r.n_preempted)()
        n = self._fn("preempted_of")(self._h, record, buf, r.n_preempted)
        if n != r.n_preempted:
            raise RuntimeError("preempted_of(%d) returned %d for %d allocs" % (record, n, r.n_preempted))
        return list(buf)

    def SelectRaw(self, tg, options: SelectOptions = None) -> RankedNode:
        """Select, but also returns the metrics when no node was found."""
        out = abi.pe_ranked_node()
        opts = abi.pe_select_options()
        if options is not None:
            opts.preempt = int(options.preempt)
        self._check(self._fn("select")(self._h, self._tg_index(tg), C.byref(opts), C.byref(out)))
        return RankedNode.from_c(out, self.nodes, self._full_preempted(0, out))

    def Commit(self, tg, node_or_row, preempted: Sequence[int] = ()):
        """Plan.AppendAlloc (+ AppendPreemptedAlloc of `preempted` alloc-table rows)."""
        row = node_or_row if isinstance(node_or_row, (int, np.integer)) else self.row(node_or_row)
        if len(preempted):
            pre = np.asarray(preempted, dtype=np.uint32)
            self._check(self._fn("commit_preempt")(self._h, self._tg_index(tg), int(row),
                                                   pre.ctypes.data_as(abi.u32p), len(pre)))
        else:
            self._check(self._fn("commit")(self._h, self._tg_index(tg), int(row)))

    def StopAllocs(self, allocs: Sequence[int]):
        """Plan.AppendStoppedAlloc of snapshot allocs (alloc-table rows)."""
        a = np.ascontiguousarray(np.asarray(list(allocs) or [0], dtype=np.uint32))
        self._check(self._fn("plan_stop")(self._h, a.ctypes.data_as(abi.u32p), len(allocs)))

    def PopUpdate(self, alloc: int):
        """Plan.PopUpdate of a snapshot alloc (alloc-table row)."""
        self._check(self._fn("plan_pop_update")(self._h, int(alloc)))

    def InplaceUpdate(self, tg, allocs: Sequence[int], fallback: bool = True):
        """inplaceUpdate (util.go:692-806) of snapshot allocs (alloc-table rows)
        against task group `tg`, in list order, in one call (pe_inplace_update).
        Returns (records, status): records[i] the RankedNode of update i's
        Select or None, status[i] 0 updated in place / 1 filtered / 2 exhausted.
        The node list is unspecified afterwards: SetNodes before the next Select.
        A job the batched path refuses (Unsupported) is answered by
        inplace_update_by_select when `fallback`, else the refusal propagates."""
        allocs = [int(a) for a in allocs]
        try:
            if not hasattr(self._lib, self._p + "inplace_update"):
                raise Unsupported(abi.PE_EUNSUPPORTED, "no batched in-place update behind this ABI")
            n = len(allocs)
            a = np.ascontiguousarray(np.asarray(allocs or [0], dtype=np.uint32))
            out = (abi.pe_ranked_node * max(1, n))()
            status = np.zeros(max(1, n), dtype=np.uint8)
            updated = C.c_uint32(0)
            self._check(self._fn("inplace_update")(self._h, self._tg_index(tg), a.ctypes.data_as(abi.u32p), n, out,
                                                   status.ctypes.data_as(abi.u8p), C.byref(updated)))
        except Unsupported:
            if not fallback:
                raise
            return inplace_update_by_select(self, tg, allocs)
        records = [RankedNode.from_c(out[i], self.nodes) if status[i] == 0 else None for i in range(n)]
        assert updated.value == sum(1 for r in records if r is not None)
        return records, [int(x) for x in status[:n]]

    def InplaceUpdateMetrics(self, tg, allocs: Sequence[int], fallback: bool = True):
        """InplaceUpdate / InplaceUpdatePreempt for a caller that keeps
        AllocMetric (pe_inplace_update_metrics): it runs with EnableMetrics on,
        on a generic stack, a system stack, or a system stack with preemption
        enabled. Returns (records, status, metrics): the first two are
        InplaceUpdatePreempt's, metrics[i] is what LastMetrics() gives after
        update i's Select in the per-call sequence (at most one key per map,
        or one ScoreMetaData item). With metrics off the call is
        InplaceUpdatePreempt and `metrics` is None. A job the call refuses
        (Unsupported) is answered by inplace_update_metrics_by_select when
        `fallback` (inplace_update_by_select with metrics off)."""
        allocs = [int(a) for a in allocs]
        on = getattr(self, "_metrics_on", False)
        try:
            if not hasattr(self._lib, self._p + "inplace_update_metrics"):
                raise Unsupported(abi.PE_EUNSUPPORTED, "no batched in-place update with AllocMetric behind this ABI")
            n = len(allocs)
            a = np.ascontiguousarray(np.asarray(allocs or [0], dtype=np.uint32))
            out = (abi.pe_ranked_node * max(1, n))()
            status = np.zeros(max(1, n), dtype=np.uint8)
            updated = C.c_uint32(0)
            self._check(self._fn("inplace_update_metrics")(self._h, self._tg_index(tg), a.ctypes.data_as(abi.u32p), n,
                                                           out, status.ctypes.data_as(abi.u8p), C.byref(updated)))
        except Unsupported:
            if not fallback:
                raise
            if on:
                return inplace_update_metrics_by_select(self, tg, allocs)
            return inplace_update_by_select(self, tg, allocs) + (None,)
        full = SystemStack.InplaceUpdatePreempted(self)
        records = [RankedNode.from_c(out[i], self.nodes, full.get(i)) if status[i] == 0 else None for i in range(n)]
        assert updated.value == sum(1 for r in records if r is not None)
        return records, [int(x) for x in status[:n]], (self.InplaceMetrics(status[:n]) if on else None)

    def InplaceUpdateSpread(self, tg, allocs: Sequence[int], fallback: bool = True):
        """InplaceUpdateMetrics for a job that may carry spread stanzas, at job
        or group level (pe_inplace_update_spread): the most general in-place
        call. Returns (records, status, metrics) in InplaceUpdateMetrics'
        shape; the records' scores and the maps' ScoreMetaData carry the
        allocation-spread part as each update's Select computes it in the
        per-call sequence. On a job without spreads the call is
        InplaceUpdateMetrics. A job the call refuses (Unsupported:
        distinct_property, reserved cores, static ports, ...) is answered by
        inplace_update_metrics_by_select when `fallback`
        (inplace_update_by_select with metrics off)."""
        allocs = [int(a) for a in allocs]
        on = getattr(self, "_metrics_on", False)
        try:
            if not hasattr(self._lib, self._p + "inplace_update_spread"):
                raise Unsupported(abi.PE_EUNSUPPORTED, "no batched in-place update with spreads behind this ABI")
            n = len(allocs)
            a = np.ascontiguousarray(np.asarray(allocs or [0], dtype=np.uint32))
            out = (abi.pe_ranked_node * max(1, n))()
            status = np.zeros(max(1, n), dtype=np.uint8)
            updated = C.c_uint32(0)
            self._check(self._fn("inplace_update_spread")(self._h, self._tg_index(tg), a.ctypes.data_as(abi.u32p), n,
                                                          out, status.ctypes.data_as(abi.u8p), C.byref(updated)))
        except Unsupported:
            if not fallback:
                raise
            if on:
                return inplace_update_metrics_by_select(self, tg, allocs)
            return inplace_update_by_select(self, tg, allocs) + (None,)
        full = SystemStack.InplaceUpdatePreempted(self)
        records = [RankedNode.from_c(out[i], self.nodes, full.get(i)) if status[i] == 0 else None for i in range(n)]
        assert updated.value == sum(1 for r in records if r is not None)
        return records, [int(x) for x in status[:n]], (self.InplaceMetrics(status[:n]) if on else None)

    def InplaceUpdateCSI(self, tg, allocs: Sequence[int], alloc_idx: Optional[Sequence[int]] = None,
                         fallback: bool = True):
        """InplaceUpdateSpread for a group that may carry CSI volume requests
        (pe_inplace_update_csi): the in-place call for every group.
        `alloc_idx[i]` is the name index of allocs[i], which per_alloc sources
        take as their suffix for that update; None: the index CSIAllocIndex
        holds. Returns (records, status, metrics) in InplaceUpdateSpread's
        shape; an update whose node passes the job and group checks and is
        unavailable for its volumes has status 1 and, with EnableMetrics on,
        the CSI checker's reason. On a group without CSI requests the call is
        InplaceUpdateSpread. A job the call refuses (Unsupported) is answered
        by inplace_update_csi_by_select when `fallback`: the per-alloc
        sequence with CSIAllocIndex before each Select (which, for a CSI group
        with EnableMetrics on, Select itself refuses)."""
        allocs = [int(a) for a in allocs]
        n = len(allocs)
        if alloc_idx is not None:
            alloc_idx = [int(i) for i in alloc_idx]
            if len(alloc_idx) != n:
                raise ValueError("alloc_idx needs one index per listed alloc")
        on = getattr(self, "_metrics_on", False)
        try:
            if not hasattr(self._lib, self._p + "inplace_update_csi"):
                raise Unsupported(abi.PE_EUNSUPPORTED, "no batched in-place update with CSI volumes behind this ABI")
            a = np.ascontiguousarray(np.asarray(allocs or [0], dtype=np.uint32))
            idx = None
            if alloc_idx is not None:
                idx = np.ascontiguousarray(np.asarray(alloc_idx or [0], dtype=np.uint32))
            out = (abi.pe_ranked_node * max(1, n))()
            status = np.zeros(max(1, n), dtype=np.uint8)
            updated = C.c_uint32(0)
            self._check(self._fn("inplace_update_csi")(self._h, self._tg_index(tg), a.ctypes.data_as(abi.u32p),
                                                       None if idx is None else idx.ctypes.data_as(abi.u32p), n,
                                                       out, status.ctypes.data_as(abi.u8p), C.byref(updated)))
        except Unsupported:
            if not fallback:
                raise
            return inplace_update_csi_by_select(self, tg, allocs, alloc_idx, metrics=on)
        full = SystemStack.InplaceUpdatePreempted(self)
        records = [RankedNode.from_c(out[i], self.nodes, full.get(i)) if status[i] == 0 else None for i in range(n)]
        assert updated.value == sum(1 for r in records if r is not None)
        return records, [int(x) for x in status[:n]], (self.InplaceMetrics(status[:n]) if on else None)

    def inplace_stage_ms(self):
        """HIP-event times (ms) of the last InplaceUpdate* call: (the walk, the
        spread stage; 0.0 when it did not run)."""
        buf = (C.c_double * 2)()
        self._check(self._lib.pe_inplace_spread_ms(self._h, C.cast(buf, abi.f64p)))
        return buf[0], buf[1]

    def InplaceMetrics(self, status=None) -> List[Dict]:
        """pe_inplace_metrics of the last InplaceUpdateMetrics: per update a
        dict in LastMetrics' shape. `status` (that call's, or None: taken from
        the entries, where an entry without any key reads as exhausted) tells
        the filtered maps from the exhausted ones. EngineError(PE_ESTATE) when
        that call ran with metrics off or an InplaceUpdate* call came since."""
        mp, sp = C.POINTER(abi.pe_inplace_metric)(), C.POINTER(abi.pe_metric_score)()
        n, ns = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.pe_inplace_metrics(self._h, C.byref(mp), C.byref(n), C.byref(sp), C.byref(ns)))
        cache = getattr(self, "_mkey_cache", None)
        if cache is None:
            cache = self._mkey_cache = {}

        def text(key):
            if key not in cache:
                cache[key] = self.MetricString(key)
            return cache[key]

        out = []
        for i in range(n.value):
            e = mp[i]
            m = {v: {} for v in _KIND_NAMES.values()}
            m["ScoreMetaData"] = []
            if e.score != abi.PE_NONE:
                assert e.score < ns.value
                m["ScoreMetaData"] = decode_metrics(self, None, 0, 0, sp, e.score, e.score + 1)["ScoreMetaData"]
            else:
                if status is not None:
                    filtered = int(status[i]) == 1
                else:   # the reason keys of the two kinds never coincide: FilterNode's are checker reasons
                    filtered = e.reason_key != abi.PE_NONE and not _is_dimension(text(e.reason_key))
                if e.class_key != abi.PE_NONE:
                    m["ClassFiltered" if filtered else "ClassExhausted"][text(e.class_key)] = 1
                if e.reason_key != abi.PE_NONE:
                    m["ConstraintFiltered" if filtered else "DimensionExhausted"][text(e.reason_key)] = 1
            out.append(m)
        return out

    def Place(self, tg, count: int) -> List[RankedNode]:
        out = (abi.pe_ranked_node * max(1, count))()
        placed = C.c_uint32(0)
        self._check(self._fn("place")(self._h, self._tg_index(tg), count, out, C.byref(placed)))
        n = min(count, placed.value + 1)
        return [RankedNode.from_c(out[i], self.nodes, self._full_preempted(i, out[i])) for i in range(n)]

    def PlaceArrays(self, tg, count: int):
        """Fused count loop returning (rows, final_scores, placed, records) as numpy
        arrays. The record buffer is reused across calls with the same count."""
        cache = getattr(self, "_place_buf", None)
        if cache is None or cache[0] != count:
            out = (abi.pe_ranked_node * max(1, count))()
            cache = (count, out, np.ctypeslib.as_array(out), C.c_uint32(0))
            self._place_buf = cache
        _, out, arr, placed = cache
        self._check(self._fn("place")(self._h, self._tg_index(tg), count, out, C.byref(placed)))
        return arr["row"].copy(), arr["final_score"].copy(), placed.value, arr

    def SystemPlaceView(self, tg):
        """SystemPlace with the results left in the engine's page-locked
        staging (pe_system_place with null arrays + pe_system_results): numpy
        views valid until the next SystemPlace on this stack, no copy."""
        placed = C.c_uint32(0)
        self._check(self._fn("system_place")(self._h, self._tg_index(tg), None, None, C.byref(placed)))
        lib = self._lib
        lib.pe_system_results.restype = C.c_int
        lib.pe_system_results.argtypes = [C.c_void_p, C.POINTER(abi.f64p), C.POINTER(abi.u8p), abi.u32p]
        sc, st, n = abi.f64p(), abi.u8p(), C.c_uint32(0)
        self._check(lib.pe_system_results(self._h, C.byref(sc), C.byref(st), C.byref(n)))
        if n.value == 0:
            return np.empty(0), np.empty(0, dtype=np.uint8), placed.value
        return (np.ctypeslib.as_array(sc, shape=(n.value,)), np.ctypeslib.as_array(st, shape=(n.value,)),
                placed.value)

    def SystemPlace(self, tg):
        n = len(self._visit)
        score = np.empty(max(1, n), dtype=np.float64)
        status = np.empty(max(1, n), dtype=np.uint8)
        placed = C.c_uint32(0)
        self._check(self._fn("system_place")(self._h, self._tg_index(tg), score.ctypes.data_as(abi.f64p),
                                             status.ctypes.data_as(abi.u8p), C.byref(placed)))
        return score[:n], status[:n], placed.value

    def SystemPlaceGroups(self, tgs, fallback: bool = True, staged: bool = False):
        """SystemScheduler.computePlacements for several task groups of a
        system job in one pass (pe_system_place_groups): every position of the
        SetNodes list in order and, within it, every group of `tgs` in list
        order. Returns (score[n, G], status[n, G], counts[G, 3], placed):
        FinalScore or NaN where nothing was placed, pe_system_place's codes,
        the entries of each group per code. The arrays are copies (nothing
        points into the engine's staging). `staged`: the call leaves the
        results in the staging (null arrays) and they are copied from
        pe_system_groups_results. A job the pass refuses (Unsupported), or a
        library without the entry point, is answered by
        system_place_groups_by_select when `fallback`."""
        return self._system_place_groups(tgs, fallback, staged, "system_place_groups")[:4]

    def SystemPlaceGroupsPreempt(self, tgs, fallback: bool = True, staged: bool = False):
        """SystemPlaceGroups on a stack with preemption enabled
        (pe_system_place_groups_preempt): a pair whose plain fit is exhausted
        goes through BinPack with evict, and a pair placed by eviction counts
        as placed with the eviction Select's FinalScore. Returns
        (score[n, G], status[n, G], counts[G, 3], placed, preempted), where
        `preempted` is {(pos, k): [alloc-table rows]} for every entry that
        preempted something (pe_system_groups_preempted; no PE_MAX_PREEMPT
        cap). The fallback is system_place_groups_preempt_by_select; it is the
        stack's own Select in a loop, so it raises Unsupported itself for a job
        or snapshot that Select refuses where it would evict (reserved cores,
        allocs outside the on-device eviction limits, an alloc holding one
        device group twice, several task networks)."""
        return self._system_place_groups(tgs, fallback, staged, "system_place_groups_preempt")

    def SystemPlaceGroupsMetrics(self, tgs, fallback: bool = True, staged: bool = False):
        """SystemPlaceGroupsPreempt for a caller that keeps AllocMetric
        (pe_system_place_groups_metrics): it runs with EnableMetrics on, on a
        preempting or a non-preempting system stack. Returns
        SystemPlaceGroupsPreempt's five results and a `metrics` dict with what
        computePlacements keeps of the Selects' maps:
        {"failed": {k: (pos, dimension, node class)}, "scores": {(pos, k):
        {"binpack": x, "devices": y}}}. `failed[k]` is the first exhausted
        Select of listed group k in walk order, with the one key of its
        DimensionExhausted and of its ClassExhausted (None where that Select
        recorded none); a group without an exhausted entry has no item.
        `scores` holds the named scores of the placed entries of the one group
        whose ask scores devices (the other groups' only score is "binpack",
        equal to the FinalScore). With metrics off the call is
        SystemPlaceGroupsPreempt and both maps are empty. The fallback is
        system_place_groups_metrics_by_select."""
        return self._system_place_groups(tgs, fallback, staged, "system_place_groups_metrics")

    def SystemGroupsMetrics(self, n_tg: int) -> Dict:
        """pe_system_groups_metrics of the last SystemPlaceGroupsMetrics over
        `n_tg` groups, in its `metrics` shape. EngineError(PE_ESTATE) when that
        call ran with metrics off or a pe_system_place* call came since."""
        fl = C.POINTER(abi.pe_sysg_failure)()
        dg, bp, dv, nn = C.c_int32(-1), abi.f64p(), abi.f64p(), C.c_uint32(0)
        self._check(self._lib.pe_system_groups_metrics(self._h, C.byref(fl), C.byref(dg), C.byref(bp), C.byref(dv),
                                                       C.byref(nn)))
        cache = getattr(self, "_mkey_cache", None)
        if cache is None:
            cache = self._mkey_cache = {}

        def text(key):
            if key == abi.PE_NONE:
                return None
            if key not in cache:
                cache[key] = self.MetricString(key)
            return cache[key]

        failed, scores = {}, {}
        for k in range(n_tg):
            f = fl[k]
            if f.pos != abi.PE_NONE:
                failed[k] = (int(f.pos), text(f.dimension), text(f.node_class))
        if dg.value >= 0 and nn.value:
            b = np.ctypeslib.as_array(bp, shape=(nn.value,))
            d = np.ctypeslib.as_array(dv, shape=(nn.value,))
            for pos in np.flatnonzero(~np.isnan(b)):
                scores[(int(pos), int(dg.value))] = {"binpack": float(b[pos]), "devices": float(d[pos])}
        return {"failed": failed, "scores": scores}

    def _system_place_groups(self, tgs, fallback, staged, name):
        idx = [self._tg_index(t) for t in tgs]
        n, G = len(self._visit), len(idx)
        try:
            if not hasattr(self._lib, self._p + name):
                raise Unsupported(abi.PE_EUNSUPPORTED, "no %s behind this ABI" % name)
            fn = getattr(self._lib, self._p + name)
            t = np.ascontiguousarray(np.asarray(idx or [0], dtype=np.uint32))
            placed = C.c_uint32(0)
            E = n * G
            if staged:
                self._check(fn(self._h, t.ctypes.data_as(abi.u32p), G, None, None, None, C.byref(placed)))
                sc, st, cn = abi.f64p(), abi.u8p(), abi.u32p()
                rn, rg, rp = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
                self._check(self._lib.pe_system_groups_results(self._h, C.byref(sc), C.byref(st), C.byref(cn),
                                                               C.byref(rn), C.byref(rg), C.byref(rp)))
                assert (rn.value, rg.value, rp.value) == (n, G, placed.value)
                p = placed.value
                dense = np.ctypeslib.as_array(sc, shape=(p,)).copy() if p else np.empty(0)
                packed = np.ctypeslib.as_array(st, shape=((E + 3) // 4,)).copy() if E else np.empty(0, np.uint8)
                counts = np.ctypeslib.as_array(cn, shape=(3 * G,)).copy()
            else:
                dense = np.empty(max(1, E), dtype=np.float64)
                packed = np.zeros(max(1, (E + 3) // 4), dtype=np.uint8)
                counts = np.zeros(3 * max(1, G), dtype=np.uint32)
                self._check(fn(self._h, t.ctypes.data_as(abi.u32p), G, dense.ctypes.data_as(abi.f64p),
                               packed.ctypes.data_as(abi.u8p), counts.ctypes.data_as(abi.u32p), C.byref(placed)))
                counts = counts[:3 * G]
        except Unsupported:
            if not fallback:
                raise
            if name == "system_place_groups_metrics":
                if getattr(self, "_metrics_on", False):
                    return system_place_groups_metrics_by_select(self, idx)
                return system_place_groups_preempt_by_select(self, idx) + ({"failed": {}, "scores": {}},)
            return system_place_groups_preempt_by_select(self, idx)
        p = placed.value
        status = unpack_status2(packed, E)
        score = np.full(E, np.nan)
        score[status == 0] = dense[:p]
        preempted = {}
        if name != "system_place_groups":
            en, of, al = abi.u32p(), abi.u32p(), abi.u32p()
            ne = C.c_uint32(0)
            self._check(self._lib.pe_system_groups_preempted(self._h, C.byref(en), C.byref(of), C.byref(al),
                                                             C.byref(ne)))
            if ne.value:
                offs = np.ctypeslib.as_array(of, shape=(ne.value + 1,)).copy()
                preempted = preempted_from_csr(np.ctypeslib.as_array(en, shape=(ne.value,)).copy(), offs,
                                               np.ctypeslib.as_array(al, shape=(int(offs[-1]),)).copy(), G)
        out = (score.reshape(n, G), status.reshape(n, G), counts.reshape(G, 3).astype(np.uint32), p, preempted)
        if name == "system_place_groups_metrics":
            on = getattr(self, "_metrics_on", False)
            out += (self.SystemGroupsMetrics(G) if on else {"failed": {}, "scores": {}},)
        return out


def pack_status2(status) -> np.ndarray:
    """Outcome codes (0 placed, 1 filtered, 2 exhausted) packed as
    pe_system_place_groups returns them: 2 bits per entry, entry e in byte
    e >> 2 at bits 2 * (e & 3), unused bits of the last byte 0."""
    st = np.asarray(status, dtype=np.uint8).ravel()
    pad = np.zeros(4 * ((len(st) + 3) // 4), dtype=np.uint8)
    pad[:len(st)] = st & 3
    q = pad.reshape(-1, 4)
    return (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8)


def unpack_status2(packed, n: int) -> np.ndarray:
    """The first `n` outcome codes of a pack_status2 array."""
    b = np.asarray(packed, dtype=np.uint8).ravel()[:(n + 3) // 4]
    out = np.empty((len(b), 4), dtype=np.uint8)
    for j in range(4):
        out[:, j] = (b >> (2 * j)) & 3
    return out.ravel()[:n].copy()


def system_place_groups_by_select(stack, tgs):
    """SystemScheduler.computePlacements' loop (scheduler_system.go:283-425)
    for several task groups as the per-call sequence, on any stack with
    SetNodes / SelectRaw / Commit (the engine's and the oracle's): for each
    position of the SetNodes list, for each group of `tgs` in list order,
    SetNodes([row]), Select(tg) and Commit on an option. SelectRaw keeps a nil
    Select's counters, which tell filtered from exhausted. Returns
    SystemPlaceGroups' shape; the node list is put back at the end."""
    return system_place_groups_preempt_by_select(stack, tgs)[:4]


def preempted_from_csr(entries, off, allocs, n_tg: int) -> Dict:
    """pe_system_groups_preempted's CSR as {(pos, k): [alloc-table rows]}:
    entry e = pos * n_tg + k, its allocs in allocs[off[i]:off[i + 1]]."""
    out = {}
    for i, e in enumerate(entries):
        out[(int(e) // n_tg, int(e) % n_tg)] = [int(a) for a in allocs[int(off[i]):int(off[i + 1])]]
    return out


def inplace_preempted_from_csr(updates, off, allocs) -> Dict:
    """pe_inplace_update_preempted's CSR as {list position: [alloc-table rows]}:
    update updates[i] preempted allocs[off[i]:off[i + 1]]."""
    out = {}
    for i, u in enumerate(updates):
        out[int(u)] = [int(a) for a in allocs[int(off[i]):int(off[i + 1])]]
    return out


def system_place_groups_preempt_by_select(stack, tgs):
    """system_place_groups_by_select's loop, which on a stack with preemption
    enabled evicts where the plain fit is exhausted (the Select's record
    carries the PreemptedAllocs, Commit appends them to the plan). Returns
    SystemPlaceGroupsPreempt's shape: the four results and
    {(pos, k): [alloc-table rows]} for every entry that preempted something."""
    rows = np.array(stack._visit, dtype=np.uint32, copy=True)
    n, G = len(rows), len(tgs)
    score = np.full((n, G), np.nan)
    status = np.zeros((n, G), dtype=np.uint8)
    counts = np.zeros((G, 3), dtype=np.uint32)
    preempted = {}
    for pos in range(n):
        one = rows[pos:pos + 1]
        for k, tg in enumerate(tgs):
            stack.SetNodes(one)
            r = stack.SelectRaw(tg)
            if r.row >= 0:
                stack.Commit(tg, r.row, r.preempted)   # with the evictions of a preempting stack
                score[pos, k] = r.final_score
                if len(r.preempted):
                    # increasing alloc-table row, as pe_system_groups_preempted lists them (the
                    # slots of a node are in table order; the reference's order is Go map order)
                    preempted[(pos, k)] = sorted(int(a) for a in r.preempted)
            else:
                status[pos, k] = 1 if r.nodes_filtered else 2
            counts[k, status[pos, k]] += 1
    stack.SetNodes(rows)
    return score, status, counts, int(counts[:, 0].sum()), preempted


def system_place_groups_metrics_by_select(stack, tgs):
    """system_place_groups_preempt_by_select's loop on a stack with
    EnableMetrics on (the engine's or the oracle's), keeping of each Select's
    maps what SystemScheduler.computePlacements keeps
    (scheduler_system.go:311-382): after a group's first exhausted Select the
    one key of DimensionExhausted and of ClassExhausted, after a placed one the
    node's ScoreMetaData scores. Returns SystemPlaceGroupsMetrics' shape; here
    `scores` has an item for every placed entry."""
    rows = np.array(stack._visit, dtype=np.uint32, copy=True)
    n, G = len(rows), len(tgs)
    score = np.full((n, G), np.nan)
    status = np.zeros((n, G), dtype=np.uint8)
    counts = np.zeros((G, 3), dtype=np.uint32)
    preempted, failed, scores = {}, {}, {}

    def only(m):
        assert len(m) <= 1, m
        return next(iter(m), None)

    for pos in range(n):
        one = rows[pos:pos + 1]
        for k, tg in enumerate(tgs):
            stack.SetNodes(one)
            r = stack.SelectRaw(tg)
            if r.row >= 0:
                meta = stack.LastMetrics()["ScoreMetaData"]
                assert len(meta) == 1, meta
                scores[(pos, k)] = dict(meta[0][2])
                stack.Commit(tg, r.row, r.preempted)
                score[pos, k] = r.final_score
                if len(r.preempted):
                    preempted[(pos, k)] = sorted(int(a) for a in r.preempted)
            else:
                status[pos, k] = 1 if r.nodes_filtered else 2
                if status[pos, k] == 2 and k not in failed:
                    m = stack.LastMetrics()
                    failed[k] = (pos, only(m["DimensionExhausted"]), only(m["ClassExhausted"]))
            counts[k, status[pos, k]] += 1
    stack.SetNodes(rows)
    return score, status, counts, int(counts[:, 0].sum()), preempted, {"failed": failed, "scores": scores}


def inplace_update_by_select(stack, tg, allocs: Sequence[int]):
    """inplaceUpdate's loop (util.go:743-760) as the per-call sequence, on any
    stack with StopAllocs / SetNodes / SelectRaw / PopUpdate / Commit and the
    encoded state (the engine's and the oracle's): per alloc
    AppendStoppedAlloc, SetNodes([its node]), Select(tg), PopUpdate and, when
    the Select returned an option, the updated alloc in place of the old one
    (the stop again, then Commit). SelectRaw keeps a nil Select's counters,
    which tell filtered from exhausted. Returns (records, status) in
    InplaceUpdate's shape; the node list is left on the last alloc's node."""
    node_row = stack.state.alloc_table.node_row
    records, status = [], []
    for ai in allocs:
        ai = int(ai)
        row = int(node_row[ai])
        stack.StopAllocs([ai])
        stack.SetNodes(np.asarray([row], dtype=np.uint32))
        r = stack.SelectRaw(tg)
        stack.PopUpdate(ai)
        if r.row >= 0:
            stack.StopAllocs([ai])        # the in-place alloc replaces the old one (same ID)
            stack.Commit(tg, r.row)
            records.append(r)
            status.append(0)
        else:
            records.append(None)
            status.append(1 if r.nodes_filtered else 2)
    return records, status


def place_destructive_by_select(stack, tg, allocs: Sequence[int]):
    """computePlacements' destructive-update loop (generic_sched.go:543-645) as
    the per-call sequence, on any stack with StopAllocs / SelectRaw / Commit /
    PopUpdate (the engine's and the oracle's): per update
    AppendStoppedAlloc(prev), Select(tg) on the current list from the current
    cursor, AppendAlloc on an option; on nil PopUpdate(prev) and the loop ends.
    SelectRaw keeps the nil Select's counters. Returns the records in
    PlaceDestructive's shape: the placements, then the nil record if any."""
    records = []
    for ai in allocs:
        ai = int(ai)
        stack.StopAllocs([ai])
        r = stack.SelectRaw(tg)
        records.append(r)
        if r.row < 0:
            stack.PopUpdate(ai)
            break
        stack.Commit(tg, r.row)
    return records


def place_destructive_metrics_by_select(stack, tg, allocs: Sequence[int]):
    """place_destructive_by_select on a stack with EnableMetrics on (the
    engine's or the oracle's), with LastMetrics() read after each SelectRaw,
    before PopUpdate / Commit: what computePlacements stores on the new alloc,
    or in failedTGAllocs for the nil Select (generic_sched.go:552-645). Returns
    (records, maps) in PlaceDestructiveMetrics' shape."""
    records, maps = [], []
    for ai in allocs:
        ai = int(ai)
        stack.StopAllocs([ai])
        r = stack.SelectRaw(tg)
        records.append(r)
        maps.append(stack.LastMetrics())
        if r.row < 0:
            stack.PopUpdate(ai)
            break
        stack.Commit(tg, r.row)
    return records, maps


def _is_dimension(reason: str) -> bool:
    """Whether an AllocMetric reason is one ExhaustedNode records
    (rank.go:255-497: a network or devices message, or AllocsFit's dimension)."""
    return reason in ("cpu", "memory", "disk", "cores") or reason.startswith(("network: ", "devices: "))


def inplace_update_metrics_by_select(stack, tg, allocs: Sequence[int]):
    """inplace_update_by_select on a stack with EnableMetrics on (the engine's
    or the oracle's), with LastMetrics() read after each update's Select,
    before PopUpdate: what inplaceUpdate keeps as newAlloc.Metrics
    (util.go:801). Returns (records, status, metrics) in InplaceUpdateMetrics'
    shape; the node list is left on the last alloc's node."""
    node_row = stack.state.alloc_table.node_row
    records, status, metrics = [], [], []
    for ai in allocs:
        ai = int(ai)
        row = int(node_row[ai])
        stack.StopAllocs([ai])
        stack.SetNodes(np.asarray([row], dtype=np.uint32))
        r = stack.SelectRaw(tg)
        metrics.append(stack.LastMetrics())
        stack.PopUpdate(ai)
        if r.row >= 0:
            stack.StopAllocs([ai])        # the in-place alloc replaces the old one (same ID)
            stack.Commit(tg, r.row)
            records.append(r)
            status.append(0)
        else:
            records.append(None)
            status.append(1 if r.nodes_filtered else 2)
    return records, status, metrics


def inplace_update_csi_by_select(stack, tg, allocs: Sequence[int], alloc_idx: Optional[Sequence[int]] = None,
                                 metrics: bool = False):
    """inplace_update_by_select for a group with CSI volume requests: the
    update's name index goes to the checker (CSIAllocIndex, SetVolumes with the
    alloc's name) before its Select. `metrics`: LastMetrics() after each
    Select, as inplace_update_metrics_by_select reads it. Returns (records,
    status, metrics or None) in InplaceUpdateCSI's shape."""
    node_row = stack.state.alloc_table.node_row
    records, status, maps = [], [], []
    for i, ai in enumerate(allocs):
        ai = int(ai)
        row = int(node_row[ai])
        stack.StopAllocs([ai])
        stack.SetNodes(np.asarray([row], dtype=np.uint32))
        if alloc_idx is not None:
            stack.CSIAllocIndex(tg, int(alloc_idx[i]))
        r = stack.SelectRaw(tg)
        if metrics:
            maps.append(stack.LastMetrics())
        stack.PopUpdate(ai)
        if r.row >= 0:
            stack.StopAllocs([ai])        # the in-place alloc replaces the old one (same ID)
            stack.Commit(tg, r.row)
            records.append(r)
            status.append(0)
        else:
            records.append(None)
            status.append(1 if r.nodes_filtered else 2)
    return records, status, (maps if metrics else None)


class GenericStack(_Stack):
    """NewGenericStack (stack.go:336-431) on the MI355X engine."""
    stack_kind = abi.PE_STACK_GENERIC

    def __init__(self, batch: bool = False, config: SchedulerConfig = None, device: int = 0,
                 devices: Optional[Sequence[int]] = None):
        super().__init__(load_engine(), "pe_", batch, config, device, devices)

    def PlaceDestructive(self, tg, allocs: Sequence[int], fallback: bool = True) -> List[RankedNode]:
        """computePlacements' destructive-update loop (generic_sched.go:543-645)
        for the previous allocs `allocs` (alloc-table rows) of task group `tg`
        in one call (pe_place_destructive): per update AppendStoppedAlloc, a
        plain Select, AppendAlloc; a nil Select pops its stop and ends the loop.
        Returns the records as Place does: the placements and, when the loop
        ended early, the nil Select's record (row -1). Updates with penalty or
        preferred nodes go through the per-call sequence. A job the batched
        path refuses (Unsupported) is answered by place_destructive_by_select
        when `fallback`, else the refusal propagates."""
        allocs = [int(a) for a in allocs]
        n = len(allocs)
        try:
            if not hasattr(self._lib, "pe_place_destructive"):
                raise Unsupported(abi.PE_EUNSUPPORTED, "no batched destructive update behind this ABI")
            a = np.ascontiguousarray(np.asarray(allocs or [0], dtype=np.uint32))
            out = (abi.pe_ranked_node * max(1, n))()
            placed = C.c_uint32(0)
            self._check(self._lib.pe_place_destructive(self._h, self._tg_index(tg), a.ctypes.data_as(abi.u32p), n, out,
                                                       C.byref(placed)))
        except Unsupported:
            if not fallback:
                raise
            return place_destructive_by_select(self, tg, allocs)
        return [RankedNode.from_c(out[i], self.nodes) for i in range(min(n, placed.value + 1))]

    def PlaceDestructiveFull(self, tg, allocs: Sequence[int], fallback: bool = True) -> List[RankedNode]:
        """pe_place_destructive_full: PlaceDestructive for a task group that
        runs full passes (node affinities, spreads, or a limit a sibling
        group's Select latched to MaxInt32); on any other group the call is
        PlaceDestructive's. Records in PlaceDestructive's shape. A job the
        batched path refuses (Unsupported) is answered by
        place_destructive_by_select when `fallback`, else the refusal
        propagates."""
        allocs = [int(a) for a in allocs]
        n = len(allocs)
        try:
            if not hasattr(self._lib, "pe_place_destructive_full"):
                raise Unsupported(abi.PE_EUNSUPPORTED, "no batched full-pass destructive update behind this ABI")
            a = np.ascontiguousarray(np.asarray(allocs or [0], dtype=np.uint32))
            out = (abi.pe_ranked_node * max(1, n))()
            placed = C.c_uint32(0)
            self._check(self._lib.pe_place_destructive_full(self._h, self._tg_index(tg), a.ctypes.data_as(abi.u32p), n,
                                                            out, C.byref(placed)))
        except Unsupported:
            if not fallback:
                raise
            return place_destructive_by_select(self, tg, allocs)
        return [RankedNode.from_c(out[i], self.nodes) for i in range(min(n, placed.value + 1))]

    def PlaceDestructiveMetrics(self, tg, allocs: Sequence[int], fallback: bool = True):
        """pe_place_destructive_metrics: PlaceDestructive with AllocMetric kept.
        Returns (records, maps): PlaceDestructive's records and, with
        EnableMetrics on, one dict per record in LastMetrics' shape, the nil
        Select's included (metrics off: PlaceDestructive's records and None).
        A job the batched path refuses (Unsupported) is answered by
        place_destructive_metrics_by_select when `fallback`, else the refusal
        propagates."""
        allocs = [int(a) for a in allocs]
        n = len(allocs)
        try:
            if not hasattr(self._lib, "pe_place_destructive_metrics"):
                raise Unsupported(abi.PE_EUNSUPPORTED, "no batched destructive update with metrics behind this ABI")
            a = np.ascontiguousarray(np.asarray(allocs or [0], dtype=np.uint32))
            out = (abi.pe_ranked_node * max(1, n))()
            placed = C.c_uint32(0)
            self._check(self._lib.pe_place_destructive_metrics(self._h, self._tg_index(tg), a.ctypes.data_as(abi.u32p),
                                                               n, out, C.byref(placed)))
        except Unsupported:
            if not fallback:
                raise
            if not getattr(self, "_metrics_on", False):
                return place_destructive_by_select(self, tg, allocs), None
            return place_destructive_metrics_by_select(self, tg, allocs)
        records = [RankedNode.from_c(out[i], self.nodes) for i in range(min(n, placed.value + 1))]
        if not getattr(self, "_metrics_on", False):
            return records, None
        return records, (self.PlaceDestructiveMaps() if n else [])

    def PlaceDestructiveFullMetrics(self, tg, allocs: Sequence[int], fallback: bool = True):
        """pe_place_destructive_full_metrics: the one entry for every run of
        destructive updates of a caller that keeps AllocMetric. A full-pass
        group (node affinities, spreads, a latched limit) runs
        PlaceDestructiveFull's loop with its maps; any other group is
        PlaceDestructiveMetrics'; with EnableMetrics off the call is
        PlaceDestructiveFull's. Returns (records, maps) in
        PlaceDestructiveMetrics' shape (maps None with metrics off). A job the
        batched path refuses (Unsupported) is answered by
        place_destructive_metrics_by_select when `fallback`, else the refusal
        propagates."""
        allocs = [int(a) for a in allocs]
        n = len(allocs)
        try:
            if not hasattr(self._lib, "pe_place_destructive_full_metrics"):
                raise Unsupported(abi.PE_EUNSUPPORTED,
                                  "no batched full-pass destructive update with metrics behind this ABI")
            a = np.ascontiguousarray(np.asarray(allocs or [0], dtype=np.uint32))
            out = (abi.pe_ranked_node * max(1, n))()
            placed = C.c_uint32(0)
            self._check(self._lib.pe_place_destructive_full_metrics(self._h, self._tg_index(tg),
                                                                    a.ctypes.data_as(abi.u32p), n, out,
                                                                    C.byref(placed)))
        except Unsupported:
            if not fallback:
                raise
            if not getattr(self, "_metrics_on", False):
                return place_destructive_by_select(self, tg, allocs), None
            return place_destructive_metrics_by_select(self, tg, allocs)
        records = [RankedNode.from_c(out[i], self.nodes) for i in range(min(n, placed.value + 1))]
        if not getattr(self, "_metrics_on", False):
            return records, None
        return records, (self.PlaceDestructiveMaps() if n else [])

    def PlaceDestructiveMaps(self) -> List[Dict]:
        """pe_place_destructive_maps: the maps of the last
        PlaceDestructiveMetrics' or PlaceDestructiveFullMetrics' records, one dict per record in LastMetrics' shape."""
        c, sc = C.POINTER(abi.pe_metric_count)(), C.POINTER(abi.pe_metric_score)()
        co, so, n = abi.u32p(), abi.u32p(), C.c_uint32(0)
        self._check(self._lib.pe_place_destructive_maps(self._h, C.byref(c), C.byref(co), C.byref(sc), C.byref(so),
                                                        C.byref(n)))
        return [decode_metrics(self, c, co[k], co[k + 1], sc, so[k], so[k + 1]) for k in range(n.value)]

    def place_destructive_stats(self):
        """(launches, synchronisations, uploads) of the last PlaceDestructive, PlaceDestructiveMetrics,
        PlaceDestructiveFull or PlaceDestructiveFullMetrics call."""
        out = (C.c_uint64 * 3)()
        self._check(self._lib.pe_place_destructive_stats(self._h, out))
        return tuple(int(x) for x in out)

    def StageOrders(self, orders: np.ndarray):
        """Stage E visit orders (E x n rows, each a shuffled SetNodes list) in HBM."""
        o = np.ascontiguousarray(np.asarray(orders, dtype=np.uint32))
        if o.ndim != 2:
            raise ValueError("orders must be 2-D (evals x nodes)")
        self._check(self._lib.pe_stage_orders(self._h, o.ctypes.data_as(abi.u32p), o.shape[0], o.shape[1]))
        self._staged = o.shape[0]

    _PLACEMENT = np.dtype([("row", "<i4"), ("nodes_evaluated", "<u4"), ("final_score", "<f8")])

    def PlaceBatch(self, tg, count: int, copy: bool = True):
        """Independent evaluations over the staged orders; returns (rows, scores, evaluated, placed).

        copy=False returns views of the engine's page-locked result buffer
        (valid until the next PlaceBatch) instead of copies."""
        self._check(self._lib.pe_place_batch(self._h, self._tg_index(tg), count, None, None))
        res = C.POINTER(abi.pe_placement)()
        status = abi.u32p()
        n_evals, cnt = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.pe_batch_results(self._h, C.byref(res), C.byref(status), C.byref(n_evals),
                                               C.byref(cnt)))
        E = n_evals.value
        total = E * count
        if total:
            raw = np.ctypeslib.as_array(C.cast(res, C.POINTER(C.c_uint8)), shape=(total * 16,))
            out = raw.view(self._PLACEMENT).reshape(E, count)
            st = np.ctypeslib.as_array(status, shape=(2 * E,))
            placed = st[0::2]
        else:
            out = np.zeros((E, count), dtype=self._PLACEMENT)
            placed = np.zeros(E, dtype=np.uint32)
        if copy:
            out = out.copy()
            placed = placed.copy()
        return out["row"], out["final_score"], out["nodes_evaluated"], placed

    def SelectShard(self, tg, row_begin: int, row_end: int) -> bytes:
        """This GPU's part of a full-pass Select: the 80-byte record of snapshot
        rows [row_begin, row_end) (pe_select_shard)."""
        rec = abi.pe_shard_rec()
        self._check(self._lib.pe_select_shard(self._h, self._tg_index(tg), row_begin, row_end, C.byref(rec)))
        return bytes(rec.bytes)

    def SelectMerge(self, tg, recs) -> RankedNode:
        """Resolve the Select from every shard's record (pe_select_merge)."""
        arr = (abi.pe_shard_rec * max(1, len(recs)))()
        for i, r in enumerate(recs):
            C.memmove(arr[i].bytes, bytes(r), 80)
        out = abi.pe_ranked_node()
        self._check(self._lib.pe_select_merge(self._h, self._tg_index(tg), arr, len(recs), C.byref(out)))
        return RankedNode.from_c(out, self.nodes)

    def CommInit(self, nranks: int, rank: int, unique_id: bytes):
        """Join the RCCL communicator of `nranks` engines (pe_comm_init); every
        rank passes the same 128-byte id (comm_unique_id on one rank)."""
        buf = np.frombuffer(bytes(unique_id), dtype=np.uint8).copy()
        self._check(self._lib.pe_comm_init(self._h, nranks, rank, buf.ctypes.data_as(abi.u8p)))

    def CommInitHost(self, nranks: int, rank: int, all_gather):
        """Join `nranks` engines over a caller transport (pe_comm_init_host):
        all_gather(record: bytes) -> list of nranks records in rank order, called
        once per placement of PlaceSharded (e.g. torch.distributed over gloo)."""
        def exchange(_ctx, send, recv, nbytes):
            try:
                recs = all_gather(C.string_at(send, nbytes))
                if len(recs) != nranks or any(len(r) != nbytes for r in recs):
                    return 2
                C.memmove(recv, b"".join(recs), nbytes * nranks)
                return 0
            except Exception:   # noqa: BLE001 - reported to the engine as a failed exchange
                return 1
        self._xfn = abi.pe_exchange_fn(exchange)   # kept alive with the handle
        self._check(self._lib.pe_comm_init_host(self._h, nranks, rank, self._xfn, None))

    def PlaceSharded(self, tg, count: int, row_begin: int, row_end: int) -> List[RankedNode]:
        """The full-pass count loop over the communicator's ranks, this rank
        sweeping snapshot rows [row_begin, row_end) (pe_place_sharded); every
        rank returns the same records."""
        out = (abi.pe_ranked_node * max(1, count))()
        placed = C.c_uint32(0)
        self._check(self._lib.pe_place_sharded(self._h, self._tg_index(tg), count, row_begin, row_end, out,
                                               C.byref(placed)))
        n = min(count, placed.value + 1)
        return [RankedNode.from_c(out[i], self.nodes) for i in range(n)]

    def last_exchange_us(self) -> float:
        """Device time of the all-gather in the last PlaceSharded (us, mean over every placement)."""
        return self._lib.pe_last_exchange_us(self._h)

    def last_exchange_stats(self):
        """(mean, min, max) us of the last PlaceSharded's all-gathers and the placements timed."""
        out = (C.c_double * 4)()
        self._lib.pe_last_exchange_stats(C.c_void_p(self._h), out)
        return float(out[0]), float(out[1]), float(out[2]), int(out[3])

    def SpeculationStats(self):
        """(runs, Selects answered from records, rollbacks, records computed) of
        the speculative count loop behind Select / Commit (pe_speculation_stats)."""
        buf = (C.c_uint64 * 4)()
        self._check(self._lib.pe_speculation_stats(self._h, buf))
        return tuple(int(x) for x in buf)

    def ChainWideStats(self):
        """(phases resolved, phases declined) by the chain's wide phase launches
        (pe_chain_wide_stats); a declined phase is left to k_chain."""
        buf = (C.c_uint64 * 2)()
        self._check(self._lib.pe_chain_wide_stats(self._h, buf))
        return tuple(int(x) for x in buf)

    def ChainWideLaunches(self):
        """Chain launches with wide phases, by kind: (with two k_phase launches,
        with both phases in one k_phases launch) (pe_chain_wide_launches)."""
        buf = (C.c_uint64 * 2)()
        self._check(self._lib.pe_chain_wide_launches(self._h, buf))
        return tuple(int(x) for x in buf)

    def ChainWideOneLds(self, n_visit, count, limit):
        """(takes, need, cap): whether one k_phases launch takes a chain launch
        of `count` Selects on `n_visit` positions, the dynamic LDS bytes it
        needs and what a workgroup of this device may hold (pe_chain_wide_one_lds)."""
        buf = (C.c_uint64 * 2)()
        rc = self._lib.pe_chain_wide_one_lds(int(n_visit), int(count), int(limit), buf)
        if rc < 0:
            self._check(rc)
        return bool(rc), int(buf[0]), int(buf[1])

    def last_phase_ms(self):
        """[host prep, kernel, D2H copy, total] of the last PlaceBatch, ms."""
        buf = (C.c_double * 4)()
        self._lib.pe_last_phase_ms(self._h, C.cast(buf, abi.f64p))
        return list(buf)

    def last_kernel_ms(self) -> float:
        return self._lib.pe_last_kernel_ms(self._h)

    def last_sweep_bytes(self) -> int:
        """Algorithmic bytes per node of the last full-scan sweep Select."""
        return self._lib.pe_last_sweep_bytes(self._h)

    def SetKernelSplit(self, on: bool = True):
        """Record HIP events between the windowed chain's kernels (measurement aid)."""
        self._check(self._lib.pe_set_kernel_split(self._h, 1 if on else 0))

    def last_kernel_split(self):
        """{k_base, k_chain, k_emit, k_emit_writeback} device ms of the last chain launch."""
        buf = (C.c_double * 4)()
        self._check(self._lib.pe_last_kernel_split(self._h, C.cast(buf, abi.f64p)))
        return dict(zip(("k_base", "k_chain", "k_emit", "k_emit_writeback"), list(buf)))


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the engine (pe_comm_unique_id): 128 bytes that
    rank 0 hands to every rank's CommInit."""
    buf = np.zeros(128, dtype=np.uint8)
    rc = load_engine().pe_comm_unique_id(buf.ctypes.data_as(abi.u8p), 128)
    if rc:
        raise RuntimeError("pe_comm_unique_id failed (%d)" % rc)
    return buf.tobytes()


class SystemStack(_Stack):
    """NewSystemStack (stack.go:207-283) on the MI355X engine."""
    stack_kind = abi.PE_STACK_SYSTEM

    def __init__(self, sysbatch: bool = False, config: SchedulerConfig = None, device: int = 0,
                 devices: Optional[Sequence[int]] = None):
        super().__init__(load_engine(), "pe_", False, config, device, devices)

    def InplaceUpdatePreempt(self, tg, allocs: Sequence[int], fallback: bool = True):
        """InplaceUpdate on a stack with preemption enabled, in one call
        (pe_inplace_update_preempt): the Select of an update whose plain fit
        fails evicts, and its record carries the whole PreemptedAllocs list
        (pe_inplace_update_preempted; no PE_MAX_PREEMPT cap). The evicted
        allocs stay in the plan's proposed state, as inplaceUpdate leaves them
        (util.go:759-802). Returns InplaceUpdate's (records, status); without
        preemption on the stack it is InplaceUpdate. A job the call refuses
        (Unsupported) is answered by inplace_update_by_select when `fallback`."""
        allocs = [int(a) for a in allocs]
        try:
            if not hasattr(self._lib, "pe_inplace_update_preempt"):
                raise Unsupported(abi.PE_EUNSUPPORTED, "no batched in-place update with preemption behind this ABI")
            n = len(allocs)
            a = np.ascontiguousarray(np.asarray(allocs or [0], dtype=np.uint32))
            out = (abi.pe_ranked_node * max(1, n))()
            status = np.zeros(max(1, n), dtype=np.uint8)
            updated = C.c_uint32(0)
            self._check(self._lib.pe_inplace_update_preempt(self._h, self._tg_index(tg), a.ctypes.data_as(abi.u32p), n,
                                                            out, status.ctypes.data_as(abi.u8p), C.byref(updated)))
        except Unsupported:
            if not fallback:
                raise
            return inplace_update_by_select(self, tg, allocs)
        full = self.InplaceUpdatePreempted()
        records = [RankedNode.from_c(out[i], self.nodes, full.get(i)) if status[i] == 0 else None for i in range(n)]
        assert updated.value == sum(1 for r in records if r is not None)
        return records, [int(x) for x in status[:n]]

    def InplaceUpdatePreempted(self) -> Dict:
        """{list position: [alloc-table rows]} of the last InplaceUpdatePreempt's
        evicting updates (pe_inplace_update_preempted)."""
        up, of, al = abi.u32p(), abi.u32p(), abi.u32p()
        ne = C.c_uint32(0)
        self._check(self._lib.pe_inplace_update_preempted(self._h, C.byref(up), C.byref(of), C.byref(al), C.byref(ne)))
        k = ne.value
        if not k:
            return {}
        off = np.ctypeslib.as_array(of, shape=(k + 1,))
        return inplace_preempted_from_csr(np.ctypeslib.as_array(up, shape=(k,)), off,
                                          np.ctypeslib.as_array(al, shape=(int(off[k]),)))

    def last_kernel_ms(self) -> float:
        return self._lib.pe_last_kernel_ms(self._h)
