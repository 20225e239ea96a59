// HIP kernels of the MI355X placement engine (gfx950, wave64).
//
// k_place<BLOCK, FULL, CORES>  persistent count loop, one workgroup per evaluation.
//   The node SoA in HBM is the snapshot's proposed state and is read-only
//   during the loop; each evaluation keeps the allocs it places in a private
//   LDS overlay (open-addressed hash keyed by node row: cpu/mem/disk/collision/
//   network deltas), so any number of evaluations share one L2-resident table
//   (NumSchedulers workers, nomad/config.go:468). Per placement the workgroup
//   sweeps the visit order from the StaticIterator cursor in chunks of BLOCK
//   positions, runs the fused ranking pipeline per node (FeasibilityWrapper
//   verdict from the class table, distinct_hosts, BinPack fit + ScoreFit, job
//   anti-affinity, rescheduling penalty, node affinity, spread, score
//   normalisation), reproduces LimitIterator + MaxScoreIterator with ballot
//   prefix counts and commits the winner to the overlay
//   (Plan.AppendAlloc). FULL=false: one wave per eval for windowed binpack
//   (limit = ceil(log2 n)); FULL=true: 256 threads per eval for full scans
//   (affinities / spreads: limit = MaxInt32) with per-value spread tables in LDS.
//   With `writeback` the overlay is merged into the HBM SoA at the end (single
//   eval API: the plan persists in the stack).
// k_system              SystemStack: independent single-node Selects, grid-stride.
// k_commit              one Plan.AppendAlloc on the HBM SoA (pe_commit).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <type_traits>
#include <cstring>
#include <vector>
#include "engine_types.h"
#include "csi_limit.h"
#include "csi_reason.h"
#include "gomath_dev.h"
#include "gosort.h"
#include "launchers.h"

namespace pe {

enum : int { kOption = 0, kFiltered = 1, kExhausted = 2 };
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kFoldMaxClasses = 16384;   // class verdict table staged in LDS by a fold

struct NodeEval {
    int status;
    double score;
    uint32_t nscores;
    double parts[PE_MAX_SCORES];
};

// Per-eval LDS overlay of the allocs this eval placed: row -> k placements.
// Every placement of the count loop has the same ask, so the deltas are k * ask.
// Packed form (k == null): one u32 per entry, row << kshift | k, which halves
// the LDS per evaluation and so doubles the evaluations resident per CU.
struct Overlay {
    uint32_t* keys;      // null: no overlay
    uint32_t* k;         // null: packed entries
    uint32_t mask;
    int bits;
    int kshift;
    uint32_t kmask;
};

__device__ __forceinline__ uint32_t ov_hash(const Overlay& o, uint32_t row) {
    return (row * 2654435761u) >> (32 - o.bits);
}

__device__ __forceinline__ uint32_t ov_count(const Overlay& o, uint32_t row) {
    if (!o.keys) return 0;
    uint32_t h = ov_hash(o, row);
    if (!o.k) {
        for (;;) {
            const uint32_t e = o.keys[h];
            if (e == kEmpty) return 0;
            if ((e >> o.kshift) == row) return e & o.kmask;
            h = (h + 1) & o.mask;
        }
    }
    for (;;) {
        const uint32_t key = o.keys[h];
        if (key == row) return o.k[h];
        if (key == kEmpty) return 0;
        h = (h + 1) & o.mask;
    }
}

// Plan.AppendAlloc into the overlay (one lane); returns the row's slot.
__device__ __forceinline__ uint32_t ov_add(const Overlay& o, uint32_t row) {
    uint32_t h = ov_hash(o, row);
    if (!o.k) {
        for (;;) {
            const uint32_t e = o.keys[h];
            if (e == kEmpty) { o.keys[h] = (row << o.kshift) | 1u; return h; }
            if ((e >> o.kshift) == row) { o.keys[h] = e + 1u; return h; }
            h = (h + 1) & o.mask;
        }
    }
    for (;;) {
        const uint32_t key = o.keys[h];
        if (key == row) { o.k[h] += 1; return h; }
        if (key == kEmpty) { o.keys[h] = row; o.k[h] = 1; return h; }
        h = (h + 1) & o.mask;
    }
}

// Slot of `row` in the overlay, or -1 when the row holds no placement.
__device__ __forceinline__ int ov_slot(const Overlay& o, uint32_t row) {
    uint32_t h = ov_hash(o, row);
    if (!o.k) {
        for (;;) {
            const uint32_t e = o.keys[h];
            if (e == kEmpty) return -1;
            if ((e >> o.kshift) == row) return (int)h;
            h = (h + 1) & o.mask;
        }
    }
    for (;;) {
        const uint32_t key = o.keys[h];
        if (key == row) return (int)h;
        if (key == kEmpty) return -1;
        h = (h + 1) & o.mask;
    }
}

__device__ __forceinline__ uint32_t pset_value(const TgTables& t, int p, uint32_t row, uint32_t cls) {
    return t.pset_val_node[p] ? t.pset_val_node[p][row] : t.pset_val_class[p][cls];
}

// The per-node HBM reads of the pipeline, all independent of each other: the
// 64-byte record, the (job, tg) collision count and the folded verdict byte.
struct NodeIn {
    NodeRec r;
    uint32_t coll_tg;
    uint32_t feas;
    uint32_t dev_free;   // free healthy instances per device group (4 x u8), device asks only
};

__device__ __forceinline__ void load_node(const NodeSoA& s, const TgTables& t, uint32_t row, NodeIn& in) {
    in.r = s.rec[row];
    in.coll_tg = t.coll_tg[row];
    in.feas = t.node_feas ? t.node_feas[row] : 1u;
    in.dev_free = t.dev_free ? t.dev_free[row] : 0u;
}

// deviceAllocator.AssignDevice for the task group's requests in order
// (scheduler/device.go:32-131, BinPack rank.go:366-414) on a node's packed
// free counts: per request the best-scoring matching group with enough free
// instances, equal scores -> the later group (the reference walks a map);
// the offer's instances are consumed (AddReserved). Returns false when a
// request cannot be met; *matched = Σ matched weights of requests with
// affinities.
__device__ __forceinline__ bool dev_assign(const Ask& a, const DevClass& dc, uint32_t& free, double* matched,
                                           uint32_t* groups = nullptr) {
    double sum = 0.0;
    if (dc.n_groups == 0) return false;   // "no devices available"
    for (int q = 0; q < kMaxDevReq; q++) {
        if (q >= a.n_dev) break;
        const uint32_t cnt = (uint32_t)a.dev_cnt[q];
        if (cnt == 0) return false;       // "invalid request of zero devices"
        int best = -1;
        double best_score = 0.0;
        for (int g = 0; g < kMaxDevGroups; g++) {
            if (g >= (int)dc.n_groups) break;
            const uint32_t f = (free >> (8 * g)) & 255u;
            if (f < cnt || !((dc.match[q] >> g) & 1u)) continue;
            const double sc = dc.choice[q][g];
            if (best >= 0 && sc < best_score) continue;
            best = g;
            best_score = sc;
        }
        if (best < 0) return false;        // "no devices match request"
        free -= cnt << (8 * best);
        if (groups) groups[q] = (uint32_t)best;
        if ((a.dev_aff >> q) & 1u) sum += dc.matched[q][best];
    }
    *matched = sum;
    return true;
}

// Device state after k further placements of the task group on a node.
__device__ __forceinline__ uint32_t dev_after(const Ask& a, const DevClass& dc, uint32_t free, uint32_t k) {
    for (uint32_t j = 0; j < k; j++) {
        double m;
        dev_assign(a, dc, free, &m);
    }
    return free;
}

// Reserved cores of the (dk+1)-th placement on the row, out of line so that
// the hot pipeline keeps its registers: status 1 when too few cores are free
// ("cores"), 2 when a chosen core is outside the AllocsFit-available set;
// cpu = the cores' CpuShares (SharesPerCore x cores).
struct CoreFit {
    int64_t cpu;
    int32_t status;
};

__device__ __forceinline__ CoreFit core_fit(const uint64_t* rsvable, const uint64_t* used, const uint64_t* avail,
                                         const int64_t* spc, uint32_t cores, uint32_t row, uint32_t dk) {
    CoreFit f{0, 1};
    if (!rsvable) return f;
    uint32_t skip = dk * cores, need = cores;
    uint64_t out = 0, any_av = 0;
#pragma unroll 1
    for (int w = 0; w < 4; w++) {
        any_av |= avail[4 * row + w];
        uint64_t fr = rsvable[4 * row + w] & ~used[4 * row + w];
        const uint32_t c = (uint32_t)__popcll(fr);
        if (skip >= c) { skip -= c; continue; }
        for (; skip; skip--) fr &= fr - 1;
        uint64_t ch = 0;
        for (; fr && need; need--) { ch |= fr & (~fr + 1); fr &= fr - 1; }
        out |= ch & ~avail[4 * row + w];
    }
    if (need) return f;
    f.status = (any_av && out) ? 2 : 0;
    f.cpu = (int64_t)cores * spc[row];
    return f;
}

// CpuShares of one placement on the row: tasks with cores hold SharesPerCore x
// cores (rank.go:461-463).
__device__ __forceinline__ int64_t ask_cpu(const NodeSoA& s, const Ask& a, uint32_t row) {
    return a.cores > 0 ? a.cpu + (int64_t)a.cores * s.core_spc[row] : a.cpu;
}

// Plan.AppendAlloc of k placements on the row: their cores leave the free set.
__device__ __forceinline__ void core_take_rows(const uint64_t* rsvable, uint64_t* used, uint32_t row, uint32_t need) {
#pragma unroll 1
    for (int w = 0; w < 4 && need; w++) {
        uint64_t f = rsvable[4 * row + w] & ~used[4 * row + w], t = 0;
        for (; f && need; need--) { t |= f & (~f + 1); f &= f - 1; }
        used[4 * row + w] |= t;
    }
}

__device__ __forceinline__ void core_take(const NodeSoA& s, const Ask& a, uint32_t row, uint32_t k) {
    if (a.cores > 0 && s.core_rsvable) core_take_rows(s.core_rsvable, s.core_used, row, k * (uint32_t)a.cores);
}

// Inputs of the scoring half of the pipeline (everything after AllocsFit).
// The table lookups (affinity, spread, penalty) are resolved by
// lookup_scores so that their loads issue with the node's own loads; the
// scoring half is then pure arithmetic.
struct ScoreIn {
    int64_t ccpu, cmem, ucpu, umem;   // capacity and proposed use including the ask
    double dev_aff;                   // BinPack device-affinity score (appended when Ask::dev_tw != 0)
    double aff;                       // NodeAffinityIterator score (0 = not appended)
    double spread;                    // SpreadIterator total (0 = not appended)
    uint32_t coll;                    // proposed allocs of (job, tg) on the node
    uint32_t penalty;                 // node in the rescheduling penalty set
};

// Feasibility half of the fused per-node pipeline over base (HBM) + overlay
// (dk placements of this eval): FeasibilityWrapper verdict, distinct_hosts,
// BinPack network offers and AllocsFit. Returns kOption with the scoring
// inputs filled, else kFiltered / kExhausted.
// DistinctPropertyIterator (feasible.go:601-704): the node's value of each
// distinct_property set must exist and be used fewer than `allowed` times.
// `tab` (the eval's per-value table, 0.0 = open) or the HBM counts.
__device__ __forceinline__ bool distinct_ok(const TgTables& t, const double* tab, uint32_t row, uint32_t c) {
    for (int p = t.n_spread; p < t.n_psets; p++) {
        const uint32_t v = pset_value(t, p, row, c);
        if (v == kMissing) return false;
        const bool blocked = tab ? tab[t.pset_tab_off[p] + v] != 0.0 : t.pset_counts[p][v] >= t.pset_allowed[p];
        if (blocked) return false;
    }
    return true;
}

// kDistinctHosts false (k_trace<true>): the caller ran the distinct_hosts test
// itself, on a job count the column does not hold.
template <bool kCores = true, bool kDistinctHosts = true>
__device__ __forceinline__ int status_loaded(const NodeSoA& s, const TgTables& t, const uint8_t* class_ok,
                                             const Ask& a, uint32_t dk, uint32_t row, const NodeIn& in,
                                             ScoreIn* si, const double* ptab = nullptr) {
    const NodeRec& r = in.r;
    const uint32_t c = r.cls;
    // FeasibilityWrapper: memoised job + task-group checks (host-resolved per class)
    bool ok;
    if (t.node_feas) ok = in.feas != 0;
    else {
        ok = class_ok[c] != 0;
        if (t.node_ok) ok = ok && t.node_ok[row] != 0;
    }
    const uint32_t coll = in.coll_tg + dk;
    // DistinctHostsIterator (feasible.go:569-595)
    if (kDistinctHosts && ok && (a.distinct_job | a.distinct_tg)) {
        if (a.distinct_job && s.coll_job[row] + dk > 0) ok = false;
        if (a.distinct_tg && coll > 0) ok = false;
    }
    if (ok && t.n_psets > t.n_spread) ok = distinct_ok(t, ptab, row, c);
    if (!ok) return kFiltered;
    // BinPackIterator (rank.go:193-527): network offers, then AllocsFit.
    // AssignPorts' static ports first (network.go:317-363): the host-built gate
    // (free on the node's address, no placement of the group since)
    if (t.static_gate) {
        const uint32_t gt = t.static_gate[row];
        if (gt == 0u || in.coll_tg + dk + 1u != gt) return kExhausted;
    }
    if (a.tg_dyn > 0 || a.has_task_net) {
        int32_t dyn = r.used_dyn + (int32_t)dk * a.commit_dyn;
        if (a.tg_dyn > 0) {
            if ((t.alias_ok && !t.alias_ok[row]) || kDynPortCapacity - dyn - a.static_dyn < 1) return kExhausted;
            dyn += a.tg_dyn + a.static_dyn;
        }
        if (a.has_task_net) {
            const uint32_t md_lim = t.md ? t.md[row].lim : ~0u;
            if (md_lim != ~0u) {   // a multi-device node: the host's first fit over its devices
                if (in.coll_tg + dk >= md_lim) return kExhausted;
            } else {
                const int32_t avail = r.avail_mbits;
                const int32_t mb = r.used_mbits + (int32_t)dk * a.commit_mbits;
                if (avail < 0 || mb + a.task_mbits > avail || kDynPortCapacity - dyn < a.task_dyn) return kExhausted;
                if (t.task_gate) {   // AssignNetwork's static ports (network.go:419-431), host-built gate
                    const uint32_t gt = t.task_gate[row];
                    if (gt == 0u || in.coll_tg + dk + 1u != gt) return kExhausted;
                }
            }
        }
    }
    si->dev_aff = 0.0;
    if (a.n_dev > 0) {   // devices: this eval's dk earlier placements first consumed their offers
        const DevClass& dc = t.dev_cls[c];
        uint32_t fr = dev_after(a, dc, in.dev_free, dk);
        double m;
        if (!dev_assign(a, dc, fr, &m)) return kExhausted;
        if (a.dev_tw != 0.0) si->dev_aff = m / a.dev_tw;
    }
    int64_t acpu = a.cpu;
    bool core_out = false;
    if (kCores && a.cores > 0) {   // reserved cores (rank.go:437-466), then AllocsFit's Superset check
        const CoreFit f = core_fit(s.core_rsvable, s.core_used, s.core_avail, s.core_spc, (uint32_t)a.cores, row, dk);
        if (f.status == 1) return kExhausted;
        acpu += f.cpu;
        core_out = f.status == 2;
    }
    const int64_t ucpu = r.used_cpu + (int64_t)(dk + 1) * acpu;
    const int64_t umem = r.used_mem + (int64_t)(dk + 1) * a.mem;
    const int64_t udisk = r.used_disk + (int64_t)(dk + 1) * a.disk;
    if (r.cap_cpu < ucpu || core_out || r.cap_mem < umem || r.cap_disk < udisk) return kExhausted;
    si->ccpu = r.cap_cpu;
    si->cmem = r.cap_mem;
    si->ucpu = ucpu;
    si->umem = umem;
    si->coll = coll;
    return kOption;
}

// Table lookups of the scoring half for an option: penalty bit, node affinity,
// spread total (per-property boosts summed in property order, spread.go:145-170).
__device__ __forceinline__ void lookup_scores(const TgTables& t, const uint32_t* penalty_bits,
                                              const double* spread_tab, uint32_t row, uint32_t c, ScoreIn* si) {
    si->penalty = penalty_bits ? (penalty_bits[row >> 5] >> (row & 31)) & 1u : 0u;
    si->aff = (t.class_aff || t.node_aff) ? (t.node_aff ? t.node_aff[row] : t.class_aff[c]) : 0.0;
    double total = 0.0;
    for (int p = 0; p < t.n_spread; p++) {
        const uint32_t v = pset_value(t, p, row, c);
        total += (v == kMissing) ? -1.0 : spread_tab[t.pset_tab_off[p] + v];
    }
    si->spread = total;
}

// Scoring half: scores in append order, summed left to
// right, then ScoreNormalizationIterator.
// The scores before the spread one, summed left to right; k = how many.
template <bool kKeepParts>
__device__ __forceinline__ double score_head(const Ask& a, double log10, const ScoreIn& si, double* parts,
                                             uint32_t& k_out) {
    const uint32_t coll = si.coll;
    const double fit = gm::fit_score(si.ccpu, si.cmem, si.ucpu, si.umem, a.algo_spread, log10);
    double sum = fit;
    uint32_t k = 1;
    if (kKeepParts) parts[0] = fit;
    if (a.dev_tw != 0.0) {   // device affinity (rank.go:518-523)
        sum += si.dev_aff;
        if (kKeepParts) parts[k] = si.dev_aff;
        k++;
    }
    if (a.anti_aff && coll > 0) {   // JobAntiAffinityIterator (rank.go:588-591)
        const double pen = -1 * (double)(coll + 1) / (double)a.desired_count;
        sum += pen;
        if (kKeepParts) parts[k] = pen;
        k++;
    }
    if (si.penalty) {   // NodeReschedulingPenaltyIterator (rank.go:632-635)
        sum += -1.0;
        if (kKeepParts) parts[k] = -1.0;
        k++;
    }
    if (si.aff != 0.0) {   // NodeAffinityIterator (rank.go:698-725)
        sum += si.aff;
        if (kKeepParts) parts[k] = si.aff;
        k++;
    }
    k_out = k;
    return sum;
}

// The normalised score; with kKeepParts the parts go to `parts` (any
// address space: a runtime index into a stack array would live in scratch).
template <bool kKeepParts>
__device__ __forceinline__ double score_into(const Ask& a, double log10, const ScoreIn& si, double* parts,
                                             uint32_t* nscores) {
    uint32_t k;
    double sum = score_head<kKeepParts>(a, log10, si, parts, k);
    if (si.spread != 0.0) {   // SpreadIterator (spread.go:110-174)
        sum += si.spread;
        if (kKeepParts) parts[k] = si.spread;
        k++;
    }
    *nscores = k;
    return sum / (double)k;   // ScoreNormalizationIterator (rank.go:762-767)
}

template <bool kKeepParts>
__device__ __forceinline__ void score_option(const Ask& a, double log10, const ScoreIn& si, NodeEval* out) {
    uint32_t k;
    double sum = score_head<kKeepParts>(a, log10, si, out->parts, k);
    if (si.spread != 0.0) {   // SpreadIterator (spread.go:110-174)
        sum += si.spread;
        if (kKeepParts) out->parts[k] = si.spread;
        k++;
    }
    out->status = kOption;
    out->score = sum / (double)k;   // ScoreNormalizationIterator (rank.go:762-767)
    out->nscores = k;
}

// The whole fused per-node pipeline.
template <bool kKeepParts, bool kCores = true>
__device__ __forceinline__ void eval_loaded(const NodeSoA& s, const TgTables& t, const uint8_t* class_ok,
                                            const Ask& a, uint32_t dk, const uint32_t* penalty_bits,
                                            double log10, const double* spread_tab, uint32_t row,
                                            const NodeIn& in, NodeEval* out) {
    ScoreIn si;
    const int st = status_loaded<kCores>(s, t, class_ok, a, dk, row, in, &si, spread_tab);
    if (st != kOption) { out->status = st; return; }
    lookup_scores(t, penalty_bits, spread_tab, row, in.r.cls, &si);
    score_option<kKeepParts>(a, log10, si, out);
}

template <bool kKeepParts, bool kCores = true>
__device__ __forceinline__ void eval_node(const NodeSoA& s, const TgTables& t, const uint8_t* class_ok,
                                          const Ask& a, const Overlay& ov, const uint32_t* penalty_bits,
                                          double log10, const double* spread_tab, uint32_t row,
                                          NodeEval* out) {
    NodeIn in;
    load_node(s, t, row, in);
    eval_loaded<kKeepParts, kCores>(s, t, class_ok, a, ov_count(ov, row), penalty_bits, log10, spread_tab, row, in,
                            out);
}

// AllocMetric trace (structs.go:9903-9937): for visited rows that passed the
// FeasibilityWrapper, which iterator stopped them and why, with the same state
// the Select saw (HBM SoA, no overlay). Codes: kTr* in engine_types.h; a
// distinct_property failure carries its set index in bits 8-15.
// Options also get their named scores (ScoreNode calls, rank.go:516-522, 591-593,
// 635-637, 704-722, spread.go:170, rank.go:769) as 6 doubles: binpack, devices,
// job-anti-affinity, node-affinity, allocation-spread, normalized-score.
// Row of entry j of record k of a batched trace (TraceSrc).
__device__ __forceinline__ uint32_t trace_row(const TraceSrc& r, uint32_t k, uint32_t j) {
    const uint32_t src = r.rsrc[k];
    if (!(src & kTraceRot)) return r.rows[src + j];
    uint32_t p = (src - kTraceRot) + j;
    if (p >= r.n_list) p -= r.n_list;
    return r.list[p];
}

// Placements of records before k on `row` (the sorted (row, record) pairs).
__device__ __forceinline__ uint32_t trace_dk(const TraceSrc& r, uint32_t row, uint32_t k) {
    const uint64_t key = (uint64_t)row << 32;
    uint32_t lo = 0, hi = r.n_pl;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (r.pl[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    uint32_t d = 0;
    for (; lo < r.n_pl && (uint32_t)(r.pl[lo] >> 32) == row && (uint32_t)r.pl[lo] < k; lo++) d++;
    return d;
}

// Record of entry i of a batched trace: the first k with rec_end[k] > i.
__device__ __forceinline__ uint32_t trace_rec(const TraceSrc& r, uint32_t i) {
    uint32_t lo = 0, hi = r.n_rec;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (r.rec_end[mid] > i) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// Why BinPack exhausts the (dk+1)-th placement of the group on a loaded node
// (k_trace's chain, also walked by the multi-group system pass on a lane's
// register image). trace_offers: the network offers, then
// AssignDevice, in BinPack's order; the network columns of `in` already hold
// the dk earlier placements. kTrOption: the offers succeed.
__device__ __forceinline__ uint32_t trace_offers(const TgTables& t, const Ask& a, uint32_t row, const NodeIn& in,
                                                 uint32_t dk) {
    const NodeRec& r = in.r;
    uint32_t code = kTrOption;
    if (t.static_gate &&                                           // AssignPorts static ports (network.go:317-363)
        (t.static_gate[row] == 0u || in.coll_tg + dk + 1u != t.static_gate[row]))
        code = kTrStaticPort;
    if (code == kTrOption && (a.tg_dyn > 0 || a.has_task_net)) {   // rank.go:231-295
        int32_t dyn = r.used_dyn;
        if (a.tg_dyn > 0) {
            if (t.alias_ok && !t.alias_ok[row]) code = kTrNoAddr;
            else if (kDynPortCapacity - dyn - a.static_dyn < 1) code = kTrDynPorts;
            dyn += a.tg_dyn + a.static_dyn;
        }
        const uint32_t md_lim = (code == kTrOption && a.has_task_net && t.md) ? t.md[row].lim : ~0u;
        if (md_lim != ~0u) {   // a multi-device node: the host's outcome of the first refused placement
            if (in.coll_tg + dk >= md_lim) code = t.md[row].code;
        } else if (code == kTrOption && a.has_task_net) {
            if (r.avail_mbits < 0) code = kTrNoNetworks;
            else if (r.used_mbits + a.task_mbits > r.avail_mbits) code = kTrBandwidth;
            else if (t.task_gate && (t.task_gate[row] == 0u || in.coll_tg + dk + 1u != t.task_gate[row])) code = kTrTaskStatic;
            else if (kDynPortCapacity - dyn < a.task_dyn) code = kTrTaskDyn;
        }
    }
    if (code == kTrOption && a.n_dev > 0) {                         // AssignDevice errors (device.go:32-131)
        const DevClass& dc = t.dev_cls[r.cls];
        uint32_t free = dk ? dev_after(a, dc, in.dev_free, dk) : in.dev_free;
        if (dc.n_groups == 0) code = kTrDevNone;
        for (int q = 0; q < kMaxDevReq && code == kTrOption; q++) {
            if (q >= a.n_dev) break;
            const uint32_t cnt = (uint32_t)a.dev_cnt[q];
            if (cnt == 0) { code = kTrDevZero; break; }
            int best = -1;
            double best_score = 0.0;
            for (int g = 0; g < kMaxDevGroups; g++) {
                if (g >= (int)dc.n_groups) break;
                const uint32_t f = (free >> (8 * g)) & 255u;
                if (f < cnt || !((dc.match[q] >> g) & 1u)) continue;
                const double sc = dc.choice[q][g];
                if (best >= 0 && sc < best_score) continue;
                best = g;
                best_score = sc;
            }
            if (best < 0) { code = kTrDevNoMatch; break; }
            free -= cnt << (8 * best);
        }
    }
    return code;
}

// trace_fit: AllocsFit's dimension in its Superset order (core_out: a chosen
// reserved core outside the available set). kTrOption: the placement fits.
__device__ __forceinline__ uint32_t trace_fit(const NodeSoA& s, const Ask& a, uint32_t row, const NodeRec& r, uint32_t dk,
                                              bool core_out) {
    const int64_t k1 = (int64_t)dk + 1;
    if (r.cap_cpu < r.used_cpu + k1 * ask_cpu(s, a, row)) return kTrCpu;
    if (core_out) return kTrCores;
    if (r.cap_mem < r.used_mem + k1 * a.mem) return kTrMemory;
    if (r.cap_disk < r.used_disk + k1 * a.disk) return kTrDisk;
    return kTrOption;
}

// The node image record k's Select of a destructive loop saw (k_trace<true>,
// TraceStops), from the image of the loop's starting state: the stops of
// records <= k on the row leave it (ds_stop's arithmetic) and the dk placements
// of records < k join it (ds_fold_row's), so the caller goes on with dk = 0.
// All of it is integer sums, so the order is free, except for a device ask:
// which group a placement's offer takes depends on the free counts it meets,
// so the row's stops and placements are replayed in record order, the stop of
// record j before the placement of record j. *job_sub: the stops that leave the
// job's collision count. False: an event's slot is out of range.
__device__ __forceinline__ bool trace_stops(const TgTables& t, const Ask& a, const TraceSrc& src, const TraceStops& S,
                                            uint32_t row, uint32_t k, uint32_t dk, NodeIn& in, uint32_t* job_sub) {
    const uint64_t key = (uint64_t)row << 32;
    uint32_t lo = 0, hi = S.n_ev;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (S.ev[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    const bool devs = a.n_dev > 0 && t.dev_free;
    uint32_t pi = 0, taken = 0;   // the row's placements: the next one, and how many the free counts hold
    if (devs && dk) {
        hi = src.n_pl;
        while (pi < hi) {
            const uint32_t mid = (pi + hi) >> 1;
            if (src.pl[mid] < key) pi = mid + 1;
            else hi = mid;
        }
    }
    NodeRec& r = in.r;
    uint32_t free = in.dev_free, sub = 0;
    for (; lo < S.n_ev && (uint32_t)(S.ev[lo] >> 32) == row; lo++) {
        const uint32_t w = (uint32_t)S.ev[lo], j = w >> 3;
        if (j > k) break;
        if (devs)   // the placements of records before this stop's
            for (; taken < dk && pi < src.n_pl && (uint32_t)src.pl[pi] < j; pi++, taken++) {
                double m;
                dev_assign(a, t.dev_cls[r.cls], free, &m);
            }
        if (w & kDsLive) {
            const uint32_t slot = S.slot[lo];
            if (slot >= S.n_slots) return false;
            const PreemptAlloc x = S.palloc[slot];
            r.used_cpu -= x.cpu;
            r.used_mem -= x.mem;
            r.used_disk -= x.disk;
            r.used_mbits -= x.mbits;
            r.used_dyn -= x.dyn;
            if (devs)
                for (int q = 0; q < 4 && q < (int)x.n_dev; q++)
                    free += ((x.dev_c >> (8 * q)) & 255u) << (8 * ((x.dev_g >> (8 * q)) & 255u));
        }
        if (w & kDsJob) sub++;
        if (w & kDsTg) in.coll_tg--;
    }
    if (devs) free = dev_after(a, t.dev_cls[r.cls], free, dk - taken);
    in.dev_free = free;
    r.used_cpu += (int64_t)dk * a.cpu;
    r.used_mem += (int64_t)dk * a.mem;
    r.used_disk += (int64_t)dk * a.disk;
    r.used_mbits += (int32_t)dk * a.commit_mbits;
    r.used_dyn += (int32_t)dk * a.commit_dyn;
    in.coll_tg += dk;
    *job_sub = sub;
    return true;
}

// dk (TraceSrc): placements of this task group on the row that the state
// lacks (a speculative run's earlier Selects, traced against the run's
// starting state; no distinct_property sets then), applied as status_loaded
// does. In a batched trace record k's spread boosts are spread_tab + k *
// pset_tab_total (k_spread_tables: the record's own use counts).
// kStops (a batched trace of a destructive loop's records; no reserved-cores
// ask): the loaded image is first brought to what record k's Select saw
// (trace_stops), and every check after it runs on that image with dk = 0.
template <bool kStops>
__global__ void k_trace(NodeSoA s, TgTables t, Ask a, TraceSrc src, uint32_t n, uint32_t* out,
                        const uint32_t* penalty_bits, double log10, const double* spread_tab, double* sc,
                        TraceStops stops) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t row, dk, rec = 0;
    if (src.rec_end) {
        const uint32_t k = trace_rec(src, i);
        row = trace_row(src, k, i - (k ? src.rec_end[k - 1] : 0u));
        dk = trace_dk(src, row, k);
        if (spread_tab) spread_tab += (size_t)k * t.pset_tab_total;
        rec = k;
    } else {
        row = src.rows[i];
        dk = src.dks ? (uint32_t)src.dks[i] : 0u;
    }
    if (kStops && row >= s.n) {   // (the host walk's rows are the visit list's: a guard)
        out[i] = kTrMismatch;
        return;
    }
    NodeIn in;
    load_node(s, t, row, in);
    NodeRec& r = in.r;
    const uint32_t c = r.cls;
    uint32_t code = kTrOption;
    uint32_t dj = dk;   // what the job's collision column lacks
    if (kStops) {
        uint32_t sub;
        if (!trace_stops(t, a, src, stops, row, rec, dk, in, &sub)) {
            out[i] = kTrMismatch;
            return;
        }
        dj = dk - sub;
        dk = 0;
    }
    if ((a.distinct_job && s.coll_job[row] + dj > 0) || (a.distinct_tg && in.coll_tg + dk > 0)) {
        code = kTrDistinctHosts;                                   // feasible.go:569-595
    } else {
        for (int p = t.n_spread; p < t.n_psets && code == kTrOption; p++) {
            const uint32_t v = pset_value(t, p, row, c);
            if (v == kMissing || t.pset_counts[p][v] >= t.pset_allowed[p]) code = kTrDistinctProp | ((uint32_t)p << 8);
        }
    }
    if (dk) {   // the earlier placements' network use
        r.used_dyn += (int32_t)dk * a.commit_dyn;
        r.used_mbits += (int32_t)dk * a.commit_mbits;
    }
    if (code == kTrOption) code = trace_offers(t, a, row, in, dk);
    bool core_out = false;
    if (code == kTrOption && a.cores > 0) {                         // reserved cores (rank.go:437-466)
        const CoreFit f = core_fit(s.core_rsvable, s.core_used, s.core_avail, s.core_spc, (uint32_t)a.cores, row, dk);
        if (f.status == 1) code = kTrCores;
        core_out = f.status == 2;
    }
    if (code == kTrOption) code = trace_fit(s, a, row, r, dk, core_out);
    if (code == kTrOption) {
        ScoreIn si;
        if (dk) {   // status_loaded applies dk itself: the network columns as loaded
            r.used_dyn -= (int32_t)dk * a.commit_dyn;
            r.used_mbits -= (int32_t)dk * a.commit_mbits;
        }
        if (status_loaded<true, !kStops>(s, t, t.class_ok, a, dk, row, in, &si) != kOption) {
            out[i] = kTrMismatch;
            return;
        }
        lookup_scores(t, penalty_bits, spread_tab, row, c, &si);
        NodeEval ev;
        score_option<true>(a, log10, si, &ev);
        double* o = sc + (size_t)i * 6;
        uint32_t k = 1;
        o[0] = ev.parts[0];
        o[1] = a.dev_tw != 0.0 ? ev.parts[k++] : 0.0;
        o[2] = (a.anti_aff && si.coll > 0) ? ev.parts[k++] : 0.0;
        if (si.penalty) { code |= kTrPenalty; k++; }
        o[3] = si.aff != 0.0 ? ev.parts[k++] : 0.0;
        o[4] = si.spread != 0.0 ? ev.parts[k++] : 0.0;
        o[5] = ev.score;
    }
    out[i] = code;
}

// ScoreMetaData of every record of a speculative run from k_trace's outcomes
// (rows of record k: rec_end[k-1] .. rec_end[k]): one wave per record pushes
// its options' NormScores in visit order into a 5-slot min-heap exactly as
// kheap.ScoreHeap.Push does under container/heap (replace the minimum only
// when strictly greater, heap.Fix, then up(len - 1); lib/kheap/score_heap.go),
// pops them (GetItemsReverse) and writes the NodeScoreMeta items in their
// binary form with the names metrics_outcome gives them
// (structs.go:9976-10018). flags: 1 devices scored, 2 job anti-affinity
// scored, 4 node affinities exist, 8 generic stack.
// A push that does not enter a full heap changes nothing, and the heap's
// minimum only grows. The record's entries are split among the block's waves;
// each wave keeps the top-5 NormScores of its own segment so far and lists the
// entries that enter it: an entry that does not enter its segment's top-5 is
// at or below the minimum of a heap that has seen at least that prefix, so it
// does not enter the record's heap either. Wave 0 then pushes the listed
// entries in order into the heap (held alike in every lane). A segment with
// more entering entries than its list holds sends the record to wave 0's
// sequential pass over every entry.
constexpr uint32_t kTopWaves = 16, kTopCand = 128;
// n_other (or null): per record, its entries that are not options, the first
// kTopOther of them (entry index within the record, code; in no particular
// order) at other_list + k * kTopOther.
constexpr uint32_t kTopOther = 128;
__global__ void __launch_bounds__(1024) k_trace_top(const uint32_t* codes, const double* sc, TraceSrc src,
                                                    uint32_t flags, pe_metric_score* out, uint8_t* n_out,
                                                    uint32_t* n_other, uint2* other_list) {
    __shared__ uint32_t cand_x[kTopWaves][kTopCand];
    __shared__ double cand_v[kTopWaves][kTopCand];
    __shared__ uint32_t cand_n[kTopWaves];
    __shared__ uint32_t overflow, others;
    const uint32_t k = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    if (k >= src.n_rec) return;   // uniform across the block
    const uint32_t b = k ? src.rec_end[k - 1] : 0u, e = src.rec_end[k];
    if (tid == 0) overflow = others = 0;
    __syncthreads();
    {   // phase 1: the segment's entering entries (and its entries that are not options)
        const uint32_t total = e - b, seg = (total + nw - 1) / nw;
        const uint32_t sb = b + min(total, w * seg), se = b + min(total, (w + 1) * seg);
        double t[5];   // the segment's top-5 so far (values), unsorted; tmin its minimum once full
        uint32_t tl = 0, nc = 0, n_not = 0;
        double tmin = 0.0;
        bool over = false;
        constexpr uint32_t U = 4;
        for (uint32_t c = sb; c < se; c += 64 * U) {
            uint32_t cd[U];
#pragma unroll
            for (uint32_t u = 0; u < U; u++) {
                const uint32_t x = c + u * 64 + lane;
                cd[u] = x < se ? codes[x] : 0xFFFFFFFFu;
            }
#pragma unroll
            for (uint32_t u = 0; u < U; u++) {
                const uint32_t x = c + u * 64 + lane;
                const bool opt = (cd[u] & 255u) == kTrOption;
                const bool other = x < se && !opt;
                n_not += (uint32_t)__popcll(__ballot(other));
                if (other && other_list) {
                    const uint32_t q = atomicAdd(&others, 1u);
                    if (q < kTopOther) other_list[(size_t)k * kTopOther + q] = make_uint2(x - b, cd[u]);
                }
                const double v = opt ? sc[(size_t)x * 6 + 5] : 0.0;
                uint64_t mask = __ballot(opt && (tl < 5 || v > tmin));
                while (mask) {
                    const uint32_t l = (uint32_t)__ffsll((unsigned long long)mask) - 1u;
                    mask &= mask - 1;
                    const double nv = __shfl(v, (int)l);
                    if (tl < 5) {
                        t[tl++] = nv;   // tl is wave-uniform: a static index after unrolling below
                    } else if (nv > tmin) {
                        bool done = false;   // replace one minimum
#pragma unroll
                        for (int q = 0; q < 5; q++)
                            if (!done && t[q] == tmin) { t[q] = nv; done = true; }
                    } else {
                        continue;
                    }
                    if (tl == 5) {
                        tmin = t[0];
#pragma unroll
                        for (int q = 1; q < 5; q++) tmin = t[q] < tmin ? t[q] : tmin;
                    }
                    if (nc < kTopCand) {
                        if (lane == 0) {
                            cand_x[w][nc] = c + u * 64 + l;
                            cand_v[w][nc] = nv;
                        }
                        nc++;
                    } else {
                        over = true;
                    }
                }
            }
        }
        if (lane == 0) {
            cand_n[w] = nc;
            if (over) atomicOr(&overflow, 1u);
            if (n_not && !other_list) atomicAdd(&others, n_not);
        }
    }
    __syncthreads();
    if (tid == 0 && n_other) n_other[k] = others;
    if (w != 0) return;
    double hn[5];
    uint32_t hi[5];
    uint32_t len = 0;
    auto less = [&](uint32_t x, uint32_t y) { return hn[x] < hn[y]; };
    auto swap_ = [&](uint32_t x, uint32_t y) {
        const double tn = hn[x]; hn[x] = hn[y]; hn[y] = tn;
        const uint32_t ti = hi[x]; hi[x] = hi[y]; hi[y] = ti;
    };
    auto up = [&](uint32_t j) {
        while (j > 0) {
            const uint32_t i = (j - 1) / 2;
            if (!less(j, i)) break;
            swap_(i, j);
            j = i;
        }
    };
    auto down = [&](uint32_t i0, uint32_t n) {
        uint32_t i = i0;
        for (;;) {
            const uint32_t j1 = 2 * i + 1;
            if (j1 >= n) break;
            uint32_t j = j1;
            if (j1 + 1 < n && less(j1 + 1, j1)) j = j1 + 1;
            if (!less(j, i)) break;
            swap_(i, j);
            i = j;
        }
        return i > i0;
    };
    auto push = [&](double norm, uint32_t x) {   // ScoreHeap.Push under container/heap
        if (len < 5) {
            hn[len] = norm;
            hi[len] = x;
            len++;
        } else if (norm > hn[0]) {
            hn[0] = norm;
            hi[0] = x;
            if (!down(0, len)) up(0);
        }
        up(len - 1);
    };
    if (!overflow) {
        for (uint32_t q = 0; q < nw; q++)
            for (uint32_t i = 0; i < cand_n[q]; i++) push(cand_v[q][i], cand_x[q][i]);
    } else {   // every entry in order, 64 at a time (a candidate pass over the whole record)
        for (uint32_t c = b; c < e; c += 64) {
            const uint32_t x = c + lane;
            const bool opt = x < e && (codes[x] & 255u) == kTrOption;
            const double v = opt ? sc[(size_t)x * 6 + 5] : 0.0;
            uint64_t mask = __ballot(opt && (len < 5 || v > hn[0]));
            while (mask) {
                const uint32_t l = (uint32_t)__ffsll((unsigned long long)mask) - 1u;
                mask &= mask - 1;
                push(__shfl(v, (int)l), c + l);
            }
        }
    }
    if (lane != 0) return;
    // GetItemsReverse: heap.Pop until empty, the last popped first
    uint32_t order[5];
    const uint32_t total = len;
    uint32_t at = total;
    while (len > 0) {
        const uint32_t n = len - 1;
        swap_(0, n);
        down(0, n);
        order[--at] = hi[n];
        len--;
    }
    n_out[k] = (uint8_t)total;
    for (uint32_t q = 0; q < total; q++) {
        const uint32_t x = order[q];
        const double* o = sc + (size_t)x * 6;
        pe_metric_score m;
        for (int j = 0; j < PE_MAX_SCORES; j++) { m.scorer[j] = 0; m.score[j] = 0.0; }
        uint32_t ns = 0;
        m.scorer[ns] = PE_SCORER_BINPACK; m.score[ns++] = o[0];
        if (flags & 1u) { m.scorer[ns] = PE_SCORER_DEVICES; m.score[ns++] = o[1]; }
        if (flags & 8u) {   // the SystemStack ranks with BinPack alone (stack.go:277-281)
            if (flags & 2u) { m.scorer[ns] = PE_SCORER_JOB_ANTI_AFFINITY; m.score[ns++] = o[2]; }
            m.scorer[ns] = PE_SCORER_RESCHEDULE_PENALTY;
            m.score[ns++] = (codes[x] & kTrPenalty) ? -1.0 : 0.0;
            if (!(flags & 4u)) { m.scorer[ns] = PE_SCORER_NODE_AFFINITY; m.score[ns++] = 0.0; }
            else if (o[3] != 0.0) { m.scorer[ns] = PE_SCORER_NODE_AFFINITY; m.score[ns++] = o[3]; }
            if (o[4] != 0.0) { m.scorer[ns] = PE_SCORER_ALLOCATION_SPREAD; m.score[ns++] = o[4]; }
        }
        m.row = (int32_t)trace_row(src, k, x - b);
        m.n_scores = ns;
        m.norm = o[5];
        out[(size_t)k * 5 + q] = m;
    }
}

// evenSpreadScoreBoost (spread.go:178-228) / target boost (spread.go:143-164)
// per value of each property set, from the eval's use counts: `counts` in the
// pset_cnt_off layout (an LDS copy, or the loop's own counts), or null to read
// each set's HBM counts. `tab` in the pset_tab_off layout.
template <int BLOCK>
__device__ void build_spread_table(const TgTables& t, const uint32_t* counts, double* tab, uint32_t* scratch) {
    const int tid = threadIdx.x;
    for (int p = 0; p < t.n_psets; p++) {
        const int nv = t.pset_nvals[p];
        const uint32_t* cnt = counts ? counts + t.pset_cnt_off[p] : t.pset_counts[p];
        double* tb = tab + t.pset_tab_off[p];
        if (p >= t.n_spread) {   // distinct_property: 1.0 marks a value at its allowed count
            for (int v = tid; v < nv; v += BLOCK) tb[v] = cnt[v] >= t.pset_allowed[p] ? 1.0 : 0.0;
            continue;
        }
        if (t.pset_even[p]) {
            // min / max / number of the used values (any count of values: a
            // block reduction, the same integers as the reference's map walk)
            uint32_t lmn = 0xFFFFFFFFu, lmx = 0, lpr = 0;
            for (int v = tid; v < nv; v += BLOCK) {
                const uint32_t x = cnt[v];
                if (x == 0) continue;
                lpr++;
                lmn = x < lmn ? x : lmn;
                lmx = x > lmx ? x : lmx;
            }
            for (int off = 32; off > 0; off >>= 1) {
                lmn = min(lmn, (uint32_t)__shfl_xor((int)lmn, off));
                lmx = max(lmx, (uint32_t)__shfl_xor((int)lmx, off));
                lpr += (uint32_t)__shfl_xor((int)lpr, off);
            }
            if (tid == 0) { scratch[0] = 0xFFFFFFFFu; scratch[1] = 0; scratch[2] = 0; }
            __syncthreads();
            if ((tid & 63) == 0) {
                atomicMin(&scratch[0], lmn);
                atomicMax(&scratch[1], lmx);
                atomicAdd(&scratch[2], lpr);
            }
            __syncthreads();
            if (tid == 0 && scratch[2] == 0) { scratch[0] = 0; }   // no used value: min = max = 0
            __syncthreads();
            const uint32_t mn = scratch[0], mx = scratch[1], present = scratch[2];
            for (int v = tid; v < nv; v += BLOCK) {
                const uint32_t cur = cnt[v];
                double b;
                if (present == 0) b = 0.0;
                else {
                    double delta_boost;
                    if (mn == 0) delta_boost = -1.0;
                    else delta_boost = (double)(int)(mn - cur) / (double)mn;
                    if (cur != mn) b = delta_boost;
                    else if (mn == mx) b = -1.0;
                    else if (mn == 0) b = 1.0;
                    else b = (double)(int)(mx - mn) / (double)mn;
                }
                tb[v] = b;
            }
            __syncthreads();
        } else {
            for (int v = tid; v < nv; v += BLOCK) {
                const double desired = t.pset_desired[p][v];
                double b;
                if (desired != desired) b = -1.0;   // no target and no implicit "*"
                else {
                    const double used = (double)(cnt[v] + 1u);
                    b = ((desired - used) / desired) * t.pset_weight_frac[p];
                }
                tb[v] = b;
            }
        }
    }
    __syncthreads();
}

template <int BLOCK>
struct LoopShared {
    uint32_t scratch[4];
    uint32_t wave_a[BLOCK / 64];
    uint32_t wave_b[BLOCK / 64];
    double red_score[BLOCK / 64];
    int red_pos[BLOCK / 64];
    double aside_score[kMaxSkip];   // LimitIterator skip list
    int aside_pos[kMaxSkip];
    int stop_j;
    SweepRec red_rec[BLOCK / 64];   // full-pass mode: per-wave records
};

template <int BLOCK>
__device__ __forceinline__ void block_sync() {
    if constexpr (BLOCK > 64) __syncthreads();
}

// Ordering point for a single-wave workgroup: one wave's LDS operations execute
// in program order, so a wavefront-scope fence (a compiler barrier, no waits)
// is all the cross-lane hand-off through LDS needs. Unlike __syncthreads it
// does not drain outstanding global stores.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m, int lane) {
    return (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// Exclusive block prefix of a predicate; *total = block count.
template <int BLOCK>
__device__ __forceinline__ uint32_t block_prefix(bool pred, uint32_t* wave_tot, uint32_t* total) {
    const int lane = threadIdx.x & 63;
    const uint64_t m = __ballot(pred);
    if constexpr (BLOCK == 64) {
        *total = (uint32_t)__popcll(m);
        return lanes_below(m, lane);
    } else {
        constexpr int W = BLOCK / 64;
        const int wid = threadIdx.x >> 6;
        if (lane == 0) wave_tot[wid] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < W; w++) {
            const uint32_t x = wave_tot[w];
            before += (w < wid) ? x : 0u;
            tot += x;
        }
        __syncthreads();
        *total = tot;
        return before + lanes_below(m, lane);
    }
}

// first strict maximum: max score, ties -> smallest position
template <int BLOCK>
__device__ __forceinline__ void block_argmax(bool cand, double score, int pos, double* red_score, int* red_pos,
                                             double* best_score, int* best_pos) {
    double s = cand ? score : -__builtin_inf();
    int p = cand ? pos : 0x7FFFFFFF;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double os = __shfl_xor(s, off);
        const int op = __shfl_xor(p, off);
        if (os > s || (os == s && op < p)) { s = os; p = op; }
    }
    if constexpr (BLOCK == 64) {
        *best_score = s;
        *best_pos = p;
    } else {
        constexpr int W = BLOCK / 64;
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
        if (lane == 0) { red_score[wid] = s; red_pos[wid] = p; }
        __syncthreads();
        double bs = red_score[0];
        int bp = red_pos[0];
#pragma unroll
        for (int w = 1; w < W; w++) {
            const double os = red_score[w];
            const int op = red_pos[w];
            if (os > bs || (os == bs && op < bp)) { bs = os; bp = op; }
        }
        *best_score = bs;
        *best_pos = bp;
        __syncthreads();
    }
}

// Plan.AppendAlloc into the overlay (one lane).
__device__ __forceinline__ void commit_overlay(const NodeSoA& s, const TgTables& t, const Overlay& ov,
                                               uint32_t* counts, uint32_t row) {
    ov_add(ov, row);
    if (t.n_psets > 0) {
        const uint32_t c = s.rec[row].cls;
        for (int p = 0; p < t.n_psets; p++) {
            const uint32_t v = pset_value(t, p, row, c);
            if (v != kMissing) counts[t.pset_cnt_off[p] + v] += 1;
        }
    }
}

// TaskResources device offers of the chosen node (one lane).
__device__ __forceinline__ void record_offers(const NodeSoA& s, const Ask& a, const TgTables& t, uint32_t row,
                                              uint32_t dk, pe_ranked_node* o) {
    o->n_device_offers = 0;
    o->n_preempted = 0;
    if (a.n_dev <= 0) return;
    const DevClass& dc = t.dev_cls[s.rec[row].cls];
    uint32_t fr = dev_after(a, dc, t.dev_free[row], dk);
    double m;
    uint32_t groups[kMaxDevReq];
    if (!dev_assign(a, dc, fr, &m, groups)) return;
    o->n_device_offers = (uint32_t)a.n_dev;
    for (int q = 0; q < kMaxDevReq; q++)
        if (q < a.n_dev) o->device_offer_group[q] = groups[q];
}

// Result records of placement `it` of evaluation e (one lane).
template <bool kCores = true>
__device__ __forceinline__ void emit_placement(const BatchArgs& A, const uint8_t* class_ok, const Overlay& ov,
                                            const double* spread_tab, uint32_t e, uint32_t it, int win_row,
                                            double best_score, uint32_t consumed, uint32_t n_filtered,
                                            uint32_t n_exhausted, uint32_t new_offset) {
    if (A.full_out) {
        pe_ranked_node& o = A.full_out[(size_t)e * A.count + it];
        o.row = win_row;
        o.nodes_evaluated = consumed;
        o.nodes_filtered = n_filtered;
        o.nodes_exhausted = n_exhausted;
        o.new_offset = new_offset;
        o.final_score = 0.0;
        o.n_scores = 0;
        o.n_preempted = 0;
        o.n_device_offers = 0;
        for (int k = 0; k < PE_MAX_SCORES; k++) o.scores[k] = 0.0;
        if (win_row >= 0) {
            NodeEval ev;
            eval_node<true, kCores>(A.soa, A.tg, class_ok, A.ask, ov, A.penalty_bits, A.log10, spread_tab,
                                    (uint32_t)win_row, &ev);
            o.final_score = ev.score;
            o.n_scores = ev.nscores;
            for (int k = 0; k < (int)ev.nscores && k < PE_MAX_SCORES; k++) o.scores[k] = ev.parts[k];
            record_offers(A.soa, A.ask, A.tg, (uint32_t)win_row, ov_count(ov, (uint32_t)win_row), &o);
        }
    }
    if (A.out) {
        pe_placement& o = A.out[(size_t)e * A.count + it];
        o.row = win_row;
        o.nodes_evaluated = consumed;
        o.final_score = win_row >= 0 ? best_score : 0.0;
    }
}

// ---- full-pass reduction records (LimitIterator with limit >= options) -------
__host__ __device__ __forceinline__ void rec_init(SweepRec& r) {
    r.max_score = -__builtin_inff();
    for (int i = 0; i < 4; i++) r.max_rank[i] = 0xFFFFFFFFu;
    for (int i = 0; i < kMaxSkip; i++) { r.np_rank[i] = 0xFFFFFFFFu; r.np_score[i] = 0.0; }
    r.options = r.filtered = r.exhausted = r._pad = 0;
}

// insert x into a sorted list of N ranks (keeps the N smallest); branch-free on indices
template <int N>
__host__ __device__ __forceinline__ void ins_rank(uint32_t (&l)[N], uint32_t x) {
#pragma unroll
    for (int i = 0; i < N; i++) {
        const uint32_t lo = l[i] < x ? l[i] : x, hi = l[i] < x ? x : l[i];
        l[i] = lo;
        x = hi;
    }
}

__host__ __device__ __forceinline__ void ins_np(uint32_t (&rk)[kMaxSkip], double (&sc)[kMaxSkip], uint32_t x, double s) {
#pragma unroll
    for (int i = 0; i < kMaxSkip; i++) {
        if (x < rk[i]) {
            const uint32_t tr = rk[i]; const double ts = sc[i];
            rk[i] = x; sc[i] = s;
            x = tr; s = ts;
        }
    }
}

__device__ __forceinline__ void rec_add(SweepRec& r, uint32_t rank, double score) {
    r.options++;
    if (score > r.max_score) {
        r.max_score = score;
        r.max_rank[0] = rank;
        r.max_rank[1] = r.max_rank[2] = r.max_rank[3] = 0xFFFFFFFFu;
    } else if (score == r.max_score) {
        ins_rank<4>(r.max_rank, rank);
    }
    if (score <= 0.0) ins_np(r.np_rank, r.np_score, rank, score);
}

__host__ __device__ __forceinline__ void rec_merge(SweepRec& a, const SweepRec& b) {
    if (b.max_score > a.max_score) {
        a.max_score = b.max_score;
        for (int i = 0; i < 4; i++) a.max_rank[i] = b.max_rank[i];
    } else if (b.max_score == a.max_score) {
        for (int i = 0; i < 4; i++) ins_rank<4>(a.max_rank, b.max_rank[i]);
    }
    for (int i = 0; i < kMaxSkip; i++) ins_np(a.np_rank, a.np_score, b.np_rank[i], b.np_score[i]);
    a.options += b.options;
    a.filtered += b.filtered;
    a.exhausted += b.exhausted;
}

// Winner rank of a merged record, ~0u = no option.
__device__ __host__ __forceinline__ uint32_t rec_winner(const SweepRec& r) {
    if (r.options == 0) return 0xFFFFFFFFu;
    if (r.max_score > 0.0) return r.max_rank[0];
    for (int i = 0; i < 4; i++) {
        const uint32_t x = r.max_rank[i];
        if (x == 0xFFFFFFFFu) break;
        bool demoted = false;
        for (int k = 0; k < kMaxSkip; k++) demoted = demoted || r.np_rank[k] == x;
        if (!demoted) return x;
    }
    return r.max_rank[0];
}

__device__ __forceinline__ SweepRec rec_shfl_xor(const SweepRec& r, int off) {
    SweepRec o;
    o.max_score = __shfl_xor(r.max_score, off);
#pragma unroll
    for (int i = 0; i < 4; i++) o.max_rank[i] = (uint32_t)__shfl_xor((int)r.max_rank[i], off);
#pragma unroll
    for (int i = 0; i < kMaxSkip; i++) {
        o.np_rank[i] = (uint32_t)__shfl_xor((int)r.np_rank[i], off);
        o.np_score[i] = __shfl_xor(r.np_score[i], off);
    }
    o.options = (uint32_t)__shfl_xor((int)r.options, off);
    o.filtered = (uint32_t)__shfl_xor((int)r.filtered, off);
    o.exhausted = (uint32_t)__shfl_xor((int)r.exhausted, off);
    o._pad = 0;
    return o;
}

// Block reduction of per-thread records; the merge is commutative and
// associative over disjoint row sets, so an xor butterfly inside each wave is
// exact. Thread 0 returns the block's record.
template <int BLOCK>
__device__ __forceinline__ void rec_block_reduce(SweepRec& r, SweepRec* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const SweepRec o = rec_shfl_xor(r, off);
        rec_merge(r, o);
    }
    constexpr int W = BLOCK / 64;
    if constexpr (W > 1) {
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
        if (lane == 0) red[wid] = r;
        __syncthreads();
        if (threadIdx.x == 0)
            for (int w = 1; w < W; w++) rec_merge(r, red[w]);
    }
}

// Merge an evaluation's overlay into the HBM SoA (the stack's plan persists).
template <int BLOCK, bool FULL, bool kCores = true>
__device__ void writeback_overlay(const BatchArgs& A, const Overlay& ov, uint32_t H, const uint32_t* counts) {
    for (uint32_t h = threadIdx.x; h < H; h += BLOCK) {
        const uint32_t e = ov.keys[h];
        if (e == kEmpty) continue;
        const uint32_t row = ov.k ? e : e >> ov.kshift;
        const uint32_t k = ov.k ? ov.k[h] : e & ov.kmask;
        NodeRec& r = A.soa.rec[row];
        if (kCores) {
            r.used_cpu += (int64_t)k * ask_cpu(A.soa, A.ask, row);
            core_take(A.soa, A.ask, row, k);
        } else {
            r.used_cpu += (int64_t)k * A.ask.cpu;
        }
        r.used_mem += (int64_t)k * A.ask.mem;
        r.used_disk += (int64_t)k * A.ask.disk;
        r.used_mbits += (int32_t)k * A.ask.commit_mbits;
        r.used_dyn += (int32_t)k * A.ask.commit_dyn;
        A.soa.coll_job[row] += k;
        A.tg.coll_tg[row] += k;
        if (A.ask.n_dev > 0) A.tg.dev_free[row] = dev_after(A.ask, A.tg.dev_cls[r.cls], A.tg.dev_free[row], k);
    }
    if constexpr (FULL) {
        for (int q = 0; q < A.tg.n_psets; q++)
            for (int v = threadIdx.x; v < A.tg.pset_nvals[q]; v += BLOCK)
                A.tg.pset_counts[q][v] = counts[A.tg.pset_cnt_off[q] + v];
    }
}

template <int BLOCK, bool FULL, bool CORES>
__global__ void __launch_bounds__(BLOCK) k_place(BatchArgs A) {
    __shared__ LoopShared<BLOCK> sh;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
    const int tid = threadIdx.x;
    const uint32_t e = blockIdx.x;
    const uint32_t n = A.n_visit;
    const uint32_t* perm = A.perms + (size_t)e * A.perm_stride;
    const uint8_t* class_ok = A.tg.class_ok + (size_t)e * A.class_ok_stride;

    // carve the overlay (and spread tables) out of dynamic LDS
    const uint32_t H = 1u << A.hash_bits;
    unsigned char* p = dyn_smem;
    double* spread_tab = nullptr;
    uint32_t* counts = nullptr;
    if constexpr (FULL) {
        if (A.pset_g_tab) {   // tables beyond the LDS budget: this evaluation's HBM copy
            spread_tab = A.pset_g_tab + (size_t)e * A.tg.pset_tab_total;
            counts = A.pset_g_cnt + (size_t)e * A.tg.pset_cnt_total;
        } else {
            spread_tab = reinterpret_cast<double*>(p);
            counts = reinterpret_cast<uint32_t*>(p + sizeof(double) * A.tg.pset_tab_total);
            p += A.pset_lds;
        }
    }
    Overlay ov;
    ov.bits = A.hash_bits;
    ov.mask = H - 1;
    ov.keys = reinterpret_cast<uint32_t*>(p); p += 4 * H;
    ov.k = reinterpret_cast<uint32_t*>(p); p += 4 * H;
    for (uint32_t i = tid; i < H; i += BLOCK) ov.keys[i] = kEmpty;
    if constexpr (FULL) {
        for (int q = 0; q < A.tg.n_psets; q++)
            for (int v = tid; v < A.tg.pset_nvals[q]; v += BLOCK) counts[A.tg.pset_cnt_off[q] + v] = A.tg.pset_counts[q][v];
    }
    __syncthreads();

    uint32_t offset = A.offsets ? A.offsets[e] : A.offset0;
    if (n) offset %= n;
    uint32_t placed = 0;

    for (uint32_t it = 0; it < A.count; it++) {
        if constexpr (FULL) {
            if (A.tg.n_psets > 0) build_spread_table<BLOCK>(A.tg, counts, spread_tab, sh.scratch);
        }
        uint32_t r = 0, a = 0;            // returned / set-aside options so far
        double best_score = -__builtin_inf();
        int best_pos = -1;                // relative visit position of the winner
        uint32_t n_filtered = 0, n_exhausted = 0;
        uint32_t consumed = n;
        bool stopped = false;

        if (FULL && A.limit >= n) {
            // A full pass (limit >= every option): no prefix walk,
            // each lane folds its positions into a SweepRec, one block reduction
            // per placement gives the winner and the counters.
            SweepRec rec;
            rec_init(rec);
            for (uint32_t j = tid; j < n; j += BLOCK) {
                uint32_t pos = offset + j;
                if (pos >= n) pos -= n;
                NodeEval ev;
                eval_node<false, CORES>(A.soa, A.tg, class_ok, A.ask, ov, A.penalty_bits, A.log10, spread_tab, perm[pos], &ev);
                if (ev.status == kFiltered) rec.filtered++;
                else if (ev.status == kExhausted) rec.exhausted++;
                else rec_add(rec, j, ev.score);
            }
            rec_block_reduce<BLOCK>(rec, sh.red_rec);
            if (tid == 0) {
                const uint32_t w = rec_winner(rec);
                sh.stop_j = w == 0xFFFFFFFFu ? -1 : (int)w;
                sh.scratch[0] = rec.filtered;
                sh.scratch[1] = rec.exhausted;
                sh.red_score[0] = rec.max_score;   // the winner always scores the maximum
            }
            __syncthreads();
            best_pos = sh.stop_j;
            best_score = sh.red_score[0];
            n_filtered = sh.scratch[0];
            n_exhausted = sh.scratch[1];
            consumed = n;
            stopped = true;   // nothing set aside to append
            __syncthreads();
        }

        for (uint32_t base = 0; base < n && !(FULL && A.limit >= n); base += BLOCK) {
            const uint32_t j = base + tid;
            const bool valid = j < n;
            NodeEval ev;
            ev.status = kFiltered;
            ev.score = 0.0;
            if (valid) {
                uint32_t pos = offset + j;
                if (pos >= n) pos -= n;
                const uint32_t row = perm[pos];
                eval_node<false, CORES>(A.soa, A.tg, class_ok, A.ask, ov, A.penalty_bits, A.log10, spread_tab, row, &ev);
            }
            const bool is_opt = valid && ev.status == kOption;
            const bool is_np = is_opt && ev.score <= 0.0;
            uint32_t np_tot;
            const uint32_t np_before = a + block_prefix<BLOCK>(is_np, sh.wave_a, &np_tot);
            const bool aside = is_np && np_before < (uint32_t)kMaxSkip;
            const bool ret = is_opt && !aside;
            uint32_t ret_tot;
            const uint32_t ret_before = r + block_prefix<BLOCK>(ret, sh.wave_b, &ret_tot);
            // the limit-th returned option ends the pull
            const bool is_stop = ret && ret_before == A.limit - 1u;
            const uint64_t sm = __ballot(is_stop);
            int stop_j;
            if constexpr (BLOCK == 64) {
                stop_j = sm ? (int)__ffsll((long long)sm) - 1 : -1;
            } else {
                if (tid == 0) sh.stop_j = -1;
                __syncthreads();
                if (is_stop) sh.stop_j = tid;
                __syncthreads();
                stop_j = sh.stop_j;
            }
            const bool pulled = valid && (stop_j < 0 || tid <= stop_j);
            if (aside && pulled) {
                sh.aside_score[np_before] = ev.score;
                sh.aside_pos[np_before] = (int)j;
            }
            const bool cand = ret && ret_before < A.limit;
            double cs;
            int cp;
            block_argmax<BLOCK>(cand, ev.score, (int)j, sh.red_score, sh.red_pos, &cs, &cp);
            if (cp != 0x7FFFFFFF && cs > best_score) { best_score = cs; best_pos = cp; }
            uint32_t f_tot, e_tot, a_tot;
            block_prefix<BLOCK>(pulled && ev.status == kFiltered, sh.wave_a, &f_tot);
            block_prefix<BLOCK>(pulled && ev.status == kExhausted, sh.wave_b, &e_tot);
            block_prefix<BLOCK>(aside && pulled, sh.wave_a, &a_tot);
            n_filtered += f_tot;
            n_exhausted += e_tot;
            a += a_tot;
            if (stop_j >= 0) {
                consumed = base + (uint32_t)stop_j + 1u;
                r = A.limit;
                stopped = true;
                break;
            }
            r += ret_tot;
        }
        block_sync<BLOCK>();
        if (!stopped) {
            // source exhausted: set-aside options are emitted in order until the limit
            const uint32_t take = min(a, A.limit - r);
            for (uint32_t i = 0; i < take; i++) {
                if (sh.aside_score[i] > best_score) { best_score = sh.aside_score[i]; best_pos = sh.aside_pos[i]; }
            }
        }
        int win_row = -1;
        if (best_pos >= 0) {
            uint32_t pos = offset + (uint32_t)best_pos;
            if (pos >= n) pos -= n;
            win_row = (int)perm[pos];
        }
        uint32_t no = n ? offset + (consumed % n) : 0u;
        if (no >= n) no -= n;
        if (tid == 0) {
            emit_placement<CORES>(A, class_ok, ov, spread_tab, e, it, win_row, best_score, consumed, n_filtered,
                           n_exhausted, no);
            if (win_row >= 0 && A.commit) commit_overlay(A.soa, A.tg, ov, counts, (uint32_t)win_row);
        }
        offset = no;
        __syncthreads();
        if (win_row < 0) break;   // nil option: failedTGAllocs short-circuit
        placed++;
    }
    if (tid == 0) {
        A.eval_status[2 * e] = placed;
        A.eval_status[2 * e + 1] = offset;
    }
    if (A.writeback) writeback_overlay<BLOCK, FULL, CORES>(A, ov, H, counts);
}

// Windowed count loop (limit < n: no affinities or spreads, so a node's result
// depends only on the snapshot and its own overlay count). One wave per
// evaluation. Each placement pulls ~limit + filtered positions but a wave
// evaluates 64 at a time, so the wave keeps a 128-position ring of evaluated
// visit positions in registers (slot s of lane l = ring index 64 s + l) and
// evaluates a chunk only when the pull runs past the cache. Committing the
// winner changes only that node's overlay count: the cache is cut at the first
// cached position holding the winner's row (only reachable when the visit list
// wraps inside the ring, n < 128). Chunks are aligned to the ring so every lane
// reads its own registers; the LimitIterator / MaxScoreIterator closed form is
// the same ballot logic as k_place.
__global__ void __launch_bounds__(64) k_window(BatchArgs A) {
    __shared__ double aside_score[kMaxSkip];
    __shared__ int aside_pos[kMaxSkip];
    __shared__ pe_placement stage[64];
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
    const int lane = threadIdx.x;
    const uint32_t e = blockIdx.x;
    const uint32_t n = A.n_visit;
    const uint32_t* perm = A.perms + (size_t)e * A.perm_stride;
    const uint8_t* class_ok = A.tg.class_ok + (size_t)e * A.class_ok_stride;
    const uint32_t H = 1u << A.hash_bits;
    Overlay ov;
    ov.bits = A.hash_bits;
    ov.mask = H - 1;
    ov.keys = reinterpret_cast<uint32_t*>(dyn_smem);
    ov.k = A.packed_overlay ? nullptr : ov.keys + H;
    ov.kshift = A.packed_overlay;
    ov.kmask = A.packed_overlay ? (1u << A.packed_overlay) - 1u : 0u;
    for (uint32_t i = lane; i < H; i += 64) ov.keys[i] = kEmpty;
    __syncthreads();

    uint32_t offset = A.offsets ? A.offsets[e] : A.offset0;
    if (n) offset %= n;
    uint32_t placed = 0;
    int st0 = kFiltered, st1 = kFiltered;
    double sc0 = 0.0, sc1 = 0.0;
    uint32_t rw0 = kEmpty, rw1 = kEmpty;
    uint32_t rb = 0;     // ring index of the cursor
    uint32_t have = 0;   // relative positions [0, have) are cached (have <= min(n, 128) at loop top)

    for (uint32_t it = 0; it < A.count; it++) {
        uint32_t r = 0, a = 0;
        double best_score = -__builtin_inf();
        int best_pos = -1;
        uint32_t n_filtered = 0, n_exhausted = 0;
        uint32_t consumed = n;
        bool stopped = false;
        double lbest_s = -__builtin_inf();
        int lbest_p = -1;
        const uint32_t skew = rb & 63u;
        for (uint32_t k = 0; 64u * k < n + skew; k++) {
            const int j = (int)(64u * k + (uint32_t)lane) - (int)skew;   // relative visit position
            const bool valid = j >= 0 && (uint32_t)j < n;
            const bool s1 = (((rb >> 6) + k) & 1u) != 0;
            int st = s1 ? st1 : st0;
            double sc = s1 ? sc1 : sc0;
            const bool need = valid && (uint32_t)j >= have;
            if (__ballot(need)) {
                // The pull ran past the cache: evaluate this chunk and the next
                // one (every position >= have is uncached), all loads in flight
                // before any compute.
                const uint32_t j2 = (uint32_t)(j + 64);
                const bool need2 = j2 < n;
                uint32_t p1 = need ? offset + (uint32_t)j : 0u;
                uint32_t p2 = need2 ? offset + j2 : 0u;
                if (p1 >= n) p1 -= n;
                if (p2 >= n) p2 -= n;
                const uint32_t row1 = perm[p1], row2 = perm[p2];
                NodeIn in1, in2;
                load_node(A.soa, A.tg, row1, in1);
                load_node(A.soa, A.tg, row2, in2);
                const uint32_t dk1 = ov_count(ov, row1), dk2 = ov_count(ov, row2);
                NodeEval e1, e2;
                e1.score = 0.0;
                e2.score = 0.0;
                eval_loaded<false>(A.soa, A.tg, class_ok, A.ask, dk1, A.penalty_bits, A.log10, nullptr, row1, in1,
                                   &e1);
                eval_loaded<false>(A.soa, A.tg, class_ok, A.ask, dk2, A.penalty_bits, A.log10, nullptr, row2, in2,
                                   &e2);
                if (need) {
                    st = e1.status;
                    sc = e1.score;
                    if (s1) { st1 = st; sc1 = sc; rw1 = row1; } else { st0 = st; sc0 = sc; rw0 = row1; }
                }
                if (need2) {
                    if (s1) { st0 = e2.status; sc0 = e2.score; rw0 = row2; }
                    else { st1 = e2.status; sc1 = e2.score; rw1 = row2; }
                }
                have = min(64u * (k + 2) - skew, n);
            }

            const bool is_opt = valid && st == kOption;
            const bool is_np = is_opt && sc <= 0.0;
            uint32_t np_tot;
            const uint32_t np_before = a + block_prefix<64>(is_np, nullptr, &np_tot);
            const bool aside = is_np && np_before < (uint32_t)kMaxSkip;
            const bool ret = is_opt && !aside;
            uint32_t ret_tot;
            const uint32_t ret_before = r + block_prefix<64>(ret, nullptr, &ret_tot);
            const uint64_t sm = __ballot(ret && ret_before == A.limit - 1u);
            const int stop_lane = sm ? (int)__ffsll((long long)sm) - 1 : 64;
            const bool pulled = valid && lane <= stop_lane;
            if (aside && pulled) {
                aside_score[np_before] = sc;
                aside_pos[np_before] = j;
            }
            // lane-local first strict maximum; positions grow with the chunk,
            // so one wave reduction per placement suffices
            if (ret && ret_before < A.limit && sc > lbest_s) { lbest_s = sc; lbest_p = j; }
            if (A.full_out) {
                n_filtered += (uint32_t)__popcll(__ballot(pulled && st == kFiltered));
                n_exhausted += (uint32_t)__popcll(__ballot(pulled && st == kExhausted));
            }
            a += (uint32_t)__popcll(__ballot(aside && pulled));
            if (sm) {
                consumed = 64u * k + (uint32_t)stop_lane - skew + 1u;
                r = A.limit;
                stopped = true;
                break;
            }
            r += ret_tot;
        }
        {
            double cs;
            int cp;
            block_argmax<64>(lbest_p >= 0, lbest_s, lbest_p, nullptr, nullptr, &cs, &cp);
            if (cp != 0x7FFFFFFF) { best_score = cs; best_pos = cp; }
        }
        if (!stopped) {
            const uint32_t take = min(a, A.limit - r);
            for (uint32_t i = 0; i < take; i++) {
                if (aside_score[i] > best_score) { best_score = aside_score[i]; best_pos = aside_pos[i]; }
            }
        }
        int win_row = -1;
        if (best_pos >= 0) {
            if (best_pos + 128 >= (int)have) {
                // still in the ring: positions [have - 128, have) are intact
                const uint32_t idx = (rb + (uint32_t)best_pos) & 127u;
                win_row = __shfl((int)((idx & 64u) ? rw1 : rw0), (int)(idx & 63u));
            } else {
                uint32_t pos = offset + (uint32_t)best_pos;
                if (pos >= n) pos -= n;
                win_row = (int)perm[pos];
            }
        }
        uint32_t no = n ? offset + (consumed % n) : 0u;
        if (no >= n) no -= n;
        if (lane == 0) {
            if (A.full_out)
                emit_placement(A, class_ok, ov, nullptr, e, it, win_row, best_score, consumed, n_filtered,
                               n_exhausted, no);
            if (A.aside_out) *A.aside_out = a;
            pe_placement& o = stage[it & 63u];
            o.row = win_row;
            o.nodes_evaluated = consumed;
            o.final_score = win_row >= 0 ? best_score : 0.0;
            if (win_row >= 0 && A.commit) ov_add(ov, (uint32_t)win_row);
        }
        wave_sync();
        // compact records leave in 1 KB wave stores (possibly straight into
        // mapped host memory, so the transfer overlaps the count loop)
        if (A.out && ((it & 63u) == 63u || win_row < 0 || it + 1 == A.count)) {
            const uint32_t fill = (it & 63u) + 1u;
            if ((uint32_t)lane < fill)
                A.out[(size_t)e * A.count + (it + 1u - fill) + lane] = stage[lane];
        }
        offset = no;
        // slide the cache: a full pass (no stop) leaves the cursor in place but
        // the ring is keyed by unwrapped position, so it restarts empty
        if (stopped) {
            rb = (rb + consumed) & 127u;
            have = have > consumed ? have - consumed : 0u;
        } else {
            have = 0;
        }
        if (win_row >= 0 && A.commit && have) {
            const uint32_t j0 = ((uint32_t)lane - rb) & 127u, j1 = (64u + (uint32_t)lane - rb) & 127u;
            const bool bad0 = j0 < have && rw0 == (uint32_t)win_row;
            const bool bad1 = j1 < have && rw1 == (uint32_t)win_row;
            if (__ballot(bad0 || bad1)) {
                uint32_t cut = min(bad0 ? j0 : 128u, bad1 ? j1 : 128u);
                for (int off = 32; off > 0; off >>= 1) cut = min(cut, (uint32_t)__shfl_xor((int)cut, off));
                if (cut < have) have = cut;
            }
        }
        wave_sync();
        if (win_row < 0) break;
        placed++;
    }
    if (lane == 0) {
        A.eval_status[2 * e] = placed;
        A.eval_status[2 * e + 1] = offset;
    }
    if (A.writeback) writeback_overlay<64, false>(A, ov, H, nullptr);
}

// ---- shared base table ----------------------------------------------------------
__device__ __forceinline__ double encode_eval(const NodeEval& ev) {
    return ev.status == kOption ? ev.score : (ev.status == kFiltered ? -__builtin_inf() : __builtin_inf());
}

// base[row]: the fused pipeline of every row of the snapshot with no placement
// of this launch on it. It does not depend on the visit order, so one pass
// serves every evaluation of a batch. base1 (one placement on the row) is
// computed by a second set of lanes rather than after base in the same lane:
// the pass is one dependent load + evaluate chain per lane, so the two tables
// finish in the time of one; 64-lane workgroups spread it over more CUs. The
// two lanes of one position are neighbours in a wave, so the row's column
// lines are fetched once for both (halves in separate workgroups landed on
// separate XCDs and fetched every line twice).
// With FOLD the launch also carries the FeasibilityWrapper fold (FoldArgs):
// each workgroup pulls the class verdict table from the staging ring into LDS,
// the grid stores node_feas for every row (the later kernels read it), and the
// evaluation reads the verdict from the table (no dependency on another
// workgroup's stores). FoldArgs::list_covers: the visit list is a permutation
// of the table, so the main loop's dk == 0 lane stores its row's node_feas and
// no separate pass over the table runs.
constexpr int kBaseBlock = 64;
static_assert(kBaseBlock == 64, "k_base's bitmaps: one wave per workgroup, 32 positions x 2 tables");

// bits 0, 2, 4, .. of x packed into the low 32 bits
__device__ __forceinline__ uint32_t even_bits(uint64_t x) {
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return (uint32_t)x;
}

// WIDE: the launch is armed for the wide phases (BatchArgs::wide) and stores
// their bitmaps; a launch that is not runs the kernel without that code.
template <bool FOLD, bool WIDE = false>
__global__ void __launch_bounds__(kBaseBlock) k_base(BatchArgs A) {
    __shared__ uint8_t cls_ok[FOLD ? kFoldMaxClasses : 1];
    const uint32_t stride = gridDim.x * kBaseBlock;
    // the tables straight from the kernel arguments: a local copy of TgTables
    // (its per-set arrays are indexed at run time) lived in scratch, 680 B per
    // lane written and read back by every launch
    const TgTables& tg = A.tg;
    const uint8_t* class_ok = A.tg.class_ok;
    auto fold_ok = [&](uint32_t row, uint32_t c) {
        bool ok = c < A.fold.ncls && cls_ok[c] != 0;
        if (A.fold.node_ok) ok = ok && A.fold.node_ok[row] != 0;
        return ok;
    };
    const uint32_t m = A.base_by_pos ? A.n_visit : A.soa.n;
    const uint32_t sh = A.base1 ? 1u : 0u;
    const uint32_t total = m << sh;
    const uint32_t first = blockIdx.x * kBaseBlock + threadIdx.x;
    // the row of position t >> sh (a staged list is read over the bus)
    auto row_of = [&](uint32_t t) {
        const uint32_t j = t >> sh;
        if (!A.base_by_pos) return j;
        return A.perm_src ? A.perm_src[j] : A.perms[j];
    };
    // the row's reads but the verdict (FOLD takes it from the LDS table)
    auto load_row = [&](uint32_t row, NodeIn& in) {
        in.r = A.soa.rec[row];
        in.coll_tg = tg.coll_tg[row];
        in.dev_free = tg.dev_free ? tg.dev_free[row] : 0u;
    };
    uint32_t row = 0;
    NodeIn in;
    if (FOLD) {
        // The lane's first position is in flight while the class table comes
        // over the bus: its list entry is requested before the table, its row's
        // reads as soon as the entry is there, and nothing waits for them
        // before the evaluation.
        const FoldArgs& F = A.fold;
        if (first < total) row = row_of(first);
        uint8_t v0 = 0;
        if (threadIdx.x < F.ncls) v0 = F.class_src[threadIdx.x];
        if (first < total) load_row(row, in);
        if (threadIdx.x < F.ncls) {
            cls_ok[threadIdx.x] = v0;
            if (blockIdx.x == 0) F.class_dst[threadIdx.x] = v0;
        }
        for (uint32_t c = threadIdx.x + kBaseBlock; c < F.ncls; c += kBaseBlock) {
            const uint8_t v = F.class_src[c];
            cls_ok[c] = v;
            if (blockIdx.x == 0) F.class_dst[c] = v;
        }
        __syncthreads();
        // node_feas of every row: by the main loop below when the list is a
        // permutation of the table (it holds each row's record and verdict
        // once), else by a pass over the table
        if (!F.list_covers)
            for (uint32_t r = first; r < A.soa.n; r += stride)
                F.feas[r] = fold_ok(r, A.soa.rec[r].cls) ? 1 : 0;
        class_ok = cls_ok;
    }
    for (uint32_t t = first; t < total; t += stride) {
        const uint32_t dk = t & sh;
        const uint32_t j = t >> sh;
        if (FOLD) {   // the verdict from the LDS table: other workgroups are still storing node_feas
            if (t != first) {
                row = row_of(t);
                load_row(row, in);
            }
            in.feas = fold_ok(row, in.r.cls) ? 1u : 0u;
            if (A.fold.list_covers && !dk) A.fold.feas[row] = (uint8_t)in.feas;
        } else {
            row = row_of(t);
            load_node(A.soa, tg, row, in);
        }
        if (A.base_by_pos && A.perm_src && !dk) A.perm_dst[j] = row;
        NodeEval ev;
        ev.score = 0.0;
        eval_loaded<false, false>(A.soa, tg, class_ok, A.ask, dk, A.penalty_bits, A.log10, nullptr, row, in, &ev);
        const double v = encode_eval(ev);
        (dk ? A.base1 : A.base)[j] = v;
        if (WIDE) {
            // the wide phases' bitmaps by visit position: a wave holds 32
            // positions, the two tables' lanes interleaved (a lane past the
            // list's end is not in the ballot, so the last word ends in zeros)
            const bool is_o = v > -__builtin_inf() && v < __builtin_inf();
            const uint64_t bo = __ballot(is_o), bf = __ballot(v == -__builtin_inf()),
                           bn = __ballot(is_o && v <= 0.0);
            const uint32_t w = (t - threadIdx.x) >> 6, nw = A.wide.words;
            if (threadIdx.x == 0 && sh && w < nw) {
                uint32_t* b = A.wide.bits + w;
                b[0] = even_bits(bo);
                b[nw] = even_bits(bo >> 1);
                b[2 * nw] = even_bits(bf);
                b[3 * nw] = even_bits(bf >> 1);
                b[4 * nw] = even_bits(bn);
                b[5 * nw] = even_bits(bn >> 1);
                A.wide.won[w] = 0u;
                A.wide.won[nw + w] = 0u;
                if (w == 0) *A.wide.err = 0u;
            }
        }
    }
}

// ---- windowed count loop: phase-static selection ------------------------------
//
// Windowed binpack (limit = ceil(log2 n) < n; no affinity or spread) of one
// evaluation. The value of visit position T (FinalScore, or filtered /
// exhausted) depends only on the row there and on how many of this
// evaluation's placements that row holds. A visit list without repeated rows
// shows a row again only n positions later, and every Select's winner lies
// behind the next Select's start, so once the cursor is at c the values of all
// positions [c, c + n) (one rotation) are fixed: no Select that stops inside
// that window can change them. A *phase* therefore:
//   1. evaluates the n positions in parallel: base[row] (shared, k_base) or the
//      row re-evaluated with its placement count from the LDS overlay;
//   2. scans option / non-positive-option (N) counts into option indices and
//      nb[k] = N options before option k;
//   3. resolves the Select boundaries serially but in O(1) per Select: a Select
//      starting at option i returns every positive option and every N after its
//      third, so it stops at option i + L - 1 + m for the smallest m in {0,1,2}
//      with exactly m N's in [i, i + L - 1 + m], else at i + L + 2
//      (LimitIterator, select.go:35-74);
//   4. finds every Select's winner at once (first strict maximum over its
//      returned options: LDS atomicMax on an order-preserving key, then
//      atomicMin on the option index) and commits the winners to the overlay
//      (distinct rows within a phase, so the inserts are independent).
// The next phase starts after the last stop. A Select that cannot stop inside
// the window ends the phase early; if it is the phase's first one it has seen
// the whole list: the stream is exhausted, set-aside options are appended
// (at most `limit` in total) and the cursor stays (feasible.go:90-107).
// One record of a deferred-record k_chain launch: the full Select result of
// the entry, evaluated on the state the launch started from (the entry's dk =
// placements of the launch on the row before it).
__device__ __forceinline__ void build_emit_rec(const BatchArgs& A, const ChainEmit& m, EmitRec& o) {
    o.row = m.row;
    o.nodes_evaluated = m.consumed;
    o.nodes_filtered = m.filtered;
    o.nodes_exhausted = m.exhausted;
    o.new_offset = m.new_offset;
    o.final_score = 0.0;
    o.n_scores = 0;
    o.n_device_offers = 0;
    o.flags = 0;
    for (int q = 0; q < PE_MAX_SCORES; q++) o.scores[q] = 0.0;
    for (int q = 0; q < PE_MAX_DEVICE_REQ; q++) o.device_offer_group[q] = 0;
    if (m.row < 0) return;
    const uint32_t row = (uint32_t)m.row;
    if (A.fused_parts && m.dk == 0 && m.pos != PE_NONE && A.ask.n_dev == 0) {
        // the row's first-phase evaluation (its state at the launch's start)
        const uint32_t np = A.fused_nparts[m.pos];
        o.final_score = m.score;
        o.n_scores = np;
        for (int q = 0; q < PE_MAX_SCORES; q++)
            if (q < (int)np) o.scores[q] = A.fused_parts[(size_t)m.pos * PE_MAX_SCORES + q];
        return;
    }
    NodeIn in;
    load_node(A.soa, A.tg, row, in);
    NodeEval ev;
    ev.score = 0.0;
    eval_loaded<true, false>(A.soa, A.tg, A.tg.class_ok, A.ask, m.dk, A.penalty_bits, A.log10, nullptr, row, in, &ev);
    o.final_score = ev.score;
    o.n_scores = ev.nscores;
    for (int q = 0; q < PE_MAX_SCORES; q++) if (q < (int)ev.nscores) o.scores[q] = ev.parts[q];
    if (A.ask.n_dev > 0) {
        const DevClass& dc = A.tg.dev_cls[A.soa.rec[row].cls];
        uint32_t fr = dev_after(A.ask, dc, A.tg.dev_free[row], m.dk);
        double mm;
        uint32_t groups[kMaxDevReq];
        if (dev_assign(A.ask, dc, fr, &mm, groups)) {
            o.n_device_offers = (uint32_t)A.ask.n_dev;
            for (int q = 0; q < kMaxDevReq; q++)
                if (q < A.ask.n_dev) o.device_offer_group[q] = (uint16_t)groups[q];
        }
    }
}

constexpr int kChainBlock = 1024;
constexpr int kChainItems = 16;                               // positions per lane of the largest shape
constexpr uint32_t kChainMaxN = kChainBlock * kChainItems;   // positions per phase held in registers (largest shape)
#ifndef PE_CHAIN_LOAD_BATCH
#define PE_CHAIN_LOAD_BATCH 4
#endif
constexpr int kChainLoadBatch = PE_CHAIN_LOAD_BATCH;          // window values a lane loads per memory round trip
constexpr int kChainMaxSel = 1024;                            // Selects resolved per phase
constexpr uint32_t kChainMaxRedo = 2048;                      // rows re-evaluated per phase (<= placements per launch)

enum : int { kPhaseMore = 0, kPhaseCount = 1, kPhaseExhausted = 2, kPhaseStall = 3, kPhaseRetry = 4 };
constexpr uint32_t kChainStalled = 0x80000000u;   // eval_status cursor flag: continue with the lazy loop
constexpr int kSegE = 21;                 // entry offsets into a segment: a Select spans <= limit + 3 options
constexpr uint32_t kSegLen = 256;         // options per segment of the boundary walk
constexpr uint32_t kMaxChainLimit = kSegE - 3;
constexpr uint16_t kNxFail = 0xFFFF;      // the Select starting at this option cannot stop in the window
constexpr uint32_t kExFail = 0xFF;
// k_chain error flags (eval_status cursor word, beside kChainStalled): an
// index the shape's arrays do not cover. The kernel stops the evaluation
// instead of storing out of bounds and the host fails the call.
constexpr uint32_t kChainError = 0x40000000u;

// Per-instantiation shape of k_chain: ITEMS visit positions per lane, so one
// phase covers kMaxN = 1024 * ITEMS positions. Every array and loop bound below
// derives from it, including the wave-0 tile scan (kScanPer tiles per lane,
// at least one: a shape with fewer than 64 tiles still scans all of them).
template <int ITEMS>
struct ChainShape {
    static constexpr int kItems = ITEMS;
    static constexpr uint32_t kMaxN = (uint32_t)kChainBlock * ITEMS;
    static constexpr int kTiles = (int)(kMaxN / 64);
    static constexpr int kSegs = (int)((kMaxN + kSegLen - 1) / kSegLen);
    static constexpr int kScanPer = (kTiles + 63) / 64;
    static_assert(kScanPer * 64 >= kTiles, "the tile scan covers every tile");
    static_assert(kMaxN <= kChainMaxN, "the host sizes scratch for the largest shape");
    static_assert(kMaxN % 32 == 0, "position bitmaps");
};

template <int ITEMS>
struct ChainShared {
    using Shp = ChainShape<ITEMS>;
    uint32_t tile_o[Shp::kTiles], tile_n[Shp::kTiles];    // per 64-position tile counts, then exclusive offsets
    uint32_t sel_b[kChainMaxSel];                          // option index of each Select's stop
    uint32_t sel_end[kChainMaxSel];                        // its visit position (relative to the phase start)
    unsigned long long sel_max[kChainMaxSel];              // order-preserving key of the max returned score,
                                                           // then the winner's FinalScore bits
    uint32_t sel_arg[kChainMaxSel];                        // option index of the first maximum
    uint32_t sel_row[kChainMaxSel];                        // the winner's row
    uint32_t sel_f[kChainMaxSel], sel_x[kChainMaxSel];     // filtered / exhausted positions (metrics)
    uint32_t seg_tab[Shp::kSegs][kSegE];                  // per segment and entry offset: count | exit << 16
    uint16_t seg_entry[Shp::kSegs], seg_base[Shp::kSegs];
    uint2 redo[kChainMaxRedo];                             // (row, placements) to re-evaluate; then the value
    uint16_t sel_pos[kChainMaxSel];                        // the winner's visit position (relative)
    // visit positions (mod n) whose row holds >= 1 / >= 2 placements of this
    // launch: later phases find their values without probing the overlay
    uint32_t bm1[Shp::kMaxN / 32], bm2[Shp::kMaxN / 32];
    double aside_v[kMaxSkip];
    uint32_t aside_row[kMaxSkip];
    uint32_t tot_o, tot_n, nsel, mode, n_redo, n_seg, slow, n_emit, n_ov;
    uint32_t err;                                          // a bounds guard tripped (kChainError)
};

__host__ __device__ __forceinline__ unsigned long long order_key(double x) {
    const unsigned long long b = (unsigned long long)gm::f2u(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ uint32_t wrap_pos(uint32_t x, uint32_t n) {
    if (x < n) return x;
    x -= n;
    return x < n ? x : x % n;
}

// Plan.AppendAlloc into the overlay from many threads at once; the rows are
// distinct, so no two threads race on one key.
__device__ __forceinline__ uint32_t ov_add_atomic(const Overlay& o, uint32_t row) {
    uint32_t h = ov_hash(o, row);
    if (!o.k) {
        const uint32_t fresh = (row << o.kshift) | 1u;
        for (;;) {
            uint32_t e = o.keys[h];
            if (e == kEmpty) {
                e = atomicCAS(&o.keys[h], kEmpty, fresh);
                if (e == kEmpty) return h;
            }
            if ((e >> o.kshift) == row) { atomicAdd(&o.keys[h], 1u); return h; }
            h = (h + 1) & o.mask;
        }
    }
    for (;;) {
        uint32_t key = o.keys[h];
        if (key == kEmpty) {
            key = atomicCAS(&o.keys[h], kEmpty, row);
            if (key == kEmpty) { atomicAdd(&o.k[h], 1u); return h; }
        }
        if (key == row) { atomicAdd(&o.k[h], 1u); return h; }
        h = (h + 1) & o.mask;
    }
}

// first index s in [0, cnt) with a[s] >= x (a ascending; cnt if none)
__device__ __forceinline__ uint32_t lower_bound_lds(const uint32_t* a, uint32_t cnt, uint32_t x) {
    uint32_t lo = 0, hi = cnt;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Register state per position q of a thread: option index (14 bits) and, until
// the Select ids are known, the N-option prefix (14 bits); afterwards the
// Select id (10 bits) in the high half.
constexpr uint32_t kIdxBits = 14, kIdxMask = (1u << kIdxBits) - 1u;

// Optional step profile (PE_CHAIN_PROF): thread 0 accumulates shader clocks
// per step into A.prof[phase * 8 + step] (phases 0..3, the last one
// accumulating the rest); marks follow the block barriers. Step 0 of phase 0
// includes the kernel's start and the overlay initialisation.
#define PE_PROF_MARK(k)                                                   \
    do {                                                                  \
        if (A.prof && tid == 0) {                                         \
            const uint64_t now_ = __builtin_readcyclecounter();           \
            A.prof[prof_ph * 8 + (k)] += now_ - prof_t;                   \
            prof_t = now_;                                                \
        }                                                                 \
    } while (0)


// The chain's rare heavy paths out of line: inlined, the table and ask fields
// they read were hoisted to the kernel's start and held (spilled) for its
// whole run.
__device__ __noinline__ void chain_emit_full(const BatchArgs& A, Overlay ov, uint32_t e, uint32_t it, int win_row,
                                             double score, uint32_t consumed, uint32_t f, uint32_t x, uint32_t next_off) {
    emit_placement<false>(A, A.tg.class_ok, ov, nullptr, e, it, win_row, score, consumed, f, x, next_off);
}

// The FUSED first phase's evaluation of visit position p: its value, and its
// score parts into A.fused_parts (the records of winners without an earlier
// placement of the launch copy them)
__device__ __noinline__ double chain_eval_parts(const BatchArgs& A, uint32_t row, uint32_t p) {
    NodeIn in;
    load_node(A.soa, A.tg, row, in);
    NodeEval ev;
    ev.score = 0.0;
    eval_loaded<true, false>(A.soa, A.tg, A.tg.class_ok, A.ask, 0u, A.penalty_bits, A.log10, nullptr, row, in, &ev);
    if (ev.status == kOption) {
        A.fused_nparts[p] = (uint8_t)ev.nscores;
        for (int q = 0; q < PE_MAX_SCORES; q++) A.fused_parts[(size_t)p * PE_MAX_SCORES + q] = ev.parts[q];
    }
    return encode_eval(ev);
}

// value of (row, placements) re-evaluated: the k_base pipeline with dk placements
__device__ __noinline__ double chain_reeval(const BatchArgs& A, uint32_t row, uint32_t dk) {
    NodeIn in;
    load_node(A.soa, A.tg, row, in);
    NodeEval ev;
    ev.score = 0.0;
    eval_loaded<false, false>(A.soa, A.tg, A.tg.class_ok, A.ask, dk, A.penalty_bits, A.log10, nullptr, row, in, &ev);
    return encode_eval(ev);
}

// Step 5 of k_chain (out of line: its loads would otherwise raise the whole
// kernel's register pressure).
template <class Sh>
__device__ __noinline__ void chain_walk(Sh& sh, const uint16_t* nb, const double* vs, const uint32_t* perm,
                                        uint32_t cur, uint32_t n, uint32_t nsel, int tid) {
    for (uint32_t s = (uint32_t)tid; s < nsel; s += kChainBlock) {
        const uint32_t p0 = s ? (uint32_t)nb[sh.sel_b[s - 1]] + 1u : 0u;
        const uint32_t p1 = nb[sh.sel_b[s]];
        uint32_t n_aside = 0, f = 0, x = 0;
        int bp = -1;
        double best = 0.0;
        for (uint32_t pb = p0; pb <= p1; pb += 8u) {
            double y[8];
#pragma unroll
            for (int k = 0; k < 8; k++) y[k] = vs[min(pb + (uint32_t)k, p1)];   // one round of loads
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if (pb + (uint32_t)k > p1) break;
                const double yk = y[k];
                if (yk == -__builtin_inf()) { f++; continue; }
                if (yk == __builtin_inf()) { x++; continue; }
                if (yk <= 0.0 && n_aside < (uint32_t)kMaxSkip) { n_aside++; continue; }
                if (bp < 0 || yk > best) { best = yk; bp = (int)(pb + (uint32_t)k); }
            }
        }
        if (bp < 0) {   // every Select returns at least one option past its set-aside ones
            sh.err = 1u;
            bp = (int)p1;
        }
        sh.sel_end[s] = p1;
        sh.sel_pos[s] = (uint16_t)bp;
        sh.sel_max[s] = (unsigned long long)gm::f2u(best);
        sh.sel_row[s] = perm[wrap_pos(cur + (uint32_t)bp, n)];
        sh.sel_f[s] = f;
        sh.sel_x[s] = x;
    }
}

// Row patches (pe_update_nodes): payload = rows[n] then n rows of `words`
// 4-byte words each, read from the mapped staging; dst row r gets its row.
__global__ void __launch_bounds__(256) k_scatter_rows(uint32_t* dst, uint32_t words, const uint32_t* payload,
                                                      uint32_t n) {
    const uint64_t total = (uint64_t)n * words;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const uint32_t i = (uint32_t)(t / words), w = (uint32_t)(t % words);
        dst[(uint64_t)payload[i] * words + w] = payload[n + t];
    }
}

// Per-node count arrays from a sorted sparse list (key = row << 5 | array,
// value = count): each thread owns one row, zeroes it in every array and
// writes the row's entries found by binary search. A deferred ResetPlan (R.rec)
// rides along: its arrays are disjoint from the counts.
// `first` / `stride`: this thread's first index and the launch's thread count.
__device__ __forceinline__ void counts_apply(const CountDsts& D, uint32_t nd, uint32_t n, const uint2* ents,
                                             uint32_t m, const ResetArgs& R, uint32_t first, uint32_t stride) {
    if (R.rec) {
        for (uint32_t i = first; i < R.n; i += stride) {
            R.rec[i] = R.base_rec[i];
            R.dev_free[i] = R.dev_free_base[i];
        }
        for (uint32_t i = first; i < R.m; i += stride) R.preempted[i] = 0;
        for (uint32_t i = first; i < R.keys; i += stride) R.pcount[i] = 0;
    }
    for (uint32_t row = first; row < n; row += stride) {
        uint32_t lo = 0, hi = m;
        const uint32_t k0 = row << 5;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (ents[mid].x < k0) lo = mid + 1;
            else hi = mid;
        }
        for (uint32_t d = 0; d < nd; d++) {
            if (!D.d[d]) continue;
            uint32_t v = 0;
            if (lo < m && ents[lo].x == (k0 | d)) v = ents[lo++].y;
            D.d[d][row] = v;
        }
    }
}

// FUSED (short lists of one evaluation, BatchArgs::fused): no k_base, k_emit
// or k_emit_writeback launch; the kernel carries the fold (FoldArgs), evaluates
// its first phase's positions itself (storing them as the base table of the
// later phases, whose rows with placements are re-evaluated: no base1), builds
// the records into the mapped output, writes the placements back and raises
// done_flag[0].
constexpr uint32_t kFusedMaxClasses = 4096;
// WIDE (BatchArgs::wide armed, not FUSED): the kernel starts from what the wide
// phase launches resolved (ChainSeed); every other launch runs without that code.
template <int ITEMS, bool FUSED, bool WIDE = false>
__global__ void __launch_bounds__(kChainBlock) k_chain(BatchArgs A, uint32_t n_evals) {
    static_assert(!(FUSED && WIDE), "the wide phases precede the unfused chain only");
    using Shp = ChainShape<ITEMS>;
    static_assert(Shp::kMaxN <= (1u << kIdxBits), "option index packing");
    static_assert(kChainMaxSel <= (1 << (32 - 2 * kIdxBits + kIdxBits)), "select id packing");
    __shared__ ChainShared<ITEMS> sh;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n = A.n_visit;
    // positions per phase: one rotation, or its first Shp::kMaxN positions on a
    // longer list (every Select of the phase still stops inside the window)
    const uint32_t Wfull = n < Shp::kMaxN ? n : Shp::kMaxN;
    const uint32_t L = A.limit;
    const uint32_t H = 1u << A.hash_bits;
    // A in the kernel-argument segment, for the out-of-line helpers (taking the
    // parameter's address would copy the whole struct to scratch)
    const BatchArgs& Ak = *(const BatchArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    Overlay ov;
    ov.bits = A.hash_bits;
    ov.mask = H - 1;
    ov.keys = reinterpret_cast<uint32_t*>(dyn_smem);
    ov.k = A.packed_overlay ? nullptr : ov.keys + H;
    ov.kshift = A.packed_overlay;
    ov.kmask = A.packed_overlay ? (1u << A.packed_overlay) - 1u : 0u;
    uint16_t* nb = reinterpret_cast<uint16_t*>(ov.keys + (A.packed_overlay ? H : 2 * H));   // [n + 2]
    uint16_t* nx = nb + ((Wfull + 2 + 1) & ~1u);   // [W + 2]: next Select start per option, then Select id per option

    // what the wide phase launches resolved before this one (none: placed 0)
    ChainSeed seed;
    seed.status = kSeedDeclined;
    seed.placed = seed.cur = seed.pos_used = 0;
    if (WIDE) {
        seed = A.wide.seed[A.wide.phases - 1];
        const bool werr = *A.wide.err != 0u || seed.placed > A.count || seed.cur >= (n ? n : 1u);
        if (werr || seed.placed == A.count) {
            // a guard of k_phase tripped (the host fails the call), or the
            // count is reached: the records and the writeback entries are there
            if (tid == 0) {
                A.eval_status[0] = werr ? 0u : seed.placed;
                A.eval_status[1] = werr ? kChainError : seed.cur;
                A.emit_n[0] = werr ? 0u : seed.placed;
                A.emit_n[1] = werr || !A.writeback ? 0u : seed.placed;
            }
            return;
        }
    }
    uint64_t prof_t = A.prof ? __builtin_readcyclecounter() : 0;
    int prof_ph = 0;   // profile slot group: phase (capped at 3)
    if (FUSED && A.counts.nd) {
        // SetJob's collision counts (and the deferred ResetPlan copy) carried
        // by this launch instead of a k_counts launch of their own
        const CountArgs& C = A.counts;
        counts_apply(C.D, C.nd, C.n, C.ents, C.m, C.R, (uint32_t)tid, kChainBlock);
        __syncthreads();
    }
    if (FUSED && A.fold.feas) {
        // the FeasibilityWrapper fold of every row, before any evaluation
        __shared__ uint8_t fcls[FUSED ? kFusedMaxClasses : 1];
        const FoldArgs& F = A.fold;
        for (uint32_t c = tid; c < F.ncls; c += kChainBlock) {
            const uint8_t v = F.class_src[c];
            fcls[c] = v;
            F.class_dst[c] = v;
        }
        __syncthreads();
        for (uint32_t row = tid; row < A.soa.n; row += kChainBlock) {
            const uint32_t c = A.soa.rec[row].cls;
            bool ok = c < F.ncls && fcls[c] != 0;
            if (F.node_ok) ok = ok && F.node_ok[row] != 0;
            F.feas[row] = ok ? 1 : 0;
        }
        __syncthreads();
    }
    for (uint32_t e = blockIdx.x; e < n_evals; e += gridDim.x) {
        const uint32_t* __restrict__ perm = A.perms + (size_t)e * A.perm_stride;
        double* __restrict__ vs = A.chain_vs + (size_t)blockIdx.x * kChainMaxN;   // values by relative position
        for (uint32_t i = tid; i < H; i += kChainBlock) {
            ov.keys[i] = kEmpty;
            if (ov.k) ov.k[i] = 0;
        }
        for (uint32_t i = tid; i < Shp::kMaxN / 32; i += kChainBlock) {
            sh.bm1[i] = 0;
            sh.bm2[i] = 0;
        }
        if (tid == 0) {
            sh.slow = n > Shp::kMaxN ? 1u : 0u;   // the position bitmaps cover one window of the list
            sh.n_emit = 0;
            sh.err = 0;
        }
        uint32_t cur = wrap_pos(A.offsets ? A.offsets[e] : A.offset0, n);
        uint32_t placed = 0;
        bool stalled = false;
        bool done = n == 0 || A.count == 0;
        uint32_t pos_used = 0;      // visit positions the resolved Selects consumed so far
        bool force_full = false;    // a shortened window held no whole Select: use the full one
        if (n == 0 && A.count && tid == 0 && A.out) {
            pe_placement& o = A.out[(size_t)e * A.count];
            o.row = -1; o.nodes_evaluated = 0; o.final_score = 0.0;
        }
        __syncthreads();
        if (WIDE && seed.placed) {
            // the wide phases' placements into the overlay and the position
            // bitmaps, from their records; the phase loop goes on after them
            for (uint32_t i = tid; i < seed.placed; i += kChainBlock) {
                const int32_t r = A.emit[i].row;
                const uint32_t p = A.emit[i].pos;
                if (r < 0 || p >= n || n > Shp::kMaxN) {
                    sh.err = 1u;
                    continue;
                }
                ov_add_atomic(ov, (uint32_t)r);
                const uint32_t bit = 1u << (p & 31);
                if (atomicOr(&sh.bm1[p >> 5], bit) & bit) atomicOr(&sh.bm2[p >> 5], bit);
            }
            placed = seed.placed;
            cur = seed.cur;
            pos_used = seed.pos_used;
            if (tid == 0) sh.n_emit = placed;
            __syncthreads();
        }
        while (!done) {
            PE_PROF_MARK(0);
            // positions of this phase: the full window, or after the first
            // phase what the remaining Selects need at the observed positions
            // per Select with a margin (the per-position steps scale with it)
            uint32_t W = Wfull;
            if (placed && !force_full) {
                const uint64_t need = (uint64_t)(A.count - placed) * pos_used * 3u / (2u * placed) + 1024u;
                if (need < W) W = (uint32_t)((need + kChainBlock - 1) / kChainBlock * kChainBlock);
                if (W > Wfull) W = Wfull;
            }
            force_full = false;
            // items a lane holds this phase (wave-uniform): the rest lie past the window
            const int qn = (int)((W + kChainBlock - 1) / kChainBlock);
            // 1. values of the window [cur, cur + n): base (no placement of this
            //    launch on the row), base1 (one), or queued for re-evaluation
            if (tid == 0) sh.n_redo = 0;
            // rows holding placements of this launch: one (base1) from the
            // position bitmaps, two or more re-evaluated (ov_count)
            const bool use_bm = placed && sh.slow == 0;
            uint32_t optmask = 0, nmask = 0, redo_mask = 0;   // bit q: option / non-positive option / re-evaluate
            {
                // rows are read only where the value needs them: every position
                // without the bitmaps (overlay probes) or for a row-indexed base,
                // else none (the first phase reads base, later ones base / base1
                // by position and re-evaluate the bitmaps' rows from the list)
                const bool rows_all = !A.base_by_pos || (placed && !use_bm);
                uint32_t row[ITEMS];
#pragma unroll
                for (int q = 0; q < ITEMS; q++) row[q] = 0u;   // a valid index where the position is not read
#pragma unroll
                for (int q = 0; q < ITEMS; q++) {
                    if (q >= qn) break;
                    const uint32_t j = (uint32_t)(q * kChainBlock + tid);
                    row[q] = rows_all && j < W ? perm[wrap_pos(cur + j, n)] : 0u;
                }
                uint32_t one_mask = 0;
                if (placed) {
#pragma unroll
                    for (int q = 0; q < ITEMS; q++) {
                        if (q >= qn) break;
                        const uint32_t j = (uint32_t)(q * kChainBlock + tid);
                        if (j < W) {
                            uint32_t b1 = 1, b2 = 1;
                            if (use_bm) {
                                const uint32_t p = wrap_pos(cur + j, n), bit = 1u << (p & 31);
                                b1 = sh.bm1[p >> 5] & bit;
                                b2 = sh.bm2[p >> 5] & bit;
                                if (b1 && (b2 || !A.base1)) redo_mask |= 1u << q;
                                else if (b1) one_mask |= 1u << q;
                            } else {
                                const uint32_t dk = ov_count(ov, row[q]);
                                if (dk == 1u && A.base1) one_mask |= 1u << q;
                                else if (dk) redo_mask |= 1u << q;
                            }
                        }
                    }
                }
                if (FUSED && !placed) {
#pragma unroll
                    for (int q = 0; q < ITEMS; q++) {
                        if (q >= qn) break;
                        const uint32_t j = (uint32_t)(q * kChainBlock + tid);
                        if (j < W && !((redo_mask >> q) & 1u)) {
                            // the first phase evaluates its positions (and
                            // stores the visit order when it came staged)
                            const uint32_t p = wrap_pos(cur + j, n);
                            uint32_t r;
                            if (A.perm_src) {
                                r = A.perm_src[p];
                                A.perm_dst[p] = r;
                            } else {
                                r = perm[p];
                            }
                            const double v = A.fused_parts ? chain_eval_parts(Ak, r, p) : chain_reeval(Ak, r, 0u);
                            A.base[p] = v;
                            vs[j] = v;   // read back by the Select walks of step 5 (after the barriers)
                            const bool is_o = v > -__builtin_inf() && v < __builtin_inf();
                            optmask |= (uint32_t)is_o << q;
                            nmask |= (uint32_t)(is_o && v <= 0.0) << q;
                        }
                    }
                } else {
                    // table reads in groups of kBatch: a group's loads are all
                    // issued before the first is consumed (one memory round
                    // trip per group, not per item). The index is clamped to
                    // the window's last position, so the loads need no guard;
                    // a position past the window or queued for re-evaluation
                    // drops its value.
                    constexpr int kBatch = kChainLoadBatch < ITEMS ? kChainLoadBatch : ITEMS;
                    // the lane's index as the compiler cannot see through it:
                    // the addresses vs + j of all ITEMS stores are otherwise
                    // loop-invariant, hoisted out of the phase loop and spilled
                    uint32_t ltid = (uint32_t)tid;
                    asm volatile("" : "+v"(ltid));
#pragma unroll
                    for (int g = 0; g < ITEMS; g += kBatch) {
                        if (g >= qn) break;
                        double v[kBatch];
#pragma unroll
                        for (int k = 0; k < kBatch; k++) {
                            const int q = g + k;
                            if (q >= ITEMS) break;
                            const uint32_t j = min((uint32_t)(q * kChainBlock) + ltid, W - 1u);
                            const double* src = ((one_mask >> q) & 1u) ? A.base1 : A.base;
                            uint32_t p = cur + j;   // cur < n and j < W <= n: one subtraction wraps it
                            if (p >= n) p -= n;
                            v[k] = src[A.base_by_pos ? p : row[q]];
                        }
                        // the whole group has landed here: a load still pending
                        // across the conditional stores below makes the next
                        // group wait for those stores' completion as well
#pragma unroll
                        for (int k = 0; k < kBatch; k++)
                            if (g + k < ITEMS) asm volatile("" : "+v"(v[k]));
#pragma unroll
                        for (int k = 0; k < kBatch; k++) {
                            const int q = g + k;
                            if (q >= ITEMS) break;
                            const uint32_t j = (uint32_t)(q * kChainBlock) + ltid;
                            if (j < W && !((redo_mask >> q) & 1u)) {
                                vs[j] = v[k];   // read back by the Select walks of step 5 (after the barriers)
                                const bool is_o = v[k] > -__builtin_inf() && v[k] < __builtin_inf();
                                optmask |= (uint32_t)is_o << q;
                                nmask |= (uint32_t)(is_o && v[k] <= 0.0) << q;
                            }
                        }
                    }
                }
            }
            if (__syncthreads_or(redo_mask != 0)) {
                // rows with placements of this launch the tables do not cover:
                // evaluated in parallel, the value stored at its window position
#pragma unroll
                for (int q = 0; q < ITEMS; q++) {
                    if (q >= qn) break;
                    if ((redo_mask >> q) & 1u) {
                        const uint32_t j = (uint32_t)(q * kChainBlock + tid);
                        const uint32_t r = perm[wrap_pos(cur + j, n)];
                        const uint32_t slot = atomicAdd(&sh.n_redo, 1u);
                        if (slot < kChainMaxRedo) sh.redo[slot] = make_uint2(r, ov_count(ov, r) | (j << 18));
                        else sh.err = 1u;
                    }
                }
                __syncthreads();
                const uint32_t nr = min(sh.n_redo, kChainMaxRedo);
                for (uint32_t w = tid; w < nr; w += kChainBlock) {
                    const uint2 rd = sh.redo[w];
                    vs[rd.y >> 18] = chain_reeval(Ak, rd.x, rd.y & 0x3FFFFu);
                }
                __syncthreads();
                if (sh.err) break;
                // the re-evaluated values back, in the same groups (every index
                // lies inside this workgroup's kChainMaxN doubles of vs)
                constexpr int kBatch = kChainLoadBatch < ITEMS ? kChainLoadBatch : ITEMS;
                uint32_t ltid = (uint32_t)tid;   // opaque, as in step 1: no hoisted address per item
                asm volatile("" : "+v"(ltid));
#pragma unroll
                for (int g = 0; g < ITEMS; g += kBatch) {
                    if (g >= qn) break;
                    double v[kBatch];
#pragma unroll
                    for (int k = 0; k < kBatch; k++) {
                        if (g + k >= ITEMS) break;
                        v[k] = vs[(uint32_t)((g + k) * kChainBlock) + ltid];
                    }
#pragma unroll
                    for (int k = 0; k < kBatch; k++)
                        if (g + k < ITEMS) asm volatile("" : "+v"(v[k]));
#pragma unroll
                    for (int k = 0; k < kBatch; k++) {
                        const int q = g + k;
                        if (q >= ITEMS) break;
                        if ((redo_mask >> q) & 1u) {
                            const bool is_o = v[k] > -__builtin_inf() && v[k] < __builtin_inf();
                            optmask |= (uint32_t)is_o << q;
                            nmask |= (uint32_t)(is_o && v[k] <= 0.0) << q;
                        }
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < ITEMS; q++) {
                if (q >= qn) break;
                const uint64_t bo = __ballot((optmask >> q) & 1u), bn = __ballot((nmask >> q) & 1u);
                if (lane == 0 && q * kChainBlock < (int)W) {
                    sh.tile_o[q * (kChainBlock / 64) + wave] = (uint32_t)__popcll(bo);
                    sh.tile_n[q * (kChainBlock / 64) + wave] = (uint32_t)__popcll(bn);
                }
            }
            for (uint32_t s = tid; s < kChainMaxSel; s += kChainBlock) {
                sh.sel_max[s] = 0ull;
                sh.sel_arg[s] = kEmpty;
                sh.sel_f[s] = 0;
                sh.sel_x[s] = 0;
            }
            __syncthreads();
            PE_PROF_MARK(1);
            // 2. exclusive scan of the tile counts (wave 0)
            const uint32_t ntiles = (W + 63) / 64;
            if (wave == 0) {
                constexpr int PER = Shp::kScanPer;
                uint32_t so = 0, sn = 0, lo[PER], ln[PER];
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    const uint32_t t = (uint32_t)(lane * PER + k);
                    lo[k] = t < ntiles ? sh.tile_o[t] : 0u;
                    ln[k] = t < ntiles ? sh.tile_n[t] : 0u;
                    so += lo[k];
                    sn += ln[k];
                }
                uint32_t io = so, in_ = sn;   // inclusive wave scan
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t xo = (uint32_t)__shfl_up((int)io, off), xn = (uint32_t)__shfl_up((int)in_, off);
                    if (lane >= off) { io += xo; in_ += xn; }
                }
                uint32_t eo = io - so, en = in_ - sn;
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    const uint32_t t = (uint32_t)(lane * PER + k);
                    if (t < ntiles) { sh.tile_o[t] = eo; sh.tile_n[t] = en; }
                    eo += lo[k];
                    en += ln[k];
                }
                if (lane == 63) { sh.tot_o = io; sh.tot_n = in_; }
            }
            __syncthreads();
            PE_PROF_MARK(2);
            // 3. option index and N prefix of every option; nb[k] = N options before option k
            uint32_t pk[ITEMS];
#pragma unroll
            for (int q = 0; q < ITEMS; q++) {
                if (q >= qn) break;
                const uint64_t bo = __ballot((optmask >> q) & 1u), bn = __ballot((nmask >> q) & 1u);
                const uint32_t t = (uint32_t)(q * (kChainBlock / 64) + wave);
                const bool live = (uint32_t)(q * kChainBlock) < W;
                const uint32_t k = (live ? sh.tile_o[t] : 0u) + lanes_below(bo, lane);
                const uint32_t nbk = (live ? sh.tile_n[t] : 0u) + lanes_below(bn, lane);
                pk[q] = (k & kIdxMask) | ((nbk & kIdxMask) << kIdxBits);
                if ((optmask >> q) & 1u) {
                    if (k < W) nb[k] = (uint16_t)nbk;
                    else sh.err = 1u;   // an option index past the window: the scan is wrong
                }
            }
            const uint32_t tot_o = sh.tot_o, tot_n = sh.tot_n;
            if (tid == 0) {
                if (tot_o <= W) nb[tot_o] = (uint16_t)tot_n;
                else sh.err = 1u;
            }
            __syncthreads();
            if (sh.err) break;   // stop the evaluation before any index built on the scan is used
            PE_PROF_MARK(3);
            // 4. Select boundaries. A Select starting at option i stops at option
            //    i + L - 1 + m for the smallest m in {0, 1, 2} with exactly m N's
            //    in [i, i + L - 1 + m], else at i + L + 2 (its third N is set aside
            //    and every later option returned). 4a: the next start nx[i] of every
            //    option in parallel; 4b: per 64-option segment and entry offset the
            //    Selects inside and the exit offset; 4c: one lane walks the
            //    segments; 4d: the Selects are written out in parallel.
            if (tot_n == 0) {
                // no non-positive option in the window: every Select returns
                // exactly L options (m = 0 above), so Select s stops at option
                // (s + 1) L - 1; nb takes the options' positions at once
#pragma unroll
                for (int q = 0; q < ITEMS; q++)
                    if (q < qn && ((optmask >> q) & 1u)) nb[pk[q] & kIdxMask] = (uint16_t)(q * kChainBlock + tid);
                if (tid == 0) {
                    const uint32_t want = min(A.count - placed, (uint32_t)kChainMaxSel);
                    const uint32_t fit = tot_o / L;
                    uint32_t ns = fit < want ? fit : want;
                    int fmode = kPhaseMore;
                    if (ns == 0 && W < Wfull) fmode = kPhaseRetry;
                    else if (ns == 0 && W < n) fmode = kPhaseStall;
                    else if (ns == 0) { fmode = kPhaseExhausted; ns = tot_o ? 1u : 0u; if (ns) sh.sel_b[0] = tot_o - 1; }
                    else if (ns == A.count - placed) fmode = kPhaseCount;
                    sh.nsel = ns;
                    sh.mode = (uint32_t)fmode;
                    sh.n_seg = 0;
                }
                __syncthreads();
                if (sh.mode == (uint32_t)kPhaseMore || sh.mode == (uint32_t)kPhaseCount)
                    for (uint32_t sel = tid; sel < sh.nsel; sel += kChainBlock) sh.sel_b[sel] = (sel + 1) * L - 1;
                __syncthreads();
            } else {
#pragma unroll
                for (int q = 0; q < ITEMS; q++) {
                    if (q >= qn) break;
                    if ((optmask >> q) & 1u) {
                        const uint32_t i = pk[q] & kIdxMask;
                        const uint32_t a0 = pk[q] >> kIdxBits;
                        uint32_t nxt = kNxFail;
                        if (i + L - 1 < tot_o) {
                            if (nb[min(i + L, tot_o)] - a0 == 0) nxt = i + L;
                            else if (i + L < tot_o) {
                                if (nb[i + L + 1] - a0 == 1) nxt = i + L + 1;
                                else if (i + L + 1 < tot_o) {
                                    if (nb[i + L + 2] - a0 == 2) nxt = i + L + 2;
                                    else if (i + L + 2 < tot_o) nxt = i + L + 3;
                                }
                            }
                        }
                        nx[i] = (uint16_t)nxt;
                    }
                }
                if (tid == 0) nx[tot_o] = kNxFail;
                __syncthreads();
                // nb is free from here on: the relative position of every option
#pragma unroll
                for (int q = 0; q < ITEMS; q++)
                    if (q < qn && ((optmask >> q) & 1u)) nb[pk[q] & kIdxMask] = (uint16_t)(q * kChainBlock + tid);
                const uint32_t n_seg = (tot_o + kSegLen - 1) / kSegLen;
                const uint32_t E = L + 3;
                for (uint32_t t = tid; t < n_seg * E; t += kChainBlock) {
                    const uint32_t g = t / E, o = t - g * E;
                    const uint32_t end = kSegLen * (g + 1);
                    uint32_t i = kSegLen * g + o, cnt = 0, ex = kExFail;
                    for (;;) {
                        if (i >= end) { ex = i - end; break; }
                        if (i >= tot_o) break;
                        const uint32_t x = nx[i];
                        if (x == kNxFail) break;
                        cnt++;
                        i = x;
                    }
                    sh.seg_tab[g][o] = cnt | (ex << 16);
                }
                __syncthreads();
                if (tid == 0) {
                    const uint32_t want = min(A.count - placed, (uint32_t)kChainMaxSel);
                    uint32_t total = 0, o = 0, used = 0;
                    for (uint32_t g = 0; g < n_seg; g++) {
                        const uint32_t te = sh.seg_tab[g][o], cnt = te & 0xFFFFu, ex = te >> 16;
                        sh.seg_entry[g] = (uint16_t)o;
                        sh.seg_base[g] = (uint16_t)total;
                        used = g + 1;
                        if (total + cnt >= want) { total = want; break; }
                        total += cnt;
                        if (ex == kExFail) break;
                        o = ex;
                    }
                    int mode = kPhaseMore;
                    uint32_t ns = total;
                    if (ns == 0 && W < Wfull) {
                        // the shortened window held no whole Select: again with the full one
                        mode = kPhaseRetry;
                        used = 0;
                    } else if (ns == 0 && W < n) {
                        // a Select needs more than the window: the lazy loop goes on from here
                        mode = kPhaseStall;
                        used = 0;
                    } else if (ns == 0) {
                        // the first Select saw the whole list without reaching the limit
                        mode = kPhaseExhausted;
                        ns = tot_o ? 1u : 0u;
                        if (ns) sh.sel_b[0] = tot_o - 1;
                        used = 0;
                    } else if (ns == A.count - placed) {
                        mode = kPhaseCount;
                    }
                    sh.nsel = ns;
                    sh.mode = (uint32_t)mode;
                    sh.n_seg = used;
                }
                __syncthreads();
                {
                    const uint32_t ns = sh.nsel, used = sh.n_seg;
                    for (uint32_t g = tid; g < used; g += kChainBlock) {
                        uint32_t i = kSegLen * g + sh.seg_entry[g], sel = sh.seg_base[g];
                        while (sel < ns && i < kSegLen * (g + 1)) {
                            const uint32_t x = nx[i];
                            sh.sel_b[sel++] = x - 1u;
                            i = x;
                        }
                    }
                }
                __syncthreads();
            }
            const uint32_t nsel = sh.nsel;
            const int mode = (int)sh.mode;
            if (mode == kPhaseStall) {
                stalled = true;
                break;
            }
            if (mode == kPhaseRetry) {
                force_full = true;
                continue;
            }
            PE_PROF_MARK(4);
            if (mode != kPhaseExhausted) {
                // 5. one thread per Select walks its positions (previous stop + 1
                //    .. its stop) in the scratch copy of the values: the first
                //    kMaxSkip non-positive options are set aside, MaxScoreIterator
                //    keeps the first strict maximum of the rest (select.go:79-116);
                //    filtered / exhausted positions are the Select's metrics
                chain_walk(sh, nb, vs, perm, cur, n, nsel, tid);
            } else {
                // the one Select of an exhausted stream: every option of the
                // window (atomics over one key), its first kMaxSkip N's set aside
                uint32_t retmask = 0;
#pragma unroll
                for (int q = 0; q < ITEMS; q++) {
                    if (q >= qn) break;
                    if ((optmask >> q) & 1u) {
                        const uint32_t j = (uint32_t)(q * kChainBlock + tid);
                        const double vq = vs[j];
                        const uint32_t nrank = pk[q] >> kIdxBits;   // N options before this one
                        const bool aside = ((nmask >> q) & 1u) && nrank < (uint32_t)kMaxSkip;
                        if (!aside) {
                            retmask |= 1u << q;
                            atomicMax(&sh.sel_max[0], order_key(vq));
                        } else {
                            sh.aside_v[nrank] = vq;
                            sh.aside_row[nrank] = perm[wrap_pos(cur + j, n)];
                        }
                    }
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < ITEMS; q++) {
                    if (q >= qn) break;
                    const uint32_t j = (uint32_t)(q * kChainBlock + tid);
                    if (((retmask >> q) & 1u) &&
                        order_key(vs[j]) == sh.sel_max[0])
                        atomicMin(&sh.sel_arg[0], pk[q] & kIdxMask);
                }
                if (A.full_out || A.emit) {
#pragma unroll
                    for (int q = 0; q < ITEMS; q++) {
                        if (q >= qn) break;
                        const uint32_t j = (uint32_t)(q * kChainBlock + tid);
                        if (j < W && !((optmask >> q) & 1u))
                            atomicAdd(vs[j] == -__builtin_inf()
                                          ? &sh.sel_f[0] : &sh.sel_x[0], 1u);
                    }
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < ITEMS; q++) {
                    if (q >= qn) break;
                    const uint32_t j = (uint32_t)(q * kChainBlock + tid);
                    if (((retmask >> q) & 1u) && sh.sel_arg[0] == (pk[q] & kIdxMask)) {
                        sh.sel_row[0] = perm[wrap_pos(cur + j, n)];
                        sh.sel_max[0] = (unsigned long long)gm::f2u(vs[j]);
                    }
                }
            }
            __syncthreads();
            if (sh.err) break;
            PE_PROF_MARK(5);
            // 6. emit the winners and commit them (Plan.AppendAlloc), one Select per thread
            if (mode != kPhaseExhausted) {
                for (uint32_t s = tid; s < nsel; s += kChainBlock) {
                    const uint32_t start = s ? sh.sel_end[s - 1] + 1u : 0u;
                    const uint32_t consumed = sh.sel_end[s] - start + 1u;
                    const int win_row = (int)sh.sel_row[s];
                    const double score = gm::u2f(sh.sel_max[s]);
                    const uint32_t it = placed + s;
                    const uint32_t next_off = wrap_pos(cur + sh.sel_end[s] + 1u, n);
                    if (it >= A.count) {   // nsel <= count - placed by construction
                        sh.err = 1u;
                        continue;
                    }
                    if (A.emit) {
                        ChainEmit& m = A.emit[it];
                        m.row = win_row;
                        m.pos = wrap_pos(cur + sh.sel_pos[s], n);
                        m.dk = ov_count(ov, (uint32_t)win_row);
                        m.consumed = consumed;
                        m.filtered = sh.sel_f[s];
                        m.exhausted = sh.sel_x[s];
                        m.new_offset = next_off;
                        m.score = score;
                    } else if (A.full_out) {
                        chain_emit_full(Ak, ov, e, it, win_row, score, consumed, sh.sel_f[s], sh.sel_x[s], next_off);
                    }
                    if (A.out) {
                        pe_placement& o = A.out[(size_t)e * A.count + it];
                        o.row = win_row;
                        o.nodes_evaluated = consumed;
                        o.final_score = score;
                    }
                }
                __syncthreads();   // the records read the overlay before the commits
                if (A.commit) {
                    for (uint32_t s = tid; s < nsel; s += kChainBlock) {
                        ov_add_atomic(ov, sh.sel_row[s]);
                        if (n <= Shp::kMaxN) {   // the bitmaps cover lists of one window only
                            const uint32_t p = wrap_pos(cur + sh.sel_pos[s], n), bit = 1u << (p & 31);
                            if (atomicOr(&sh.bm1[p >> 5], bit) & bit) atomicOr(&sh.bm2[p >> 5], bit);
                        }
                    }
                }
                if (tid == 0) sh.n_emit = placed + nsel;
                placed += nsel;
                pos_used += sh.sel_end[nsel - 1] + 1u;
                cur = wrap_pos(cur + sh.sel_end[nsel - 1] + 1u, n);
                done = mode == kPhaseCount;
            } else {
                // exhausted stream: returned options in order, then set-aside ones
                // until the limit (select.go:35-74); the cursor stays
                if (tid == 0) {
                    const uint32_t a = min(tot_n, (uint32_t)kMaxSkip);
                    const uint32_t r = tot_o - a;
                    double best = -__builtin_inf();
                    int win_row = -1;
                    if (nsel && r) { best = gm::u2f(sh.sel_max[0]); win_row = (int)sh.sel_row[0]; }
                    const uint32_t take = min(a, L > r ? L - r : 0u);
                    for (uint32_t k = 0; k < take; k++)
                        if (sh.aside_v[k] > best) { best = sh.aside_v[k]; win_row = (int)sh.aside_row[k]; }
                    if (A.emit) {
                        ChainEmit& m = A.emit[placed];
                        m.row = win_row;
                        m.pos = PE_NONE;
                        m.dk = win_row >= 0 ? ov_count(ov, (uint32_t)win_row) : 0u;
                        m.consumed = n;
                        m.filtered = sh.sel_f[0];
                        m.exhausted = sh.sel_x[0];
                        m.new_offset = cur;
                        m.score = best;
                    } else if (A.full_out) {
                        chain_emit_full(Ak, ov, e, placed, win_row, best, n, sh.sel_f[0], sh.sel_x[0], cur);
                    }
                    sh.n_emit = placed + 1;
                    sh.slow = 1;   // the winner's position is not tracked: later phases probe the overlay
                    if (A.out) {
                        pe_placement& o = A.out[(size_t)e * A.count + placed];
                        o.row = win_row;
                        o.nodes_evaluated = n;
                        o.final_score = win_row >= 0 ? best : 0.0;
                    }
                    if (win_row >= 0 && A.commit) ov_add(ov, (uint32_t)win_row);
                    sh.mode = win_row >= 0 ? 1u : 0u;
                }
                __syncthreads();
                if (sh.mode) placed++;
                else done = true;   // nil option: failedTGAllocs short-circuit
                if (placed >= A.count) done = true;
            }
            __syncthreads();
            PE_PROF_MARK(6);
            prof_ph = prof_ph < 3 ? prof_ph + 1 : 3;
        }
        __syncthreads();
        if (tid == 0) {
            A.eval_status[2 * e] = placed;
            A.eval_status[2 * e + 1] = cur | (stalled ? kChainStalled : 0u) | (sh.err ? kChainError : 0u);
        }
        if (FUSED) {
            // the records, on the state the launch started from, then the
            // placements into HBM, then the completion word
            __syncthreads();
            const uint32_t ne = min(sh.n_emit, A.count);
            for (uint32_t i = tid; i < ne; i += kChainBlock) build_emit_rec(Ak, A.emit[i], A.emit_out[i]);
            __syncthreads();
            if (A.writeback) writeback_overlay<kChainBlock, false, false>(A, ov, H, nullptr);
            __syncthreads();
            if (tid == 0 && A.done_flag) {
                __threadfence_system();
                __hip_atomic_store(A.done_flag, A.done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        } else if (A.emit) {
            // records and the HBM writeback are k_emit's: dump the overlay
            if (tid == 0) sh.n_ov = 0;
            __syncthreads();
            for (uint32_t h = tid; h < H; h += kChainBlock) {
                const uint32_t key = ov.keys[h];
                if (key == kEmpty) continue;
                const uint32_t r = ov.k ? key : key >> ov.kshift;
                const uint32_t kk = ov.k ? ov.k[h] : key & ov.kmask;
                const uint32_t slot = atomicAdd(&sh.n_ov, 1u);
                if (slot < A.count) A.emit_ov[slot] = make_uint2(r, kk);   // overlay rows <= placements
                else sh.err = 1u;
            }
            __syncthreads();
            if (tid == 0) {
                A.emit_n[0] = min(sh.n_emit, A.count);
                A.emit_n[1] = A.writeback ? min(sh.n_ov, A.count) : 0u;
                if (sh.err) A.eval_status[2 * e + 1] |= kChainError;
            }
        } else if (A.writeback) {
            writeback_overlay<kChainBlock, false, false>(A, ov, H, nullptr);   // no cores on the chain path
        }
        __syncthreads();
    }
}

constexpr uint32_t kEmitBlock = 64;

// Records of a single-evaluation k_chain launch (A.emit): the full Select
// result of every entry, evaluated on the state the launch started from (the
// entry's dk = placements on the row before it); k_emit_writeback then
// writes the launch's placements back to the HBM SoA.
__global__ void __launch_bounds__(kEmitBlock) k_emit(BatchArgs A) {
    // records are built in LDS and stored to the (host-mapped) output as one
    // contiguous run per workgroup: 8-byte coalesced stores of compact records
    // instead of every lane writing its own record field by field over the
    // bus; small workgroups spread the bus writes over more CUs
    __shared__ EmitRec recs[kEmitBlock];
    const uint32_t i = blockIdx.x * kEmitBlock + threadIdx.x;
    const uint32_t n_emit = min(A.emit_n[0], A.count);
    if (i < n_emit) build_emit_rec(A, A.emit[i], recs[threadIdx.x]);
    __syncthreads();
    {
        const uint32_t first = blockIdx.x * kEmitBlock;
        const uint32_t cnt = n_emit > first ? min(kEmitBlock, n_emit - first) : 0u;
        constexpr uint32_t W = sizeof(EmitRec) / 8;
        const uint2* src = reinterpret_cast<const uint2*>(recs);
        uint2* dst = reinterpret_cast<uint2*>(A.emit_out + first);
        for (uint32_t w = threadIdx.x; w < cnt * W; w += kEmitBlock) dst[w] = src[w];
    }
    if (!A.done_flag) return;
    __syncthreads();
    // every workgroup raises its own completion word once its records are out:
    // the spinning host checks them all (no ticket atomic round trip and one
    // system fence per workgroup instead of two)
    if (threadIdx.x == 0) {
        __threadfence_system();
        __hip_atomic_store(A.done_flag + blockIdx.x, A.done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The launch's placements written back to the HBM SoA, one overlay entry
// (row, placements) per thread; runs after k_emit on the stream (the records
// read the state the launch started from), off the host's critical path.
__global__ void __launch_bounds__(256) k_emit_writeback(BatchArgs A) {
    const uint32_t x = blockIdx.x * 256 + threadIdx.x;
    if (x >= A.emit_n[1]) return;
    const uint2 e = A.emit_ov[x];
    if (e.y == 0) return;   // a wide phase's second win of a row: counted in the first one's slot
    NodeRec& r = A.soa.rec[e.x];
    r.used_cpu += (int64_t)e.y * ask_cpu(A.soa, A.ask, e.x);
    core_take(A.soa, A.ask, e.x, e.y);
    r.used_mem += (int64_t)e.y * A.ask.mem;
    r.used_disk += (int64_t)e.y * A.ask.disk;
    r.used_mbits += (int32_t)e.y * A.ask.commit_mbits;
    r.used_dyn += (int32_t)e.y * A.ask.commit_dyn;
    A.soa.coll_job[e.x] += e.y;
    A.tg.coll_tg[e.x] += e.y;
    if (A.ask.n_dev > 0) A.tg.dev_free[e.x] = dev_after(A.ask, A.tg.dev_cls[r.cls], A.tg.dev_free[e.x], e.y);
}

// ---- wide phases: one rotation's Selects on many CUs ----------------------------
//
// Inside one phase of the chain the Selects do not depend on each other (the
// window's values are fixed at the phase's start, see above), and in the closed
// form (no non-positive option in the window) Select s returns exactly the
// options [s L, (s + 1) L) in visit order. All a Select needs beyond the values
// is the rank of every option: a prefix popcount over k_base's option bitmap,
// which every workgroup scans for itself (n / 32 words). k_phase(p) resolves
// phase p of the unfused single-evaluation chain, one Select per lane, and
// writes the ChainEmit entries k_chain's step 6 would write; k_chain then
// starts from ChainSeed and has nothing left to do when the count is reached.
// A phase the closed form does not cover is declined as a whole (nothing but
// the seed stored) and k_chain resolves it.
// Launch-to-launch state only: phase p reads seed[p - 1] and won[0] (phase 0's
// winners), stores seed[p] and won[p], so no workgroup reads what another
// workgroup of the same launch stores. emit_ov gets one slot per Select: a
// row's second win (phase 1 on a phase 0 winner) raises the first slot's count
// to two and leaves its own slot empty.
constexpr int kWideBlock = 64;
constexpr uint32_t kWideMaxWords = kChainMaxN / 32;
static_assert(kWideMaxWords % kWideBlock == 0, "k_phase: whole rounds of bitmap words per lane");

__device__ __forceinline__ void wide_fail(const ChainWide& Wd) { atomicOr(Wd.err, 1u); }

// set bits of the bitmap at absolute positions [0, p), p in [0, n]
__device__ __forceinline__ uint32_t wide_prefix(const uint32_t* pre, const uint32_t* bits, uint32_t nw, uint32_t p) {
    const uint32_t w = p >> 5;
    if (w >= nw) return pre[nw];
    return pre[w] + (uint32_t)__popc(bits[w] & ((1u << (p & 31u)) - 1u));
}

// position of the set bit of absolute rank r < pre[nw]; the word index and the
// word's bits from that one upwards in *w / *rest. False: no such bit.
__device__ __forceinline__ bool wide_select(const uint32_t* pre, const uint32_t* bits, uint32_t nw, uint32_t r,
                                            uint32_t* w, uint32_t* rest) {
    uint32_t lo = 0, hi = nw;   // first word index in [1, nw] whose prefix exceeds r, minus one
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre[mid + 1] <= r) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= nw) return false;
    uint32_t word = bits[lo];
    for (uint32_t k = r - pre[lo]; k; k--) word &= word - 1u;
    *w = lo;
    *rest = word;
    return word != 0u;
}

__global__ void __launch_bounds__(kWideBlock) k_phase(BatchArgs A, uint32_t phase) {
    __shared__ uint32_t s_opt[kWideMaxWords], s_fil[kWideMaxWords], s_won[kWideMaxWords];
    __shared__ uint32_t p_opt[kWideMaxWords + 1], p_fil[kWideMaxWords + 1];
    const ChainWide& Wd = A.wide;
    const uint32_t lane = threadIdx.x, n = A.n_visit, L = A.limit, nw = Wd.words;
    const bool first = blockIdx.x == 0 && lane == 0;   // the one lane that stores the seed
    if (phase > 1) return;   // a row holds at most one placement per phase: dk <= 1 below
    // One round of loads for everything the prologue reads: the lane's words
    // of every bitmap (index clamped to the last word, so no load needs a
    // guard) and, in phase 1, the seed (a vector load, one field per lane, so
    // it travels with the rest). All of them have landed at the pins below.
    constexpr int kPer = (int)(kWideMaxWords / kWideBlock);
    const bool args_ok = n != 0 && nw == (n + 31u) / 32u && nw <= kWideMaxWords && L != 0 && L <= kMaxChainLimit;
    uint32_t r_o[kPer], r_f[kPer], r_n[kPer], r_w[kPer], r_seed = 0;
#pragma unroll
    for (int i = 0; i < kPer; i++) r_o[i] = r_f[i] = r_n[i] = r_w[i] = 0u;
    if (args_ok) {
        if (phase) r_seed = reinterpret_cast<const uint32_t*>(Wd.seed + (phase - 1))[lane & 3u];
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            if ((uint32_t)i * kWideBlock >= nw) break;
            const uint32_t* b = Wd.bits + min(lane + (uint32_t)i * kWideBlock, nw - 1u);
            r_o[i] = b[0];
            r_f[i] = b[2 * nw];
            r_n[i] = b[4 * nw];
        }
        if (phase) {
            // table 1 where the row won in phase 0
            uint32_t t_o[kPer], t_f[kPer], t_n[kPer];
#pragma unroll
            for (int i = 0; i < kPer; i++) {
                t_o[i] = t_f[i] = t_n[i] = 0u;
                if ((uint32_t)i * kWideBlock >= nw) break;
                const uint32_t wc = min(lane + (uint32_t)i * kWideBlock, nw - 1u);
                const uint32_t* b = Wd.bits + wc;
                r_w[i] = Wd.won[wc];
                t_o[i] = b[nw];
                t_f[i] = b[3 * nw];
                t_n[i] = b[5 * nw];
            }
            // (the pins: an empty statement the compiler must hand the loaded
            // registers to, so every load above is issued before the first
            // value is used. Without them the loads may sink to their uses
            // behind the seed test and run as one dependent round per word.)
#pragma unroll
            for (int i = 0; i < kPer; i++) {
                asm volatile("" : "+v"(t_o[i]), "+v"(t_f[i]), "+v"(t_n[i]), "+v"(r_w[i]));
                r_o[i] = (r_o[i] & ~r_w[i]) | (t_o[i] & r_w[i]);
                r_f[i] = (r_f[i] & ~r_w[i]) | (t_f[i] & r_w[i]);
                r_n[i] = (r_n[i] & ~r_w[i]) | (t_n[i] & r_w[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < kPer; i++) asm volatile("" : "+v"(r_o[i]), "+v"(r_f[i]), "+v"(r_n[i]));
        asm volatile("" : "+v"(r_seed));
    }
    ChainSeed in;
    in.status = kSeedOk;
    in.placed = 0;
    in.cur = wrap_pos(A.offset0, n ? n : 1u);
    in.pos_used = 0;
    if (phase) {
        if (args_ok) {
            in.status = (uint32_t)__shfl((int)r_seed, 0);
            in.placed = (uint32_t)__shfl((int)r_seed, 1);
            in.cur = (uint32_t)__shfl((int)r_seed, 2);
            in.pos_used = (uint32_t)__shfl((int)r_seed, 3);
        } else {
            in = Wd.seed[phase - 1];
        }
    }
    if (in.status != kSeedOk || in.placed >= A.count) {
        if (first) Wd.seed[phase] = in;
        return;
    }
    const uint32_t cur = in.cur;
    bool ok = args_ok && cur < n;
    uint32_t tot_o = 0, ns = 0, c_opt = 0, c_fil = 0, tot_f = 0;
    if (ok) {
        uint32_t any_n = 0;
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            const uint32_t w = lane + (uint32_t)i * kWideBlock;
            if (w < nw) {
                s_opt[w] = r_o[i];
                s_fil[w] = r_f[i];
                s_won[w] = r_w[i];
                any_n |= r_n[i];
            }
        }
        __syncthreads();
        // exclusive word prefixes (absolute positions), the totals at [nw]
        const uint32_t per = (nw + kWideBlock - 1) / kWideBlock;
        const uint32_t w0 = min(lane * per, nw), w1 = min(w0 + per, nw);
        uint32_t so = 0, sf = 0;
        for (uint32_t w = w0; w < w1; w++) {
            so += (uint32_t)__popc(s_opt[w]);
            sf += (uint32_t)__popc(s_fil[w]);
        }
        uint32_t io = so, iff = sf;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t xo = (uint32_t)__shfl_up((int)io, off), xf = (uint32_t)__shfl_up((int)iff, off);
            if ((int)lane >= off) { io += xo; iff += xf; }
        }
        uint32_t eo = io - so, ef = iff - sf;
        for (uint32_t w = w0; w < w1; w++) {
            p_opt[w] = eo;
            p_fil[w] = ef;
            eo += (uint32_t)__popc(s_opt[w]);
            ef += (uint32_t)__popc(s_fil[w]);
        }
        if (lane == kWideBlock - 1) {
            p_opt[nw] = io;
            p_fil[nw] = iff;
        }
        __syncthreads();
        tot_o = p_opt[nw];
        tot_f = p_fil[nw];
        ns = min(A.count - in.placed, tot_o / L);
        // non-positive options (the Selects set them aside), or no whole Select
        // in the window (k_chain's Retry / Stall / Exhausted modes): k_chain's
        if (__ballot(any_n != 0u) != 0ull || ns == 0) ok = false;
    }
    if (!ok) {
        if (first) {
            in.status = kSeedDeclined;
            Wd.seed[phase] = in;
            Wd.stats[1] += 1ull;
        }
        return;
    }
    c_opt = wide_prefix(p_opt, s_opt, nw, cur);
    c_fil = wide_prefix(p_fil, s_fil, nw, cur);
    // filtered positions among the relative positions [0, x), x in [0, n]
    auto fil_before = [&](uint32_t x) {
        const uint32_t a = cur + x;
        if (a <= n) return wide_prefix(p_fil, s_fil, nw, a) - c_fil;
        return tot_f - c_fil + wide_prefix(p_fil, s_fil, nw, a - n);
    };
    auto rel_of = [&](uint32_t p) { return p >= cur ? p - cur : p + n - cur; };
    // the visit position (absolute) of the option of relative rank k < tot_o
    auto opt_at = [&](uint32_t k, uint32_t* w, uint32_t* rest) {
        uint32_t r = c_opt + k;
        if (r >= tot_o) r -= tot_o;
        return r < tot_o && wide_select(p_opt, s_opt, nw, r, w, rest);
    };
    for (uint32_t s = blockIdx.x * kWideBlock + lane; s < ns; s += gridDim.x * kWideBlock) {
        // the Select's options s L .. s L + L - 1: their values, rows and (on a
        // phase 0 winner's position) writeback slots in one round of loads, so
        // the winner's row does not cost a round trip of its own
        uint32_t w = 0, word = 0;
        bool good = opt_at(s * L, &w, &word);
        uint32_t pos[kMaxChainLimit], prow[kMaxChainLimit], pslot[kMaxChainLimit];
        double val[kMaxChainLimit];
#pragma unroll
        for (uint32_t k = 0; k < kMaxChainLimit; k++) {
            pos[k] = 0;
            prow[k] = 0;
            pslot[k] = ~0u;
            val[k] = 0.0;
            if (k >= L || !good) continue;
            for (uint32_t hop = 0; word == 0u && hop <= nw; hop++) {   // the next word that holds an option
                w = w + 1u < nw ? w + 1u : 0u;
                word = s_opt[w];
            }
            if (word == 0u) { good = false; continue; }
            const uint32_t bit = (uint32_t)__ffs((int)word) - 1u;
            word &= word - 1u;
            const uint32_t p = w * 32u + bit;
            if (p >= n) { good = false; continue; }
            const bool had = (s_won[w] >> bit) & 1u;
            pos[k] = p;
            val[k] = (had ? A.base1 : A.base)[p];
            prow[k] = A.perms[p];
            if (had) pslot[k] = Wd.slot[p];
        }
        // the previous Select's stop (its last option), for the span's start
        uint32_t start = 0;
        if (s && good) {
            uint32_t pw = 0, prest = 0;
            good = opt_at(s * L - 1u, &pw, &prest);
            if (good) start = rel_of(pw * 32u + (uint32_t)__ffs((int)prest) - 1u) + 1u;
        }
        const uint32_t it = in.placed + s;
        if (!good || it >= A.count) {
            wide_fail(Wd);
            continue;
        }
        // first strict maximum in visit order (chain_walk's rule without set-aside options)
        double best = val[0];
        uint32_t bp = pos[0], stop = pos[0], row = prow[0], sl = pslot[0];
#pragma unroll
        for (uint32_t k = 1; k < kMaxChainLimit; k++) {
            if (k >= L) continue;
            stop = pos[k];
            if (val[k] > best) { best = val[k]; bp = pos[k]; row = prow[k]; sl = pslot[k]; }
        }
        const uint32_t stop_rel = rel_of(stop);
        const uint32_t consumed = stop_rel + 1u - start;
        const uint32_t nf = fil_before(stop_rel + 1u) - fil_before(start);
        if (stop_rel >= n || stop_rel < start || consumed < L + nf) {
            wide_fail(Wd);
            continue;
        }
        const uint32_t dk = (s_won[bp >> 5] >> (bp & 31u)) & 1u;
        if (dk && sl >= A.count) {   // the slot phase 0 stored for this position
            wide_fail(Wd);
            continue;
        }
        ChainEmit& m = A.emit[it];
        m.row = (int32_t)row;
        m.dk = dk;
        m.consumed = consumed;
        m.filtered = nf;
        m.exhausted = consumed - L - nf;
        m.new_offset = wrap_pos(cur + stop_rel + 1u, n);
        m.pos = bp;
        m.score = best;
        // the writeback's entry: one per row
        if (dk) {
            A.emit_ov[sl] = make_uint2(row, 2u);
            A.emit_ov[it] = make_uint2(row, 0u);
        } else {
            A.emit_ov[it] = make_uint2(row, 1u);
            if (phase == 0) Wd.slot[bp] = it;
        }
        atomicOr(&Wd.won[phase * nw + (bp >> 5)], 1u << (bp & 31u));
    }
    if (first) {
        uint32_t w = 0, rest = 0;
        if (!opt_at(ns * L - 1u, &w, &rest)) {
            wide_fail(Wd);
            in.status = kSeedDeclined;
            Wd.seed[phase] = in;
            return;
        }
        const uint32_t used = rel_of(w * 32u + (uint32_t)__ffs((int)rest) - 1u) + 1u;
        in.placed += ns;
        in.cur = wrap_pos(cur + used, n);
        in.pos_used += used;
        Wd.seed[phase] = in;
        Wd.stats[0] += 1ull;
    }
}

// ---- both wide phases in one launch, options compacted by rank -------------------
//
// k_phases is k_phase(0) and k_phase(1) in one workgroup: phase 1 follows phase
// 0 behind the workgroup's own barrier, so there is one dispatch, one prologue
// per phase and no launch-to-launch state but the last seed. Instead of a rank
// select per Select (a binary search over the word prefixes and a walk over set
// bits), one pass over the visit positions writes the inverse map once: an
// option's absolute rank is prefix[word] + popc(bits below), its rank relative
// to the cursor k = rank - c_opt (wrapped by the options' total), and the
// option of relative rank k belongs to Select k / L. So position and value (a
// coalesced load of base / base1) go to LDS entry k, and Select s reads the L
// consecutive entries [s L, (s + 1) L). Everything stored (ChainEmit, emit_ov,
// slot, seed, stats, err) is what the k_phase pair stores, except `won`, which
// only phase 1 reads and which therefore stays in LDS.
// LDS: the static words below plus pe_chain_one_lds_bytes() of entries; a
// launch that needs more than a workgroup may hold keeps the k_phase pair.
constexpr int kOneBlock = 1024;
static_assert(kWideMaxWords <= (uint32_t)kOneBlock, "k_phases: one bitmap word per lane");
static_assert(kChainMaxN <= (1u << 16), "k_phases: positions in 16 bits, word prefixes of two bitmaps in one word");

// compact entries of a launch: one per option the two phases can return
__host__ __device__ inline uint32_t one_entries(uint32_t n_visit, uint32_t count, uint32_t limit) {
    const unsigned long long cl = (unsigned long long)count * limit;
    return cl < n_visit ? (uint32_t)cl : n_visit;
}
// the values (8 B each), then the positions (2 B each)
__host__ __device__ inline size_t one_lds_bytes(uint32_t entries) {
    return (size_t)entries * sizeof(double) + (((size_t)entries * sizeof(uint16_t) + 15u) & ~(size_t)15u);
}

__global__ void __launch_bounds__(kOneBlock) k_phases(BatchArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char one_smem[];
    __shared__ uint32_t s_opt[kWideMaxWords], s_fil[kWideMaxWords], s_won[kWideMaxWords];
    __shared__ uint32_t s_pre[kWideMaxWords + 1];   // exclusive word prefixes: options | filtered << 16
    __shared__ uint32_t s_wave[kOneBlock / 64], s_neg;
    const ChainWide& Wd = A.wide;
    const uint32_t tid = threadIdx.x, n = A.n_visit, L = A.limit, nw = Wd.words;
    const bool args_ok = n != 0 && nw == (n + 31u) / 32u && nw <= kWideMaxWords && L != 0 && L <= kMaxChainLimit;
    const uint32_t cap = one_entries(n, A.count, L);
    double* e_val = reinterpret_cast<double*>(one_smem);
    uint16_t* e_pos = reinterpret_cast<uint16_t*>(e_val + cap);
    // one round of loads: the lane's word of all six bitmaps, for both phases
    uint32_t t_o[2] = {0u, 0u}, t_f[2] = {0u, 0u}, t_n[2] = {0u, 0u};
    if (args_ok && tid < nw) {
        const uint32_t* b = Wd.bits + tid;
#pragma unroll
        for (uint32_t t = 0; t < 2; t++) {
            t_o[t] = b[t * nw];
            t_f[t] = b[(2 + t) * nw];
            t_n[t] = b[(4 + t) * nw];
        }
    }
    if (tid < kWideMaxWords) s_won[tid] = 0u;
    ChainSeed in;
    in.status = kSeedOk;
    in.placed = 0;
    in.cur = wrap_pos(A.offset0, n ? n : 1u);
    in.pos_used = 0;
    const uint32_t phases = Wd.phases < 2u ? Wd.phases : 2u;   // a row holds at most one placement per phase
    // (every test that leaves or declines a phase is uniform over the workgroup)
    for (uint32_t phase = 0; phase < phases; phase++) {
        if (in.status != kSeedOk || in.placed >= A.count) {
            if (tid == 0) Wd.seed[phase] = in;
            continue;
        }
        const uint32_t cur = in.cur;
        bool ok = args_ok && cur < n;
        uint32_t tot_o = 0, tot_f = 0, ns = 0;
        if (ok) {
            if (tid == 0) s_neg = 0u;
            __syncthreads();   // phase 0's winners are in s_won; its readers of the entries are done
            // the phase's bitmaps: table 1 where the row won in phase 0
            uint32_t o = 0, f = 0, neg = 0;
            if (tid < nw) {
                const uint32_t w = phase ? s_won[tid] : 0u;
                o = (t_o[0] & ~w) | (t_o[1] & w);
                f = (t_f[0] & ~w) | (t_f[1] & w);
                neg = (t_n[0] & ~w) | (t_n[1] & w);
                if (tid == nw - 1u && (n & 31u) && ((o | f) >> (n & 31u))) {   // bits past the list's end
                    wide_fail(Wd);
                    o &= (1u << (n & 31u)) - 1u;
                    f &= (1u << (n & 31u)) - 1u;
                }
                s_opt[tid] = o;
                s_fil[tid] = f;
                if (neg) atomicOr(&s_neg, 1u);
            }
            // word prefixes of both bitmaps: a scan per wave, then the waves' totals
            const uint32_t pk = (uint32_t)__popc(o) | ((uint32_t)__popc(f) << 16);
            uint32_t inc = pk;
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t x = (uint32_t)__shfl_up((int)inc, off);
                if ((int)(tid & 63u) >= off) inc += x;
            }
            if ((tid & 63u) == 63u) s_wave[tid >> 6] = inc;
            __syncthreads();
            uint32_t before = 0;
            for (uint32_t v = 0; v < (tid >> 6); v++) before += s_wave[v];
            if (tid < nw) s_pre[tid] = before + inc - pk;
            if (tid == nw - 1u) s_pre[nw] = before + inc;
            __syncthreads();
            tot_o = s_pre[nw] & 0xFFFFu;
            tot_f = s_pre[nw] >> 16;
            ns = min(A.count - in.placed, tot_o / L);
            // non-positive options (the Selects set them aside), or no whole Select
            // in the window (k_chain's Retry / Stall / Exhausted modes): k_chain's
            if (s_neg != 0u || ns == 0) ok = false;
        }
        if (!ok) {
            if (tid == 0) {
                in.status = kSeedDeclined;
                Wd.seed[phase] = in;
                Wd.stats[1] += 1ull;
            }
            in.status = kSeedDeclined;
            continue;
        }
        // set bits at absolute positions [0, p), p in [0, n]: options | filtered << 16
        auto prefix = [&](uint32_t p) {
            const uint32_t w = p >> 5;
            if (w >= nw) return s_pre[nw];
            const uint32_t below = (1u << (p & 31u)) - 1u;
            return s_pre[w] + ((uint32_t)__popc(s_opt[w] & below) | ((uint32_t)__popc(s_fil[w] & below) << 16));
        };
        const uint32_t c_pk = prefix(cur), c_opt = c_pk & 0xFFFFu, c_fil = c_pk >> 16;
        // filtered positions among the relative positions [0, x), x in [0, n]
        auto fil_before = [&](uint32_t x) {
            const uint32_t a = cur + x;
            if (a <= n) return (prefix(a) >> 16) - c_fil;
            return tot_f - c_fil + (prefix(a - n) >> 16);
        };
        auto rel_of = [&](uint32_t p) { return p >= cur ? p - cur : p + n - cur; };
        // ns <= count - placed and ns L <= tot_o <= n: the entries fit (guarded all the same)
        uint32_t need = ns * L;
        if (need > cap) {
            if (tid == 0) wide_fail(Wd);
            need = cap;
            ns = need / L;
        }
        // compaction: every option of relative rank below ns L into its entry
#pragma unroll 4
        for (uint32_t p = tid; p < n; p += kOneBlock) {
            const uint32_t w = p >> 5, bit = p & 31u, word = s_opt[w];
            if (!((word >> bit) & 1u)) continue;
            const uint32_t r = (s_pre[w] & 0xFFFFu) + (uint32_t)__popc(word & ((1u << bit) - 1u));
            const uint32_t k = r >= c_opt ? r - c_opt : r + tot_o - c_opt;
            if (k >= need) continue;
            const bool had = phase && ((s_won[w] >> bit) & 1u);
            e_val[k] = (had ? A.base1 : A.base)[p];
            e_pos[k] = (uint16_t)p;
        }
        __syncthreads();
        for (uint32_t s = tid; s < ns; s += kOneBlock) {
            // first strict maximum in visit order (chain_walk's rule without set-aside options)
            const uint32_t e0 = s * L;
            double best = e_val[e0];
            uint32_t bk = 0;
            for (uint32_t k = 1; k < L; k++) {
                const double v = e_val[e0 + k];
                if (v > best) { best = v; bk = k; }
            }
            const uint32_t bp = e_pos[e0 + bk], stop = e_pos[e0 + L - 1u];
            // the previous Select's stop (its last option), for the span's start
            const uint32_t start = s ? rel_of(e_pos[e0 - 1u]) + 1u : 0u;
            const uint32_t it = in.placed + s;
            if (bp >= n || stop >= n || it >= A.count) {
                wide_fail(Wd);
                continue;
            }
            const uint32_t stop_rel = rel_of(stop);
            const uint32_t consumed = stop_rel + 1u - start;
            const uint32_t nf = fil_before(stop_rel + 1u) - fil_before(start);
            if (stop_rel >= n || stop_rel < start || consumed < L + nf) {
                wide_fail(Wd);
                continue;
            }
            // the winner's row and (on a phase 0 winner) its writeback slot, one round of loads
            const uint32_t dk = phase ? (s_won[bp >> 5] >> (bp & 31u)) & 1u : 0u;
            const uint32_t row = A.perms[bp];
            const uint32_t sl = dk ? Wd.slot[bp] : ~0u;   // stored in phase 0, before the workgroup's barrier
            if (dk && sl >= A.count) {
                wide_fail(Wd);
                continue;
            }
            ChainEmit& m = A.emit[it];
            m.row = (int32_t)row;
            m.dk = dk;
            m.consumed = consumed;
            m.filtered = nf;
            m.exhausted = consumed - L - nf;
            m.new_offset = wrap_pos(cur + stop_rel + 1u, n);
            m.pos = bp;
            m.score = best;
            // the writeback's entry: one per row
            if (dk) {
                A.emit_ov[sl] = make_uint2(row, 2u);
                A.emit_ov[it] = make_uint2(row, 0u);
            } else {
                A.emit_ov[it] = make_uint2(row, 1u);
                if (phase == 0) {
                    Wd.slot[bp] = it;
                    atomicOr(&s_won[bp >> 5], 1u << (bp & 31u));
                }
            }
        }
        // the seed after the phase, in every lane (phase 1 starts from it)
        const uint32_t last = e_pos[ns * L - 1u];
        if (last >= n) {
            if (tid == 0) {
                wide_fail(Wd);
                in.status = kSeedDeclined;
                Wd.seed[phase] = in;
            }
            in.status = kSeedDeclined;
            continue;
        }
        const uint32_t used = rel_of(last) + 1u;
        in.placed += ns;
        in.cur = wrap_pos(cur + used, n);
        in.pos_used += used;
        if (tid == 0) {
            Wd.seed[phase] = in;
            Wd.stats[0] += 1ull;
        }
    }
}

// The placed count of a 256-lane workgroup, one atomic per workgroup into one
// of kPlacedSlots counters (the host sums them): same-address atomics from
// every wave serialise at one L2 channel (32k of them at 6.4M rows cost more
// than the evaluation).
__device__ __forceinline__ void add_placed(uint32_t local, uint32_t* slots) {
    __shared__ uint32_t red[4];
    for (int off = 32; off > 0; off >>= 1) local += __shfl_xor(local, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t x = red[0] + red[1] + red[2] + red[3];
        if (x) atomicAdd(&slots[blockIdx.x % kPlacedSlots], x);
    }
}

// SystemStack: every list entry is an independent single-node Select.
__global__ void __launch_bounds__(256) k_system(SystemArgs A) {
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t local = 0;
    Overlay none;
    none.keys = nullptr;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < A.n_list; i += stride) {
        const uint32_t row = A.list[i];
        NodeEval ev;
        eval_node<false>(A.soa, A.tg, A.tg.class_ok, A.ask, none, nullptr, A.log10, nullptr, row, &ev);
        if (ev.status == kOption) {
            A.out_score[i] = ev.score;
            A.out_status[i] = 0;
            local++;
            if (!A.commit) continue;
            // Plan.AppendAlloc: rows are unique in the list, so no races
            NodeRec& r = A.soa.rec[row];
            r.used_cpu += ask_cpu(A.soa, A.ask, row);
            core_take(A.soa, A.ask, row, 1);
            r.used_mem += A.ask.mem;
            r.used_disk += A.ask.disk;
            r.used_mbits += A.ask.commit_mbits;
            r.used_dyn += A.ask.commit_dyn;
            A.soa.coll_job[row] += 1;
            A.tg.coll_tg[row] += 1;
            if (A.ask.n_dev > 0) A.tg.dev_free[row] = dev_after(A.ask, A.tg.dev_cls[r.cls], A.tg.dev_free[row], 1);
        } else {
            A.out_score[i] = __builtin_nan("");
            A.out_status[i] = (uint8_t)ev.status;
        }
    }
    if (A.placed) add_placed(local, A.placed);
}

// k_system in row order, phase one: every row of the list evaluated (and
// committed) with coalesced accesses; the outcome lands in res[row].
__device__ __forceinline__ uint64_t sys_box(int status, double score) {
    if (status == kOption) return (uint64_t)__double_as_longlong(score);
    return 0x7FF8000000000000ull | (uint64_t)status;   // a quiet NaN carrying the outcome
}

__global__ void __launch_bounds__(256) k_system_rows(SystemArgs A) {
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t local = 0;
    Overlay none;
    none.keys = nullptr;
    for (uint32_t row = blockIdx.x * blockDim.x + threadIdx.x; row < A.n_rows; row += stride) {
        if (A.rank_of[row] == 0xFFFFFFFFu) continue;
        NodeEval ev;
        eval_node<false>(A.soa, A.tg, A.tg.class_ok, A.ask, none, nullptr, A.log10, nullptr, row, &ev);
        A.res[row] = sys_box(ev.status, ev.score);
        if (ev.status != kOption) continue;
        local++;
        if (!A.commit) continue;
        NodeRec& r = A.soa.rec[row];
        r.used_cpu += ask_cpu(A.soa, A.ask, row);
        core_take(A.soa, A.ask, row, 1);
        r.used_mem += A.ask.mem;
        r.used_disk += A.ask.disk;
        r.used_mbits += A.ask.commit_mbits;
        r.used_dyn += A.ask.commit_dyn;
        A.soa.coll_job[row] += 1;
        A.tg.coll_tg[row] += 1;
        if (A.ask.n_dev > 0) A.tg.dev_free[row] = dev_after(A.ask, A.tg.dev_cls[r.cls], A.tg.dev_free[row], 1);
    }
    if (A.placed) add_placed(local, A.placed);
}

// Phase two of the row-order pass: the outcomes back in list order. Reads the
// list coalesced and res[list[pos]] (8 B per row, L2 / MALL resident), writes
// FinalScore and the outcome coalesced; random 8-byte stores into the outputs
// would cost a 64-byte line write each.
__global__ void __launch_bounds__(256) k_system_gather(const uint32_t* list, uint32_t n_list, const uint64_t* res,
                                                      double* out_score, uint8_t* out_status) {
    const uint32_t pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= n_list) return;
    const uint64_t v = res[list[pos]];
    const bool boxed = (v & 0xFFFFFFFFFFFFFFF0ull) == 0x7FF8000000000000ull;
    out_score[pos] = boxed ? __builtin_nan("") : __longlong_as_double((long long)v);
    out_status[pos] = boxed ? (uint8_t)(v & 15u) : (uint8_t)kOption;
}

// rank_of[row] = position of row in the list (rows absent: PE_NONE, set by the caller's memset)
__global__ void __launch_bounds__(256) k_rank_of(const uint32_t* list, uint32_t n_list, uint32_t* rank_of) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_list) rank_of[list[i]] = i;
}

// Outcome census of one Select pass over the visit list on the HBM state
// (no overlay): counts[0] options, [1] filtered, [2] exhausted. With no option
// the Select is nil after pulling every node, which the count loop's
// preemption retry uses instead of a windowed scan of the whole list.
// kParts: also the score parts of each option (k_ploop's plain winner records).
template <bool kParts>
__global__ void __launch_bounds__(256) k_census(BatchArgs A, uint32_t* counts, uint8_t* status, double* score,
                                                double* parts, uint8_t* nparts) {
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t c[3] = {0, 0, 0};
    Overlay none;
    none.keys = nullptr;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < A.n_visit; j += stride) {
        NodeEval ev;
        eval_node<kParts>(A.soa, A.tg, A.tg.class_ok, A.ask, none, A.penalty_bits, A.log10, nullptr, A.perms[j], &ev);
        c[ev.status]++;
        if (status) {   // per-position outcomes for a parallel Select (k_evict_resolve)
            status[j] = (uint8_t)ev.status;
            score[j] = ev.status == kOption ? ev.score : 0.0;
        }
        if (kParts && ev.status == kOption) {
            nparts[j] = (uint8_t)ev.nscores;
            for (int k = 0; k < PE_MAX_SCORES; k++) parts[(size_t)j * PE_MAX_SCORES + k] = ev.parts[k];
        }
    }
    // one atomic per workgroup and counter (not per wave): fewer same-address
    // atomics queueing at one L2 channel
    __shared__ uint32_t red[3][4];
    for (int k = 0; k < 3; k++) {
        uint32_t x = c[k];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = x;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint32_t x = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        if (x) atomicAdd(&counts[threadIdx.x], x);
    }
}

// Host-driven Plan.AppendAlloc on the HBM SoA (pe_commit). `offers`: the
// device offers of the Select that chose the node (one byte per request), or
// ~0u to assign them on the current state.
template <bool kCores = true>
__device__ __forceinline__ void commit_row(const NodeSoA& s, const TgTables& t, const Ask& a, uint32_t row,
                                           uint32_t offers) {
    // Every load before the first store: the counters share types with the
    // record's fields, so a load placed after a store is issued only once the
    // store's own load has returned, one HBM round trip per field.
    NodeRec& r = s.rec[row];
    const int64_t cpu = r.used_cpu, mem = r.used_mem, disk = r.used_disk;
    const int32_t mbits = r.used_mbits, dyn = r.used_dyn;
    const uint32_t c = r.cls, cj = s.coll_job[row], ct = t.coll_tg[row];
    const uint32_t fr0 = a.n_dev > 0 ? t.dev_free[row] : 0u;
    const int64_t ac = kCores ? ask_cpu(s, a, row) : a.cpu;
    uint32_t fr = fr0;
    if (a.n_dev > 0) {
        if (offers == 0xFFFFFFFFu) {
            fr = dev_after(a, t.dev_cls[c], fr0, 1);
        } else {
            for (int q = 0; q < kMaxDevReq && q < a.n_dev; q++) {
                const uint32_t g = (offers >> (8 * q)) & 255u, f = (fr >> (8 * g)) & 255u;
                const uint32_t cnt = (uint32_t)a.dev_cnt[q];
                fr -= (cnt < f ? cnt : f) << (8 * g);
            }
        }
    }
    r.used_cpu = cpu + ac;
    r.used_mem = mem + a.mem;
    r.used_disk = disk + a.disk;
    r.used_mbits = mbits + a.commit_mbits;
    r.used_dyn = dyn + a.commit_dyn;
    s.coll_job[row] = cj + 1u;
    t.coll_tg[row] = ct + 1u;
    if (a.n_dev > 0) t.dev_free[row] = fr;
    if (kCores) core_take(s, a, row, 1);
    for (int p = 0; p < t.n_psets; p++) {
        const uint32_t v = pset_value(t, p, row, c);
        if (v != kMissing) t.pset_counts[p][v] += 1;
    }
}

__global__ void k_commit(NodeSoA s, TgTables t, Ask a, uint32_t row, uint32_t offers) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    commit_row(s, t, a, row, offers);
}

// Plan.AppendAlloc of distinct rows chosen on the host (SystemScheduler
// placements resolved against distinct_property counts): commit_row per
// thread, the shared property-set counts by atomics.
__global__ void __launch_bounds__(256) k_commit_rows(NodeSoA s, TgTables t, Ask a, const uint32_t* rows, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = rows[i];
    NodeRec& r = s.rec[row];
    r.used_cpu += ask_cpu(s, a, row);
    core_take(s, a, row, 1);
    r.used_mem += a.mem;
    r.used_disk += a.disk;
    r.used_mbits += a.commit_mbits;
    r.used_dyn += a.commit_dyn;
    s.coll_job[row] += 1;
    t.coll_tg[row] += 1;
    if (a.n_dev > 0) t.dev_free[row] = dev_after(a, t.dev_cls[r.cls], t.dev_free[row], 1);
    for (int p = 0; p < t.n_psets; p++) {
        const uint32_t v = pset_value(t, p, row, r.cls);
        if (v != kMissing) atomicAdd(&t.pset_counts[p][v], 1u);
    }
}

// Replay (sign +1) of a speculative loop's confirmed placements after a
// rollback to its checkpoint, or removal (sign -1) of its unconfirmed ones
// (pe_commit / pe_select, engine.cpp): one thread per placement, every update
// an integer atomic add, so repeated rows sum exactly as the sequential
// commit_row calls would. Each offer was assigned on the state that already
// held every earlier placement, so no free count underflows and the packed u8
// subtractions never borrow. Removal is only used without device asks.
__global__ void __launch_bounds__(256) k_apply_commits(NodeSoA s, TgTables t, Ask a, const uint32_t* rows,
                                                      const uint32_t* offers, uint32_t n, int sign) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = rows[i];
    NodeRec& r = s.rec[row];
    const unsigned long long s64 = (unsigned long long)(long long)sign;
    const unsigned int s32 = (unsigned int)sign;
    atomicAdd(reinterpret_cast<unsigned long long*>(&r.used_cpu), (unsigned long long)a.cpu * s64);
    atomicAdd(reinterpret_cast<unsigned long long*>(&r.used_mem), (unsigned long long)a.mem * s64);
    atomicAdd(reinterpret_cast<unsigned long long*>(&r.used_disk), (unsigned long long)a.disk * s64);
    atomicAdd(reinterpret_cast<unsigned int*>(&r.used_mbits), (unsigned int)a.commit_mbits * s32);
    atomicAdd(reinterpret_cast<unsigned int*>(&r.used_dyn), (unsigned int)a.commit_dyn * s32);
    atomicAdd(&s.coll_job[row], s32);
    atomicAdd(&t.coll_tg[row], s32);
    const uint32_t c = r.cls;
    if (a.n_dev > 0 && sign > 0) {
        const uint32_t o = offers[i];
        uint32_t sub = 0;
        for (int q = 0; q < kMaxDevReq && q < a.n_dev; q++) sub += (uint32_t)a.dev_cnt[q] << (8 * ((o >> (8 * q)) & 255u));
        atomicSub(&t.dev_free[row], sub);
    }
    for (int p = 0; p < t.n_psets; p++) {
        const uint32_t v = pset_value(t, p, row, c);
        if (v != kMissing) atomicAdd(&t.pset_counts[p][v], s32);
    }
}

// One pass of the scoring sweep over rows [row_begin, row_end), one tile of
// BLOCK rows per workgroup iteration (grid-stride), 64 rows per wave. Every
// lane streams its row (64-byte record, collision count, verdict, visit rank),
// runs the feasibility half and resolves the score-table lookups of an option.
// Options go to a wave-private LDS ring (kQueue entries); whenever it holds 64
// the wave runs the fp64 scoring half (two software Pow) on a full wave, so
// the scoring is dense and no workgroup barrier sits in the loop. Per-lane
// SweepRec records, reduced per workgroup at the end. Rows outside the visit
// list are dropped.
//
// AUX: the node's verdict, affinity index and spread values come folded in one
// u32 per node (k_fold_aux) and resolve against LDS copies of the affinity
// values and the spread boosts, so an option costs no dependent table load.
template <int BLOCK, bool AUX>
__device__ __forceinline__ void sweep_block(const SweepArgs& A) {
    constexpr int W = BLOCK / 64;
    constexpr uint32_t kQueue = 128;
    __shared__ SweepRec red[W];
    __shared__ ScoreIn q[W][kQueue];
    __shared__ uint32_t q_rank[W][kQueue];
    __shared__ double aff_lds[AUX ? kAuxValues : 1];
    __shared__ double sp_lds[AUX ? kAuxPsets : 1][AUX ? kAuxValues : 1];
    SweepRec r;
    rec_init(r);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (AUX) {
        for (int i = tid; i < kAuxValues; i += BLOCK) aff_lds[i] = A.aff_vals[i];
        for (int p = 0; p < A.tg.n_psets; p++)
            for (int i = tid; i < kAuxValues; i += BLOCK)
                sp_lds[p][i] = i < A.tg.pset_nvals[p] ? A.spread_tab[A.tg.pset_tab_off[p] + i] : 0.0;
        __syncthreads();
    }
    const uint32_t n = A.n_visit;
    const uint32_t stride = gridDim.x * BLOCK;
    ScoreIn* wq = q[wid];
    uint32_t* wr = q_rank[wid];
    uint32_t head = 0, qn = 0;   // wave-uniform ring state
    auto score_from = [&](uint32_t at) {
        const uint32_t i = (at + (uint32_t)lane) & (kQueue - 1);
        NodeEval ev;
        score_option<false>(A.ask, A.log10, wq[i], &ev);
        rec_add(r, wr[i], ev.score);
    };
    NodeIn nx;
    uint32_t npos = kEmpty, naux = 0;
    auto fetch = [&](uint32_t t) {
        const uint32_t row = t + (uint32_t)tid;
        npos = kEmpty;
        if (row < A.row_end && row >= t) {
            npos = A.rank_of[row];
            if (AUX) {
                nx.r = A.soa.rec[row];
                nx.coll_tg = A.tg.coll_tg[row];
                nx.dev_free = A.tg.dev_free ? A.tg.dev_free[row] : 0u;
                naux = A.node_aux[row];
                nx.feas = naux >> 31;
            } else {
                load_node(A.soa, A.tg, row, nx);
            }
        }
    };
    for (uint32_t tile = A.row_begin + blockIdx.x * BLOCK; tile < A.row_end; tile += stride) {
        fetch(tile);
        const NodeIn in = nx;
        const uint32_t pos = npos, aux = naux;
        const uint32_t row = tile + (uint32_t)tid;
        bool opt = false;
        uint32_t rank = 0;
        ScoreIn si;
        if (pos != kEmpty) {
            const int st = status_loaded(A.soa, A.tg, A.tg.class_ok, A.ask, 0u, row, in, &si);
            if (st == kFiltered) r.filtered++;
            else if (st == kExhausted) r.exhausted++;
            else {
                opt = true;
                rank = pos >= A.offset ? pos - A.offset : pos + n - A.offset;
                if (AUX) {
                    si.penalty = A.penalty_bits ? (A.penalty_bits[row >> 5] >> (row & 31)) & 1u : 0u;
                    si.aff = aff_lds[aux & 255u];
                    double total = 0.0;
                    for (int p = 0; p < A.tg.n_psets; p++) {
                        const uint32_t v = (aux >> (8 + 8 * p)) & 255u;
                        total += (v == kAuxMissing) ? -1.0 : sp_lds[p][v];
                    }
                    si.spread = total;
                } else {
                    lookup_scores(A.tg, A.penalty_bits, A.spread_tab, row, in.r.cls, &si);
                }
            }
        }
        const uint64_t m = __ballot(opt);
        if (opt) {
            const uint32_t i = (head + qn + lanes_below(m, lane)) & (kQueue - 1);
            wq[i] = si;
            wr[i] = rank;
        }
        qn += (uint32_t)__popcll(m);
        if (qn >= 64) {   // LDS ops of one wave complete in order: the ring is visible
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            score_from(head);
            head = (head + 64) & (kQueue - 1);
            qn -= 64;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if ((uint32_t)lane < qn) score_from(head);
    rec_block_reduce<BLOCK>(r, red);
    if (threadIdx.x == 0) A.recs[blockIdx.x] = r;
}

template <int BLOCK, bool AUX>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(AUX ? 4 : 5))) k_sweep(SweepArgs A) {
    sweep_block<BLOCK, AUX>(A);
}

// Merge the per-workgroup records (one 512-thread workgroup: a few records per
// thread, so the dependent load chain stays short).
__global__ void __launch_bounds__(512) k_sweep_merge(const SweepRec* recs, uint32_t count, SweepRec* out) {
    __shared__ SweepRec red[8];
    SweepRec r;
    rec_init(r);
    for (uint32_t i = threadIdx.x; i < count; i += 512) rec_merge(r, recs[i]);
    rec_block_reduce<512>(r, red);
    if (threadIdx.x == 0) *out = r;
}

// Spread contribution table in HBM for the sweep path (same code as the
// persistent loop's LDS table, so both paths are bit-identical).
// The spread boost tables of every record of a speculative run (spec_metrics):
// record k's use counts are the run's starting counts (t.pset_counts, the
// checkpoint) plus the earlier records' placements (`delta`: n_rec x
// pset_cnt_total, host-built, completed here in place); one block per record,
// its table at tab + k * pset_tab_total. Spread sets only.
// kAbsolute (pe_place_destructive_full_metrics): `delta` holds record k's use
// counts themselves (k_destructive_full<*, true>'s cnt_log), and t.pset_counts
// is not read.
template <bool kAbsolute>
__global__ void __launch_bounds__(256) k_spread_tables(TgTables t, uint32_t* delta, double* tab) {
    __shared__ uint32_t scratch[4];
    const uint32_t k = blockIdx.x;
    uint32_t* cnt = delta + (size_t)k * t.pset_cnt_total;
    if constexpr (!kAbsolute) {
        for (int p = 0; p < t.n_psets; p++)
            for (int v = threadIdx.x; v < t.pset_nvals[p]; v += 256) cnt[t.pset_cnt_off[p] + v] += t.pset_counts[p][v];
        __syncthreads();
    }
    build_spread_table<256>(t, cnt, tab + (size_t)k * t.pset_tab_total, scratch);
}
template __global__ void k_spread_tables<false>(TgTables, uint32_t*, double*);   // the existing form first

__global__ void __launch_bounds__(256) k_spread_table(TgTables t, double* tab) {
    __shared__ uint32_t counts[kLdsPsetValues];
    __shared__ uint32_t scratch[4];
    const bool lds = t.pset_cnt_total <= (uint32_t)kLdsPsetValues;   // else the HBM counts
    if (lds)
        for (int p = 0; p < t.n_psets; p++)
            for (int v = threadIdx.x; v < t.pset_nvals[p]; v += 256) counts[t.pset_cnt_off[p] + v] = t.pset_counts[p][v];
    __syncthreads();
    build_spread_table<256>(t, lds ? counts : nullptr, tab, scratch);
}

// Score parts of the winner straight into its record (eval_node<true> with
// the parts in the record, not in a stack array, which would live in scratch).
__device__ __forceinline__ void record_winner(const SweepArgs& A, uint32_t row, pe_ranked_node* o) {
    NodeIn in;
    load_node(A.soa, A.tg, row, in);
    ScoreIn si;
    (void)status_loaded(A.soa, A.tg, A.tg.class_ok, A.ask, 0u, row, in, &si, A.spread_tab);
    lookup_scores(A.tg, A.penalty_bits, A.spread_tab, row, in.r.cls, &si);
    for (int k = 0; k < PE_MAX_SCORES; k++) o->scores[k] = 0.0;
    uint32_t ns;
    o->final_score = score_into<true>(A.ask, A.log10, si, o->scores, &ns);
    o->n_scores = ns;
}

// Score parts of one node (the winner's RankedNode record).
__global__ void k_node_record(SweepArgs A, uint32_t row, pe_ranked_node* out) {
    if (threadIdx.x != 0) return;
    record_winner(A, row, out);
    record_offers(A.soa, A.ask, A.tg, row, 0u, out);
}

// One placement of the device-resident full-pass count loop (pe_place on long
// lists), after this placement's k_sweep: thread 0 merges the per-block
// SweepRecs (k_sweep_merge), resolves the Select result (sweep_finish +
// k_node_record) and commits the winner (k_commit with the record's device
// offers); then the workgroup rebuilds the spread table for the next
// placement from the updated counts (k_spread_table). state[0]: a nil Select
// ended the loop (later steps do nothing); state[1]: placements so far.
__device__ __forceinline__ void step_block(const SweepArgs& A, uint32_t nrecs, const uint32_t* visit, uint32_t n,
                                           uint32_t offset, pe_ranked_node* out, uint32_t* state) {
    __shared__ uint32_t counts[kLdsPsetValues];
    __shared__ uint32_t scratch[4];
    __shared__ SweepRec red[4];
    __shared__ uint32_t go;
    if (state[0]) return;   // every thread reads the flag before thread 0 may set it
    SweepRec rec;
    rec_init(rec);
    for (uint32_t i = threadIdx.x; i < nrecs; i += 256) rec_merge(rec, A.recs[i]);
    rec_block_reduce<256>(rec, red);
    if (threadIdx.x == 0) {
        go = 0;
        {
            pe_ranked_node* o = out + state[1];
            pe_ranked_node z = {};
            *o = z;
            o->row = -1;
            o->nodes_evaluated = n;            // a full pass pulls every node
            o->nodes_filtered = rec.filtered;
            o->nodes_exhausted = rec.exhausted;
            o->new_offset = offset;            // and leaves the cursor where it is
            const uint32_t rank = rec_winner(rec);
            if (rank == kEmpty) {
                state[0] = 1;
            } else {
                uint32_t pos = offset + rank;
                if (pos >= n) pos -= n;
                const uint32_t row = visit[pos];
                o->row = (int32_t)row;
                record_winner(A, row, o);
                record_offers(A.soa, A.ask, A.tg, row, 0u, o);
                uint32_t offers = 0xFFFFFFFFu;
                if (o->n_device_offers) {
                    offers = 0;
                    for (uint32_t q = 0; q < o->n_device_offers && q < 4; q++)
                        offers |= (o->device_offer_group[q] & 255u) << (8 * q);
                }
                commit_row(A.soa, A.tg, A.ask, row, offers);
                state[1] += 1;
                go = A.spread_tab != nullptr;
            }
        }
    }
    __syncthreads();
    if (!go) return;   // workgroup-uniform
    const TgTables& t = A.tg;
    const bool lds = t.pset_cnt_total <= (uint32_t)kLdsPsetValues;   // else the HBM counts
    if (lds)
        for (int p = 0; p < t.n_psets; p++)
            for (int v = threadIdx.x; v < t.pset_nvals[p]; v += 256) counts[t.pset_cnt_off[p] + v] = t.pset_counts[p][v];
    __syncthreads();
    build_spread_table<256>(t, lds ? counts : nullptr, const_cast<double*>(A.spread_tab), scratch);
}

__global__ void __launch_bounds__(256) k_sweep_step(SweepArgs A, uint32_t nrecs, const uint32_t* visit, uint32_t n,
                                                    uint32_t offset, pe_ranked_node* out, uint32_t* state) {
    step_block(A, nrecs, visit, n, offset, out, state);
}

// The whole full-pass count loop in one workgroup, for lists whose options
// fit LDS. A commit changes only the committed node's own inputs (use,
// collisions, devices, distinct_hosts) and the spread boosts (one value per
// property value), and a node that is filtered or exhausted stays so while
// the loop only adds allocations. So the workgroup evaluates the list once
// and keeps one LDS entry per option: its visit position, status, the sum of
// its scores before the spread one (score_head: binpack, device affinity,
// anti-affinity, penalty, affinity, summed left to right) and its spread
// property values. A placement then reads 16 bytes of LDS per option, adds
// the spread boost and normalises exactly as score_option does. The maximum
// is found on approximate scores (sum x 1/k, within 2^-52 relative of
// sum / k): only the options within a 2^-48 margin of a wave's maximum take
// the exact quotient, and (max score, earliest rank) is reduced over those;
// a non-positive maximum takes the exact LimitIterator skip record instead
// (rec_add / rec_winner). Two lanes of wave 0 then
// load the winner once and evaluate it side by side: lane 0 as it stands
// (dk = 0: the placement's record, parts written straight into it), lane 1
// with the placement added (dk = 1: the option's new entry, as the overlay
// chain does); lane 0 commits to the SoA and, for target spreads, refreshes
// the one boost per property whose count moved (even spreads rebuild the
// table). One launch for the whole loop; results equal `count` x (k_sweep +
// k_sweep_step). More options than entries: state[5] = 1 before any commit
// and the host runs the multi-workgroup loop instead. The arguments come
// through a device buffer: the TgTables arrays are indexed by property at
// run time, which would copy a by-value argument to scratch.
}  // namespace pe
// ROCm device library wave reduction (DPP), also behind __reduce_max_sync
extern "C" __device__ __attribute__((const)) double __ockl_wfred_max_f64(double);
namespace pe {

constexpr int kFullThreads = 1024;
constexpr int kFullWaves = kFullThreads / 64;
constexpr int kFullPer = 9;                               // entries per thread
constexpr uint32_t kFullCap = kFullThreads * kFullPer;    // LDS entries (16 B each)

__device__ __forceinline__ double readlane_f64(double x, int l) {
    const unsigned long long u = __double_as_longlong(x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

template <int NP>   // spread properties scored (A.spread_tab ? n_psets : 0), at most kAuxPsets
__global__ void __launch_bounds__(kFullThreads) k_fullpass_lds(const SweepArgs* __restrict__ Ap, const uint32_t* visit,
                                                               uint32_t n, uint32_t count, pe_ranked_node* out,
                                                               uint32_t* state, unsigned long long* prof) {
    const SweepArgs& A = *Ap;
    extern __shared__ double ent_sum[];                                    // [kFullCap] score_head sums
    uint32_t* ent_meta = reinterpret_cast<uint32_t*>(ent_sum + kFullCap);   // status | k << 2 | spread values
    uint32_t* ent_pos = ent_meta + kFullCap;                                // visit position
    // the pset_tab_off / pset_cnt_off layout of at most kAuxPsets sets of < kAuxValues values
    __shared__ double tab[kAuxPsets * (kAuxValues + 1)];
    __shared__ double desired[kAuxPsets * kAuxValues];
    __shared__ uint32_t counts[kAuxPsets * kAuxValues];
    __shared__ double aff_lds[kAuxValues];
    __shared__ double red_s[kFullWaves];
    __shared__ uint32_t red_r[kFullWaves];
    __shared__ uint32_t red_f[kFullWaves], red_e[kFullWaves];
    __shared__ SweepRec red[kFullWaves];
    __shared__ uint32_t scratch[4];
    __shared__ uint32_t sh_nf, sh_ne, sh_stop, sh_win, sh_m;
    __shared__ double parts1[PE_MAX_SCORES];   // lane 1's parts (unused)
    __shared__ double rcp_k[8];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const TgTables& t = A.tg;
    constexpr int np = NP;
    const uint32_t off = A.offset;
    bool any_even = false;
    for (int p = 0; p < np; p++) any_even = any_even || t.pset_even[p];
    for (int i = tid; i < kAuxValues; i += kFullThreads) aff_lds[i] = A.aff_vals[i];
    if (tid < 8) rcp_k[tid] = tid ? 1.0 / (double)tid : 0.0;
    if (tid == 0) sh_m = 0;
    for (int p = 0; p < np; p++)
        for (int v = tid; v < t.pset_nvals[p]; v += kFullThreads) {
            counts[t.pset_cnt_off[p] + v] = t.pset_counts[p][v];
            desired[t.pset_cnt_off[p] + v] = t.pset_even[p] ? 0.0 : t.pset_desired[p][v];
        }
    __syncthreads();
    if (np) build_spread_table<kFullThreads>(t, counts, tab, scratch);
    auto spread_of = [&](uint32_t meta) __attribute__((always_inline)) -> double {   // lookup_scores' total
        double sp = 0.0;
#pragma unroll
        for (int p = 0; p < np; p++) {
            const uint32_t v = (meta >> (8 + 8 * p)) & 255u;
            sp += (v == kAuxMissing) ? -1.0 : tab[t.pset_tab_off[p] + v];
        }
        return sp;
    };
    auto load = [&](uint32_t row, NodeIn& in) __attribute__((always_inline)) -> uint32_t {   // the sweep's AUX fetch
        in.r = A.soa.rec[row];
        in.coll_tg = t.coll_tg[row];
        in.dev_free = t.dev_free ? t.dev_free[row] : 0u;
        const uint32_t aux = A.node_aux[row];
        in.feas = aux >> 31;
        return aux;
    };
    // status and score_head of a loaded node with dk placements of this loop
    // added; with a `parts` pointer the parts are written there
    auto head = [&](uint32_t row, const NodeIn& in, uint32_t aux, uint32_t dk, double* parts, double* sum,
                    uint32_t* kk) __attribute__((always_inline)) -> int {
        ScoreIn si;
        const int st = status_loaded(A.soa, t, t.class_ok, A.ask, dk, row, in, &si);
        *kk = 0;
        *sum = 0.0;
        if (st == kOption) {
            si.penalty = A.penalty_bits ? (A.penalty_bits[row >> 5] >> (row & 31)) & 1u : 0u;
            si.aff = aff_lds[aux & 255u];
            si.spread = 0.0;
            *sum = parts ? score_head<true>(A.ask, A.log10, si, parts, *kk)
                         : score_head<false>(A.ask, A.log10, si, nullptr, *kk);
        }
        return st;
    };
    // the final score of an entry (score_option's tail)
    auto final_sum = [&](uint32_t e, uint32_t* kk_out) __attribute__((always_inline)) -> double {
        const uint32_t meta = ent_meta[e];
        double sum = ent_sum[e];
        const double sp = spread_of(meta);
        uint32_t kk = (meta >> 2) & 7u;
        if (sp != 0.0) { sum += sp; kk++; }
        *kk_out = kk;
        return sum;
    };
    uint32_t nf = 0, ne = 0;
    for (uint32_t pos = tid; pos < n; pos += kFullThreads) {
        const uint32_t row = visit[pos];
        NodeIn in;
        const uint32_t aux = load(row, in);
        double s;
        uint32_t kk;
        const int st = head(row, in, aux, 0u, nullptr, &s, &kk);
        nf += st == kFiltered;
        ne += st == kExhausted;
        if (st == kOption) {
            const uint32_t e = atomicAdd(&sh_m, 1u);
            if (e < kFullCap) {
                ent_sum[e] = s;
                ent_meta[e] = (uint32_t)st | (kk << 2) | (aux & 0x00FFFF00u);
                ent_pos[e] = pos;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        nf += (uint32_t)__shfl_xor((int)nf, o);
        ne += (uint32_t)__shfl_xor((int)ne, o);
    }
    if (lane == 0) { red_f[wid] = nf; red_e[wid] = ne; }
    __syncthreads();
    const uint32_t m = sh_m;
    if (m > kFullCap) {   // uniform: nothing committed yet, the host takes the other loop
        if (tid == 0) state[5] = 1;
        return;
    }
    if (tid == 0) {
        uint32_t a = 0, b = 0;
        for (int w = 0; w < kFullWaves; w++) { a += red_f[w]; b += red_e[w]; }
        sh_nf = a;
        sh_ne = b;
        sh_stop = 0;
    }
    __syncthreads();
    auto rank_of_pos = [&](uint32_t pos) __attribute__((always_inline)) -> uint32_t {
        return pos >= off ? pos - off : pos + n - off;
    };
    __shared__ unsigned long long sh_wprof[4];   // PE_FULL_PROF: the winner lane's load / score / record+commit
    if (prof && tid < 4) sh_wprof[tid] = 0;
    unsigned long long tp[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tl = prof ? wall_clock64() : 0;
    auto mark = [&](int i) __attribute__((always_inline)) {
        if (prof && tid == 0) {
            const unsigned long long x = wall_clock64();
            tp[i] += x - tl;
            tl = x;
        }
    };
    for (uint32_t it = 0; it < count; it++) {
        double ap[kFullPer];
        double amax = -__builtin_inff();
#pragma unroll
        for (int j = 0; j < kFullPer; j++) {
            const uint32_t e = (uint32_t)tid + (uint32_t)j * kFullThreads;
            ap[j] = -__builtin_inff();
            if (e < m) {
                uint32_t kk;
                const double sum = final_sum(e, &kk);
                if ((ent_meta[e] & 3u) == (uint32_t)kOption) ap[j] = sum * rcp_k[kk];
            }
            amax = ap[j] > amax ? ap[j] : amax;
        }
        mark(4);
        amax = __ockl_wfred_max_f64(amax);
        mark(5);
        const double cut = amax - (__builtin_fabs(amax) * 0x1p-48 + 0x1p-1000);
        double best = -__builtin_inff();
        uint32_t best_rank = 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < kFullPer; j++) {
            const bool near = ap[j] >= cut && ap[j] != -__builtin_inff();   // options only
            if (__ballot(near)) {
                if (near) {
                    const uint32_t e = (uint32_t)tid + (uint32_t)j * kFullThreads;
                    uint32_t kk;
                    const double sc = final_sum(e, &kk) / (double)kk;
                    const uint32_t rk = rank_of_pos(ent_pos[e]);
                    if (sc > best || (sc == best && rk < best_rank)) { best = sc; best_rank = rk; }
                }
            }
        }
        mark(6);
        {   // the wave's (max, earliest rank) over its few candidate lanes
            uint64_t cand = __ballot(best_rank != 0xFFFFFFFFu);
            double wb = -__builtin_inff();
            uint32_t wr = 0xFFFFFFFFu;
            while (cand) {
                const int l = __builtin_ctzll(cand);
                cand &= cand - 1;
                const double b = readlane_f64(best, l);
                const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)best_rank, l);
                if (b > wb || (b == wb && r < wr)) { wb = b; wr = r; }
            }
            best = wb;
            best_rank = wr;
        }
        mark(7);
        if (lane == 0) { red_s[wid] = best; red_r[wid] = best_rank; }
        // Each wave's lanes 0-1 look their wave's candidate row up now (the
        // winner is one of the waves' candidates): the dependent visit load
        // overlaps the barrier and the resolve, and the winning wave loads its
        // candidate's node straight after. (Loading the whole node here keeps
        // ~20 more VGPRs live across the barrier: they spill.)
        const uint32_t my_rank = best_rank;   // wave-uniform
        uint32_t c_row = 0;
        if (lane < 2 && my_rank != 0xFFFFFFFFu) {
            uint32_t pos = off + my_rank;
            if (pos >= n) pos -= n;
            c_row = visit[pos];
        }
        __syncthreads();
        mark(0);
        // every wave resolves the block's winner itself (no second barrier):
        // the maximum score, then the earliest rank among the waves holding it
        best = lane < kFullWaves ? red_s[lane] : -__builtin_inff();
        best_rank = lane < kFullWaves ? red_r[lane] : 0xFFFFFFFFu;
        best = __ockl_wfred_max_f64(best);
        uint32_t win = __ockl_wfred_min_u32(lane < kFullWaves && red_s[lane] == best ? best_rank : 0xFFFFFFFFu);
        if (win != 0xFFFFFFFFu && !(best > 0.0)) {   // every option non-positive: the skip rule decides (rare)
            SweepRec r;
            rec_init(r);
            for (uint32_t e = tid; e < m; e += kFullThreads) {
                if ((ent_meta[e] & 3u) != (uint32_t)kOption) continue;
                uint32_t kk;
                const double sum = final_sum(e, &kk);
                rec_add(r, rank_of_pos(ent_pos[e]), sum / (double)kk);
            }
            rec_block_reduce<kFullThreads>(r, red);
            if (tid == 0) sh_win = rec_winner(r);
            __syncthreads();
            win = sh_win;
        }
        mark(1);
        pe_ranked_node* o = out + it;
        // the wave whose candidate won evaluates it; when the skip rule picked
        // a rank no wave held (every option non-positive), wave 0 loads it
        bool mine = win != 0xFFFFFFFFu && my_rank == win;
        if (win != 0xFFFFFFFFu && wid == 0 &&
            __ballot(lane < kFullWaves && red_r[lane] == win) == 0) {   // wave-uniform
            mine = true;
            if (lane < 2) {
                uint32_t pos = off + win;
                if (pos >= n) pos -= n;
                c_row = visit[pos];
            }
        }
        if (wid == 0 && win == 0xFFFFFFFFu) {
            if (lane == 0) {
                o->row = -1;
                o->nodes_evaluated = n;            // a full pass pulls every node
                o->nodes_filtered = sh_nf;
                o->nodes_exhausted = sh_ne;
                o->new_offset = off;
                state[0] = 1;
                sh_stop = 1;
            }
        } else if (mine && lane < 2) {
            const uint32_t row = c_row;
            const unsigned long long w0 = prof ? wall_clock64() : 0;
            NodeIn in;
            const uint32_t aux = load(row, in);
            if (prof) {   // the load's latency alone
                __builtin_amdgcn_s_waitcnt(0);
                if (lane == 0) sh_wprof[0] += wall_clock64() - w0;
            }
            const unsigned long long w1 = prof ? wall_clock64() : 0;
            double s;
            uint32_t kk;
            const int st = head(row, in, aux, (uint32_t)lane, lane == 0 ? o->scores : parts1, &s, &kk);
            if (prof && lane == 0) sh_wprof[1] += wall_clock64() - w1;
            const unsigned long long w2 = prof ? wall_clock64() : 0;
            const int st1 = __shfl(st, 1);
            const uint32_t meta0 = (aux & 0x00FFFF00u);   // spread values: the entry's
            if (lane == 1) {
                sh_win = (uint32_t)st | (kk << 2) | meta0;
                parts1[0] = s;
            } else {           // the placement's record, then the commit
                const double sp = spread_of(meta0);
                if (sp != 0.0) {   // SpreadIterator (spread.go:110-174)
                    s += sp;
                    o->scores[kk] = sp;
                    kk++;
                }
                o->row = (int32_t)row;
                o->final_score = s / (double)kk;   // ScoreNormalizationIterator (rank.go:762-767)
                o->n_scores = kk;
                o->nodes_evaluated = n;            // a full pass pulls every node
                o->nodes_filtered = sh_nf;
                o->nodes_exhausted = sh_ne;
                o->new_offset = off;               // and leaves the cursor where it is
                record_offers(A.soa, A.ask, t, row, 0u, o);
                uint32_t offers = 0xFFFFFFFFu;
                if (o->n_device_offers) {
                    offers = 0;
                    for (uint32_t q = 0; q < o->n_device_offers && q < 4; q++)
                        offers |= (o->device_offer_group[q] & 255u) << (8 * q);
                }
                const bool fast = A.ask.n_dev == 0 && A.ask.cores == 0 && np == t.n_psets;
                if (fast) {   // commit_row from the loaded values: stores only
                    NodeRec& r = A.soa.rec[row];
                    r.used_cpu = in.r.used_cpu + A.ask.cpu;
                    r.used_mem = in.r.used_mem + A.ask.mem;
                    r.used_disk = in.r.used_disk + A.ask.disk;
                    r.used_mbits = in.r.used_mbits + A.ask.commit_mbits;
                    r.used_dyn = in.r.used_dyn + A.ask.commit_dyn;
                    A.soa.coll_job[row] += 1;
                    t.coll_tg[row] = in.coll_tg + 1;
                } else {
                    commit_row(A.soa, t, A.ask, row, offers);
                }
#pragma unroll
                for (int p = 0; p < np; p++) {
                    const uint32_t v = (meta0 >> (8 + 8 * p)) & 255u;
                    if (v == kAuxMissing) continue;
                    const uint32_t c = ++counts[t.pset_cnt_off[p] + v];
                    if (fast) t.pset_counts[p][v] = c;
                    if (!t.pset_even[p]) {       // build_spread_table's target boost of this value
                        const double d = desired[t.pset_cnt_off[p] + v];
                        tab[t.pset_tab_off[p] + v] = d != d ? -1.0 : ((d - (double)(c + 1u)) / d) *
                                                                     t.pset_weight_frac[p];
                    }
                }
                state[1] = it + 1;
                sh_nf += st1 == kFiltered;
                sh_ne += st1 == kExhausted;
                if (prof) sh_wprof[2] += wall_clock64() - w2;
            }
        }
        mark(2);
        __syncthreads();
        if (sh_stop) break;
        if (win != 0xFFFFFFFFu) {   // the winner's entry with this placement added
            uint32_t pos = off + win;
            if (pos >= n) pos -= n;
#pragma unroll
            for (int j = 0; j < kFullPer; j++) {
                const uint32_t e = (uint32_t)tid + (uint32_t)j * kFullThreads;
                if (e < m && ent_pos[e] == pos) {
                    ent_sum[e] = parts1[0];
                    ent_meta[e] = sh_win;
                }
            }
        }
        if (any_even) build_spread_table<kFullThreads>(t, counts, tab, scratch);
        __syncthreads();
        mark(3);
    }
    if (prof && tid == 0)
        for (int i = 0; i < 8; i++) prof[i] = tp[i];
    if (prof && tid == 0)
        for (int i = 0; i < 3; i++) prof[8 + i] = sh_wprof[i];
    // the HBM table the next Select starts from
    for (int p = 0; p < np; p++)
        for (int v = tid; v < t.pset_nvals[p]; v += kFullThreads)
            const_cast<double*>(A.spread_tab)[t.pset_tab_off[p] + v] = tab[t.pset_tab_off[p] + v];
}

// The full-pass loop with a service wave (C3's shape: target spreads, no
// device asks or reserved cores). Waves 0-14 hold the options (kSvcPer per
// lane) and run each placement's approximate and exact passes as
// k_fullpass_lds does; wave 15 serves the winners one placement behind. The
// build gives every option its entry with one more placement of the loop as
// well (next sum / meta), so at the resolve thread 0 swaps the winner's next
// entry in and updates its spread boost, and the next placement's passes start
// at once. Meanwhile the service wave loads the winner, writes its record
// (lane 0, dk = 0), evaluates the entry two placements on (lane 1, dk = 2:
// the next entry the winner swaps in) and commits it. The next placement's
// barrier waits for the service, so a winner's next entry is in place before
// it can win again. Results equal k_fullpass_lds. More options than kSvcCap:
// state[5] = 1 before any commit (the host runs k_fullpass_lds instead).
constexpr int kSvcEntryWaves = kFullWaves - 1;
constexpr int kSvcEntryLanes = kSvcEntryWaves * 64;
constexpr int kSvcPer = 4;
constexpr uint32_t kSvcCap = (uint32_t)kSvcEntryLanes * kSvcPer;   // 3840 options, 32 B of LDS each

// LEAN (the host checks): no distinct_hosts, no network asks or static ports,
// no devices, no reserved cores, no distinct_property, no multi-device record:
// an option of the build stays feasible, and the service's evaluation with dk
// placements added is AllocsFit's three comparisons and the scores
// (status_loaded + score_head reduced to the branches such an ask takes).
template <int NP, bool LEAN>
__global__ void __launch_bounds__(kFullThreads) k_fullpass_svc(const SweepArgs* __restrict__ Ap, const uint32_t* visit,
                                                               uint32_t n, uint32_t count, pe_ranked_node* out,
                                                               uint32_t* state) {
    const SweepArgs& A = *Ap;
    extern __shared__ double svc_sum[];                                      // [kSvcCap] score_head sums
    double* next_sum = svc_sum + kSvcCap;                                     // ... with one more placement
    uint32_t* ent_meta = reinterpret_cast<uint32_t*>(next_sum + kSvcCap);     // status | k << 2 | spread values
    uint32_t* next_meta = ent_meta + kSvcCap;
    uint32_t* ent_rank = next_meta + kSvcCap;                                 // visit rank (LimitIterator order)
    uint32_t* ent_row = ent_rank + kSvcCap;
    __shared__ double tab[kAuxPsets * (kAuxValues + 1)];
    __shared__ double desired[kAuxPsets * kAuxValues];
    __shared__ uint32_t counts[kAuxPsets * kAuxValues];
    __shared__ double aff_lds[kAuxValues];
    __shared__ double red_s[kFullWaves];
    __shared__ uint32_t red_r[kFullWaves], red_e[kFullWaves], red_f[kFullWaves], red_x[kFullWaves];
    __shared__ SweepRec red[kFullWaves];
    __shared__ uint32_t scratch[4];
    __shared__ uint32_t sh_nf, sh_ne, sh_stop, sh_win, sh_win_e, sh_m;
    __shared__ uint32_t pend_on, pend_e, pend_nf, pend_ne, pend_it;   // the winner the service wave serves next
    __shared__ double pend_sp;                                        // its spread score at its placement
    __shared__ double parts1[PE_MAX_SCORES];                          // lane 1's parts (unused)
    __shared__ double rcp_k[8];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const TgTables& t = A.tg;
    constexpr int np = NP;
    const uint32_t off = A.offset;
    for (int i = tid; i < kAuxValues; i += kFullThreads) aff_lds[i] = A.aff_vals[i];
    if (tid < 8) rcp_k[tid] = tid ? 1.0 / (double)tid : 0.0;
    if (tid == 0) { sh_m = 0; pend_on = 0; }
    for (int p = 0; p < np; p++)
        for (int v = tid; v < t.pset_nvals[p]; v += kFullThreads) {
            counts[t.pset_cnt_off[p] + v] = t.pset_counts[p][v];
            desired[t.pset_cnt_off[p] + v] = t.pset_desired[p][v];   // target spreads only (the host checks)
        }
    __syncthreads();
    if (np) build_spread_table<kFullThreads>(t, counts, tab, scratch);
    auto spread_of = [&](uint32_t meta) __attribute__((always_inline)) -> double {   // lookup_scores' total
        double sp = 0.0;
#pragma unroll
        for (int p = 0; p < np; p++) {
            const uint32_t v = (meta >> (8 + 8 * p)) & 255u;
            sp += (v == kAuxMissing) ? -1.0 : tab[t.pset_tab_off[p] + v];
        }
        return sp;
    };
    auto load = [&](uint32_t row, NodeIn& in) __attribute__((always_inline)) -> uint32_t {   // the sweep's AUX fetch
        in.r = A.soa.rec[row];
        in.coll_tg = t.coll_tg[row];
        in.dev_free = t.dev_free ? t.dev_free[row] : 0u;
        const uint32_t aux = A.node_aux[row];
        in.feas = aux >> 31;
        return aux;
    };
    // status and score_head of a loaded node with dk placements of this loop
    // added; with a `parts` pointer the parts are written there
    auto head = [&](uint32_t row, const NodeIn& in, uint32_t aux, uint32_t dk, double* parts, double* sum,
                    uint32_t* kk) __attribute__((always_inline)) -> int {
        ScoreIn si;
        const int st = status_loaded(A.soa, t, t.class_ok, A.ask, dk, row, in, &si);
        *kk = 0;
        *sum = 0.0;
        if (st == kOption) {
            si.penalty = A.penalty_bits ? (A.penalty_bits[row >> 5] >> (row & 31)) & 1u : 0u;
            si.aff = aff_lds[aux & 255u];
            si.spread = 0.0;
            *sum = parts ? score_head<true>(A.ask, A.log10, si, parts, *kk)
                         : score_head<false>(A.ask, A.log10, si, nullptr, *kk);
        }
        return st;
    };
    auto final_sum = [&](uint32_t e, uint32_t* kk_out) __attribute__((always_inline)) -> double {
        const uint32_t meta = ent_meta[e];
        double sum = svc_sum[e];
        const double sp = spread_of(meta);
        uint32_t kk = (meta >> 2) & 7u;
        if (sp != 0.0) { sum += sp; kk++; }
        *kk_out = kk;
        return sum;
    };
    auto rank_of_pos = [&](uint32_t pos) __attribute__((always_inline)) -> uint32_t {
        return pos >= off ? pos - off : pos + n - off;
    };
    // build: every option's entry now and with one more placement of the loop
    uint32_t nf = 0, ne = 0;
    for (uint32_t pos = tid; pos < n; pos += kFullThreads) {
        const uint32_t row = visit[pos];
        NodeIn in;
        const uint32_t aux = load(row, in);
        double s;
        uint32_t kk;
        const int st = head(row, in, aux, 0u, nullptr, &s, &kk);
        nf += st == kFiltered;
        ne += st == kExhausted;
        if (st == kOption) {
            const uint32_t e = atomicAdd(&sh_m, 1u);
            if (e < kSvcCap) {
                svc_sum[e] = s;
                ent_meta[e] = (uint32_t)st | (kk << 2) | (aux & 0x00FFFF00u);
                ent_rank[e] = rank_of_pos(pos);
                ent_row[e] = row;
                double s1;
                uint32_t k1;
                const int st1 = head(row, in, aux, 1u, nullptr, &s1, &k1);
                next_sum[e] = s1;
                next_meta[e] = (uint32_t)st1 | (k1 << 2) | (aux & 0x00FFFF00u);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        nf += (uint32_t)__shfl_xor((int)nf, o);
        ne += (uint32_t)__shfl_xor((int)ne, o);
    }
    if (lane == 0) { red_f[wid] = nf; red_x[wid] = ne; }
    __syncthreads();
    const uint32_t m = sh_m;
    if (m > kSvcCap) {   // uniform: nothing committed yet, the host takes the other loop
        if (tid == 0) state[5] = 1;
        return;
    }
    if (tid == 0) {
        uint32_t a = 0, b = 0;
        for (int w = 0; w < kFullWaves; w++) { a += red_f[w]; b += red_x[w]; }
        sh_nf = a;
        sh_ne = b;
        sh_stop = 0;
    }
    __syncthreads();
    // the service of one winner (lanes 0 and 1 of wave 15): its record (lane
    // 0: the placement's state, dk = 0), its entry two placements on (lane 1,
    // dk = 2: what it swaps in when it wins again), the commit (lane 0)
    auto serve = [&]() __attribute__((always_inline)) {
        const uint32_t e = pend_e, row = ent_row[e];
        pe_ranked_node* o = out + pend_it;
        NodeIn in;
        const uint32_t aux = load(row, in);
        double s;
        uint32_t kk;
        // both lanes take the parts-keeping path (lockstep, no divergence)
        int st;
        if (LEAN) {
            const uint32_t dk = lane == 0 ? 0u : 2u;
            const NodeRec& r = in.r;
            const int64_t ucpu = r.used_cpu + (int64_t)(dk + 1) * A.ask.cpu;
            const int64_t umem = r.used_mem + (int64_t)(dk + 1) * A.ask.mem;
            const int64_t udisk = r.used_disk + (int64_t)(dk + 1) * A.ask.disk;
            s = 0.0;
            kk = 0;
            if (r.cap_cpu < ucpu || r.cap_mem < umem || r.cap_disk < udisk) {   // AllocsFit
                st = kExhausted;
            } else {
                ScoreIn si;
                si.ccpu = r.cap_cpu;
                si.cmem = r.cap_mem;
                si.ucpu = ucpu;
                si.umem = umem;
                si.dev_aff = 0.0;
                si.coll = in.coll_tg + dk;
                si.penalty = A.penalty_bits ? (A.penalty_bits[row >> 5] >> (row & 31)) & 1u : 0u;
                si.aff = aff_lds[aux & 255u];
                si.spread = 0.0;
                s = score_head<true>(A.ask, A.log10, si, lane == 0 ? o->scores : parts1, kk);
                st = kOption;
            }
        } else {
            st = head(row, in, aux, lane == 0 ? 0u : 2u, lane == 0 ? o->scores : parts1, &s, &kk);
        }
        if (lane == 1) {
            next_sum[e] = s;
            next_meta[e] = (uint32_t)st | (kk << 2) | (aux & 0x00FFFF00u);
        } else {
            const double sp = pend_sp;
            if (sp != 0.0) {   // SpreadIterator (spread.go:110-174)
                s += sp;
                o->scores[kk] = sp;
                kk++;
            }
            o->row = (int32_t)row;
            o->final_score = s / (double)kk;   // ScoreNormalizationIterator (rank.go:762-767)
            o->n_scores = kk;
            o->nodes_evaluated = n;            // a full pass pulls every node
            o->nodes_filtered = pend_nf;
            o->nodes_exhausted = pend_ne;
            o->new_offset = off;               // and leaves the cursor where it is
            record_offers(A.soa, A.ask, t, row, 0u, o);
            NodeRec& r = A.soa.rec[row];       // commit_row from the loaded values: stores only
            r.used_cpu = in.r.used_cpu + A.ask.cpu;
            r.used_mem = in.r.used_mem + A.ask.mem;
            r.used_disk = in.r.used_disk + A.ask.disk;
            r.used_mbits = in.r.used_mbits + A.ask.commit_mbits;
            r.used_dyn = in.r.used_dyn + A.ask.commit_dyn;
            A.soa.coll_job[row] += 1;
            t.coll_tg[row] = in.coll_tg + 1;
            pend_on = 0;   // thread 0 sets the next one after the barrier
        }
    };
    for (uint32_t it = 0; it < count; it++) {
        if (wid < kSvcEntryWaves) {
            double ap[kSvcPer];
            double amax = -__builtin_inff();
#pragma unroll
            for (int j = 0; j < kSvcPer; j++) {
                const uint32_t e = (uint32_t)tid + (uint32_t)j * kSvcEntryLanes;
                ap[j] = -__builtin_inff();
                if (e < m) {
                    uint32_t kk;
                    const double sum = final_sum(e, &kk);
                    if ((ent_meta[e] & 3u) == (uint32_t)kOption) ap[j] = sum * rcp_k[kk];
                }
                amax = ap[j] > amax ? ap[j] : amax;
            }
            amax = __ockl_wfred_max_f64(amax);
            const double cut = amax - (__builtin_fabs(amax) * 0x1p-48 + 0x1p-1000);
            double best = -__builtin_inff();
            uint32_t best_rank = 0xFFFFFFFFu, best_e = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < kSvcPer; j++) {
                const bool near = ap[j] >= cut && ap[j] != -__builtin_inff();   // options only
                if (__ballot(near)) {
                    if (near) {
                        const uint32_t e = (uint32_t)tid + (uint32_t)j * kSvcEntryLanes;
                        uint32_t kk;
                        const double sc = final_sum(e, &kk) / (double)kk;
                        const uint32_t rk = ent_rank[e];
                        if (sc > best || (sc == best && rk < best_rank)) { best = sc; best_rank = rk; best_e = e; }
                    }
                }
            }
            {   // the wave's (max, earliest rank) over its few candidate lanes
                uint64_t cand = __ballot(best_rank != 0xFFFFFFFFu);
                double wb = -__builtin_inff();
                uint32_t wr = 0xFFFFFFFFu, we = 0xFFFFFFFFu;
                while (cand) {
                    const int l = __builtin_ctzll(cand);
                    cand &= cand - 1;
                    const double b = readlane_f64(best, l);
                    const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)best_rank, l);
                    if (b > wb || (b == wb && r < wr)) {
                        wb = b;
                        wr = r;
                        we = (uint32_t)__builtin_amdgcn_readlane((int)best_e, l);
                    }
                }
                if (lane == 0) { red_s[wid] = wb; red_r[wid] = wr; red_e[wid] = we; }
            }
        } else {
            if (pend_on && lane < 2) serve();
            if (lane == 0) { red_s[wid] = -__builtin_inff(); red_r[wid] = 0xFFFFFFFFu; }
        }
        __syncthreads();
        // every thread resolves the block's winner (max score, then the
        // earliest rank among the waves holding it)
        double best = lane < kFullWaves ? red_s[lane] : -__builtin_inff();
        best = __ockl_wfred_max_f64(best);
        uint32_t win = __ockl_wfred_min_u32(lane < kFullWaves && red_s[lane] == best ? red_r[lane] : 0xFFFFFFFFu);
        bool skip_rule = false;
        if (win != 0xFFFFFFFFu && !(best > 0.0)) {   // every option non-positive: the skip rule decides (rare)
            skip_rule = true;
            SweepRec r;
            rec_init(r);
            for (uint32_t e = tid; e < m; e += kFullThreads) {
                if ((ent_meta[e] & 3u) != (uint32_t)kOption) continue;
                uint32_t kk;
                const double sum = final_sum(e, &kk);
                rec_add(r, ent_rank[e], sum / (double)kk);
            }
            rec_block_reduce<kFullThreads>(r, red);
            if (tid == 0) sh_win = rec_winner(r);
            __syncthreads();
            win = sh_win;
            if (win != 0xFFFFFFFFu) {
                for (uint32_t e = tid; e < m; e += kFullThreads)
                    if (ent_rank[e] == win) sh_win_e = e;
            }
            __syncthreads();
        }
        if (tid == 0) {
            pe_ranked_node* o = out + it;
            if (win == 0xFFFFFFFFu) {
                o->row = -1;
                o->nodes_evaluated = n;            // a full pass pulls every node
                o->nodes_filtered = sh_nf;
                o->nodes_exhausted = sh_ne;
                o->new_offset = off;
                state[0] = 1;
                sh_stop = 1;
            } else {
                uint32_t e = sh_win_e;
                if (!skip_rule)
                    for (int w = 0; w < kFullWaves; w++)
                        if (red_s[w] == best && red_r[w] == win) { e = red_e[w]; break; }
                const uint32_t meta0 = ent_meta[e];
                pend_e = e;
                pend_it = it;
                pend_nf = sh_nf;
                pend_ne = sh_ne;
                pend_sp = spread_of(meta0);   // the boost this placement saw
                pend_on = 1;
                // the winner's entry with this placement added
                svc_sum[e] = next_sum[e];
                ent_meta[e] = next_meta[e];
                const uint32_t st1 = next_meta[e] & 3u;
                sh_nf += st1 == (uint32_t)kFiltered;
                sh_ne += st1 == (uint32_t)kExhausted;
#pragma unroll
                for (int p = 0; p < np; p++) {   // the target boost of the winner's value (build_spread_table)
                    const uint32_t v = (meta0 >> (8 + 8 * p)) & 255u;
                    if (v == kAuxMissing) continue;
                    const uint32_t c = ++counts[t.pset_cnt_off[p] + v];
                    t.pset_counts[p][v] = c;
                    const double d = desired[t.pset_cnt_off[p] + v];
                    tab[t.pset_tab_off[p] + v] = d != d ? -1.0 : ((d - (double)(c + 1u)) / d) * t.pset_weight_frac[p];
                }
                state[1] = it + 1;
            }
        }
        __syncthreads();
        if (sh_stop) break;
    }
    if (wid == kSvcEntryWaves && pend_on && lane < 2) serve();   // the last winner
    // the HBM table the next Select starts from
    for (int p = 0; p < np; p++)
        for (int v = tid; v < t.pset_nvals[p]; v += kFullThreads)
            const_cast<double*>(A.spread_tab)[t.pset_tab_off[p] + v] = tab[t.pset_tab_off[p] + v];
}

// node_feas[row] = class_ok[cls] && node_ok[row]: one verdict byte per node so
// the count loop issues a single dependent round trip per node.
// Host -> device upload as a kernel: the source is page-locked mapped host
// memory read directly over the bus (a DMA copy costs more setup per call than
// the whole transfer of these small per-evaluation arrays).
__global__ void __launch_bounds__(256) k_upload(unsigned char* dst, const unsigned char* src, size_t bytes) {
    const size_t n16 = bytes / 16;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride)
        reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    for (size_t i = n16 * 16 + (size_t)blockIdx.x * 256 + threadIdx.x; i < bytes; i += stride) dst[i] = src[i];
}

// Per-node count arrays from a sorted sparse list (key = row << 5 | array,
// value = count): each thread owns one row, zeroes it in every array and
// writes the row's entries found by binary search. A deferred ResetPlan (R.rec)
// rides in the same launch: its arrays are disjoint from the counts.
__global__ void __launch_bounds__(256) k_counts(CountDsts D, uint32_t nd, uint32_t n, const uint2* ents, uint32_t m,
                                                ResetArgs R) {
    counts_apply(D, nd, n, ents, m, R, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// ResetPlan in one launch: the proposed state back to the snapshot (node
// records, device free counts), no plan preemptions.
__global__ void __launch_bounds__(256) k_reset_plan(NodeRec* rec, const NodeRec* base_rec, uint32_t* dev_free,
                                                   const uint32_t* dev_free_base, uint32_t n, uint8_t* preempted,
                                                   uint32_t m, uint32_t* pcount, uint32_t keys) {
    const uint32_t stride = gridDim.x * 256;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        rec[i] = base_rec[i];
        dev_free[i] = dev_free_base[i];
    }
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < m; i += stride) preempted[i] = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < keys; i += stride) pcount[i] = 0;
}

__global__ void __launch_bounds__(256) k_fold_feas(NodeSoA s, const uint8_t* class_ok, const uint8_t* node_ok,
                                                   uint8_t* feas) {
    for (uint32_t row = blockIdx.x * blockDim.x + threadIdx.x; row < s.n; row += gridDim.x * blockDim.x) {
        bool ok = class_ok[s.rec[row].cls] != 0;
        if (node_ok) ok = ok && node_ok[row] != 0;
        feas[row] = ok ? 1 : 0;
    }
}

// k_fold_feas with the class table read from the page-locked staging ring:
// every workgroup pulls the (small) table over the bus into LDS, workgroup 0
// also stores it to its device copy for the later kernels; saves the
// separate upload launch.
__global__ void __launch_bounds__(256) k_fold_feas_staged(NodeSoA s, const uint8_t* class_src, uint8_t* class_dst,
                                                          uint32_t ncls, const uint8_t* node_ok, uint8_t* feas) {
    __shared__ uint8_t cls_ok[kFoldMaxClasses];
    for (uint32_t c = threadIdx.x; c < ncls; c += blockDim.x) {
        const uint8_t v = class_src[c];
        cls_ok[c] = v;
        if (blockIdx.x == 0) class_dst[c] = v;
    }
    __syncthreads();
    for (uint32_t row = blockIdx.x * blockDim.x + threadIdx.x; row < s.n; row += gridDim.x * blockDim.x) {
        const uint32_t c = s.rec[row].cls;
        bool ok = c < ncls && cls_ok[c] != 0;
        if (node_ok) ok = ok && node_ok[row] != 0;
        feas[row] = ok ? 1 : 0;
    }
}

// CSIVolumeChecker.isFeasible per node (CsiArgs, engine_types.h), one lane per
// snapshot row. The request records are staged once per workgroup. A lane
// looks the request's plugin up among its node's plugins (a handful) and, only
// when the node runs it healthy, counts the node's volumes of that plugin
// against MaxVolumes; the volume-level reasons come resolved in the record.
// The first failing request in list order gives the code. The verdict is
// folded into node_ok / node_feas, the per-node bytes every walk kernel reads,
// so an unavailable node is one filtered node to all of them.
__global__ void __launch_bounds__(256) k_csi_avail(CsiArgs A) {
    __shared__ CsiReq req[kMaxCsiReq];
    const uint32_t nr = min(A.n_req, (uint32_t)kMaxCsiReq);
    if (threadIdx.x < nr) req[threadIdx.x] = A.req[threadIdx.x];
    __syncthreads();
    for (uint32_t row = blockIdx.x * 256 + threadIdx.x; row < A.n; row += gridDim.x * 256) {
        const uint32_t pb = A.plug_off[row], pz = A.plug_off[row + 1];
        const uint32_t vb = A.nvol_off[row], ve = A.nvol_off[row + 1];
        uint32_t code = 0;
        for (uint32_t q = 0; q < nr && !code; q++) {
            const CsiReq r = req[q];
            uint32_t reason;
            if (!r.found) {
                reason = PE_CSI_NOT_FOUND;
            } else {
                uint32_t k = pb;
                while (k < pz && A.plug_id[k] != r.plugin) k++;
                if (k == pz) {
                    reason = PE_CSI_NO_PLUGIN;
                } else if (!A.plug_healthy[k]) {
                    reason = PE_CSI_UNHEALTHY;
                } else {
                    int64_t in_use = 0;   // pluginCount[vol.PluginID]
                    for (uint32_t v = vb; v < ve; v++) in_use += A.nvol_plugin[v] == r.plugin;
                    reason = in_use >= A.plug_max[k] ? PE_CSI_MAX_VOLUMES : r.vol_reason;
                }
            }
            if (reason) code = q << 3 | reason;
        }
        A.codes[row] = (uint16_t)code;
        if (!A.node_ok) continue;   // pe_place_csi's columns: the codes alone, nothing folded
        const bool ok = code == 0 && (!A.base_ok || A.base_ok[row] != 0);
        A.node_ok[row] = ok ? 1 : 0;
        A.node_feas[row] = (ok && A.class_ok[A.rec[row].cls] != 0) ? 1 : 0;
    }
}

// F[c] of pe_place_csi's stop rule: the first position, counted from the
// call's cursor without wrapping, at which FeasibilityWrapper.Next would decide
// class c's task-group status (feasible.go:1121-1143): the first node of the
// class that passes the job checks. One lane per visit position, a min over
// positions; classes the memo knows and nodes that fail the job checks do not
// count. `first` is preset to ~0u.
__global__ void __launch_bounds__(256) k_csi_first(const uint32_t* perm, uint32_t n, uint32_t offset,
                                                   const NodeRec* rec, CsiLoopArgs C) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    uint32_t p = offset + j;
    if (p >= n) p -= n;
    const uint32_t row = perm[p];
    const uint32_t c = rec[row].cls;
    if (c >= C.ncls || C.cls_state[c] != kCsiClsOpen) return;
    if (C.job_ok && !C.job_ok[row]) return;
    // a clusterful of lanes shares a handful of classes: only a lane that can still lower the
    // minimum goes to the atomic (a stale read only sends a lane there needlessly)
    if (__hip_atomic_load(&C.first[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= j) return;
    atomicMin(&C.first[c], j);
}

// pe_place_csi's count loop: k_window's shape (one wave, 64 positions per
// chunk, the 128-position register ring of evaluated positions kept across
// placements) with two differences. The ring holds the evaluation *without*
// CSI plus FeasibilityWrapper's own verdict bit; whether a node is available is
// read from the placement's code column when its position is consumed, so a
// new alloc index does not empty the ring. And the LimitIterator /
// MaxScoreIterator fold is csi_limit.h's state machine, stepped by every lane
// in lockstep (uniform state) over the chunk's events in position order: an
// option, or the nil of an unavailable node whose class is memoised eligible
// (at call start, or decided at an earlier position of the call: F[c]). An
// unavailable node of a class not yet decided is skipped and counts as
// filtered, as a stop does.
// Every loop is bounded without the data: chunks by n + skew, the events of a
// chunk by its 64 lanes, the nils after the last position by kCsiTailEvents.
// kMetrics (pe_place_csi_metrics): the trace log, one byte per consumed
// position of the call in consumption order (csi_reason.h: the placement's
// availability code and whether the node was a stop). The index is
// walked + j; the lanes a Select pulled store their byte after the chunk's
// fold, so a Select that ends mid-chunk logs exactly its consumed prefix.
// `log` is mapped page-locked memory of log_cap >= count * n_visit bytes.
template <bool kMetrics>
__global__ void __launch_bounds__(64) k_csi_loop(BatchArgs A, CsiLoopArgs C, uint8_t* log, uint32_t log_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
    const int lane = threadIdx.x;
    const uint32_t n = A.n_visit;
    const uint32_t* perm = A.perms;
    const uint8_t* class_ok = A.tg.class_ok;
    const uint32_t H = 1u << A.hash_bits;
    Overlay ov;
    ov.bits = A.hash_bits;
    ov.mask = H - 1;
    ov.keys = reinterpret_cast<uint32_t*>(dyn_smem);
    ov.k = A.packed_overlay ? nullptr : ov.keys + H;
    ov.kshift = A.packed_overlay;
    ov.kmask = A.packed_overlay ? (1u << A.packed_overlay) - 1u : 0u;
    for (uint32_t i = lane; i < H; i += 64) ov.keys[i] = kEmpty;
    __syncthreads();

    uint32_t offset = n ? A.offset0 % n : 0u;
    uint32_t placed = 0;
    int st0 = kFiltered, st1 = kFiltered;
    double sc0 = 0.0, sc1 = 0.0;
    uint32_t rw0 = kEmpty, rw1 = kEmpty;
    bool wf0 = false, wf1 = false;   // FeasibilityWrapper's verdict without CSI
    uint32_t rb = 0;     // ring index of the cursor
    uint32_t have = 0;   // relative positions [0, have) are cached
    uint64_t walked = 0; // positions consumed since the call began
    uint32_t fold_err = 0;

    for (uint32_t it = 0; n && it < A.count; it++) {
        const uint32_t set = min((uint32_t)C.set_of[it], C.n_sets - 1u);
        const uint16_t* codes = C.codes + (size_t)set * C.n_rows;
        CsiLimit L;
        bool done = csi_limit_init(L, A.limit);
        uint32_t n_filtered = 0, n_exhausted = 0;
        uint32_t consumed = done ? 0u : n;
        const uint32_t skew = rb & 63u;
        for (uint32_t k = 0; !done && 64u * k < n + skew; k++) {
            const int j = (int)(64u * k + (uint32_t)lane) - (int)skew;   // relative visit position
            const bool valid = j >= 0 && (uint32_t)j < n;
            const bool s1 = (((rb >> 6) + k) & 1u) != 0;
            int st = s1 ? st1 : st0;
            double sc = s1 ? sc1 : sc0;
            bool wf = s1 ? wf1 : wf0;
            uint32_t row = s1 ? rw1 : rw0;
            const bool need = valid && (uint32_t)j >= have;
            if (__ballot(need)) {
                // as k_window: this chunk and the next one, all loads first
                const uint32_t j2 = (uint32_t)(j + 64);
                const bool need2 = j2 < n;
                uint32_t p1 = need ? offset + (uint32_t)j : 0u;
                uint32_t p2 = need2 ? offset + j2 : 0u;
                if (p1 >= n) p1 -= n;
                if (p2 >= n) p2 -= n;
                const uint32_t row1 = perm[p1], row2 = perm[p2];
                NodeIn in1, in2;
                load_node(A.soa, A.tg, row1, in1);
                load_node(A.soa, A.tg, row2, in2);
                const bool w1 = class_ok[in1.r.cls] != 0 && (!A.tg.node_ok || A.tg.node_ok[row1] != 0);
                const bool w2 = class_ok[in2.r.cls] != 0 && (!A.tg.node_ok || A.tg.node_ok[row2] != 0);
                const uint32_t dk1 = ov_count(ov, row1), dk2 = ov_count(ov, row2);
                NodeEval e1, e2;
                e1.score = 0.0;
                e2.score = 0.0;
                eval_loaded<false>(A.soa, A.tg, class_ok, A.ask, dk1, A.penalty_bits, A.log10, nullptr, row1, in1,
                                   &e1);
                eval_loaded<false>(A.soa, A.tg, class_ok, A.ask, dk2, A.penalty_bits, A.log10, nullptr, row2, in2,
                                   &e2);
                if (need) {
                    st = e1.status;
                    sc = e1.score;
                    wf = w1;
                    row = row1;
                    if (s1) { st1 = st; sc1 = sc; rw1 = row1; wf1 = w1; } else { st0 = st; sc0 = sc; rw0 = row1; wf0 = w1; }
                }
                if (need2) {
                    if (s1) { st0 = e2.status; sc0 = e2.score; rw0 = row2; wf0 = w2; }
                    else { st1 = e2.status; sc1 = e2.score; rw1 = row2; wf1 = w2; }
                }
                have = min(64u * (k + 2) - skew, n);
            }

            // the availability of this placement, at the time the position is consumed
            const bool reach = valid && wf;   // the node reaches the availability checker
            const bool unavailable = reach && row < C.n_rows && codes[row] != 0;
            bool stop = false;
            if (unavailable && !C.escaped) {
                const uint32_t c = A.soa.rec[row].cls;
                const uint8_t cs = c < C.ncls ? C.cls_state[c] : (uint8_t)kCsiClsNever;
                stop = cs == kCsiClsEligible || (cs == kCsiClsOpen && walked + (uint64_t)j > (uint64_t)C.first[c]);
            }
            const bool is_opt = reach && !unavailable && st == kOption;
            const bool is_exh = reach && !unavailable && st == kExhausted;
            const bool is_filt = valid && !is_opt && !is_exh;
            const uint64_t nil_m = __ballot(stop), opt_m = __ballot(is_opt);
            uint64_t m = nil_m | opt_m;
            int done_lane = 64;
            while (m) {   // at most 64 events: one bit leaves m per turn
                const int l = (int)__ffsll((long long)m) - 1;
                m &= m - 1;
                const double s_l = __shfl(sc, l);
                const uint32_t kind = (nil_m >> l) & 1u ? kCsiNil : kCsiOption;
                if (csi_limit_step(L, kind, s_l, (int32_t)(64u * k + (uint32_t)l) - (int32_t)skew)) {
                    done = true;
                    done_lane = l;
                    break;
                }
            }
            const bool pulled = valid && lane <= done_lane;
            n_filtered += (uint32_t)__popcll(__ballot(pulled && is_filt));
            n_exhausted += (uint32_t)__popcll(__ballot(pulled && is_exh));
            if constexpr (kMetrics) {
                const uint64_t at = walked + (uint64_t)(pulled ? j : 0);
                if (pulled && at < (uint64_t)log_cap)
                    log[at] = csi_log_pack(unavailable ? (uint32_t)codes[row] : 0u, stop);
            }
            if (done) consumed = 64u * k + (uint32_t)done_lane - skew + 1u;
        }
        // StaticIterator has nothing left for this Select: the same nil again and again
        for (int t = 0; t < kCsiTailEvents && !done; t++) done = csi_limit_step(L, kCsiNil, 0.0, -1);
        if (!done) {   // csi_limit.h's bound does not hold: no record, the host fails the call (as pe_csi_limit_fold)
            fold_err = 1u;
            break;
        }

        const int best_pos = L.best_id;
        const double best_score = L.best_score;
        int win_row = -1;
        if (best_pos >= 0 && (uint32_t)best_pos < n) {
            uint32_t pos = offset + (uint32_t)best_pos;
            if (pos >= n) pos -= n;
            win_row = (int)perm[pos];
        }
        uint32_t no = offset + (consumed % n);
        if (no >= n) no -= n;
        if (lane == 0) {
            emit_placement(A, class_ok, ov, nullptr, 0u, it, win_row, best_score, consumed, n_filtered, n_exhausted,
                           no);
            if (win_row >= 0 && A.commit) ov_add(ov, (uint32_t)win_row);
        }
        wave_sync();
        offset = no;
        walked += consumed;
        rb = (rb + consumed) & 127u;
        have = have > consumed ? have - consumed : 0u;
        if (win_row >= 0 && A.commit && have) {
            // the winner's overlay count changed: cut the cache at its first cached position
            const uint32_t j0 = ((uint32_t)lane - rb) & 127u, j1 = (64u + (uint32_t)lane - rb) & 127u;
            const bool bad0 = j0 < have && rw0 == (uint32_t)win_row;
            const bool bad1 = j1 < have && rw1 == (uint32_t)win_row;
            if (__ballot(bad0 || bad1)) {
                uint32_t cut = min(bad0 ? j0 : 128u, bad1 ? j1 : 128u);
                for (int off = 32; off > 0; off >>= 1) cut = min(cut, (uint32_t)__shfl_xor((int)cut, off));
                if (cut < have) have = cut;
            }
        }
        wave_sync();
        if (win_row < 0) break;
        placed++;
    }
    if (lane == 0) {
        A.eval_status[0] = placed;
        A.eval_status[1] = offset;
        A.eval_status[2] = fold_err;
    }
    if (A.writeback) writeback_overlay<64, false>(A, ov, H, nullptr);
}

// node_aux[row] (SweepArgs): verdict bit, affinity index (per class, or per
// node when the affinities escape the class), spread values of the first
// kAuxPsets properties. Built once per (job, task group) tables.
__global__ void __launch_bounds__(256) k_fold_aux(NodeSoA s, TgTables t, const uint8_t* aff_idx_class,
                                                  const uint8_t* aff_idx_node, uint32_t* aux) {
    for (uint32_t row = blockIdx.x * blockDim.x + threadIdx.x; row < s.n; row += gridDim.x * blockDim.x) {
        const uint32_t c = s.rec[row].cls;
        bool ok = t.class_ok[c] != 0;
        if (t.node_ok) ok = ok && t.node_ok[row] != 0;
        uint32_t x = ok ? 1u << 31 : 0u;
        x |= aff_idx_node ? aff_idx_node[row] : (aff_idx_class ? aff_idx_class[c] : 0u);
        for (int p = 0; p < t.n_psets && p < kAuxPsets; p++) {
            const uint32_t v = pset_value(t, p, row, c);
            x |= (v == kMissing ? kAuxMissing : v) << (8 + 8 * p);
        }
        aux[row] = x;
    }
}

// Static port gate of a task group (status_loaded): blocked rows stay 0, the
// others hold the group's collision count + 1 at build time.
__global__ void __launch_bounds__(256) k_static_gate(const uint8_t* blocked, const uint32_t* coll_tg, uint32_t* gate,
                                                     uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) gate[i] = blocked[i] ? 0u : coll_tg[i] + 1u;
}

// Multi-device gates (TgTables::md): the host wrote the admitted placement
// count in `lim` (kMdUnbounded: no limit); the rows get the group's collision
// count at build time added (saturating below ~0u, which marks other rows).
__global__ void __launch_bounds__(256) k_md_gate(MdNet* md, const uint32_t* coll_tg, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    MdNet& m = md[i];
    if (m.lim == ~0u) return;
    const uint32_t c = coll_tg[i];
    m.coll = c;
    const uint64_t lim = (uint64_t)c + m.lim;
    m.lim = (m.lim == kMdUnbounded || lim >= (uint64_t)kMdUnbounded) ? kMdUnbounded : (uint32_t)lim;
}

#include "evict.inc"

// ---- pe_place_destructive: computePlacements' destructive-update loop ----------
// Per update (generic_sched.go:543-645): AppendStoppedAlloc of the previous
// alloc, Select, AppendAlloc on an option; on nil PopUpdate and the loop ends.
// k_window's shape (one wave, 64 positions per chunk, the 128-position register
// ring kept across Selects, the same ballot closed form, the launch's
// placements in the LDS overlay, written back at the end). New is what happens
// before each Select: one lane applies the stop to the HBM columns with plain
// loads and stores (k_plan_stop's arithmetic; one wave owns the launch, so no
// atomics), the wave fences at workgroup scope so that its next load_node sees
// them, and the ring is cut at the first cached position that holds the stopped
// row, wherever it lies ahead of the cursor.
// Stops stay out of the overlay: its k x ask model holds because every
// placement is the same ask. A stop on a row that already holds placements of
// the launch first folds the row's overlay entry into HBM (the entry stays with
// count 0), so the stop meets the node as the per-call sequence's stop does:
// the device offers of the row's later placements are then assigned from the
// counts the stop returned to, in the sequence's order.
// Every loop is bounded without the data: chunks by n + skew, updates by count.
// A slot or row of the stop list out of range raises eval_status[2] and ends
// the call before anything is indexed with it.
__device__ __forceinline__ void ds_fold_row(const BatchArgs& A, const Overlay& ov, uint32_t row) {
    const int h = ov_slot(ov, row);
    if (h < 0) return;
    const uint32_t e = ov.keys[h];
    const uint32_t k = ov.k ? ov.k[h] : e & ov.kmask;
    if (!k) return;
    NodeRec& r = A.soa.rec[row];
    r.used_cpu += (int64_t)k * A.ask.cpu;
    r.used_mem += (int64_t)k * A.ask.mem;
    r.used_disk += (int64_t)k * A.ask.disk;
    r.used_mbits += (int32_t)k * A.ask.commit_mbits;
    r.used_dyn += (int32_t)k * A.ask.commit_dyn;
    A.soa.coll_job[row] += k;
    A.tg.coll_tg[row] += k;
    if (A.ask.n_dev > 0) A.tg.dev_free[row] = dev_after(A.ask, A.tg.dev_cls[r.cls], A.tg.dev_free[row], k);
    if (ov.k) ov.k[h] = 0;
    else ov.keys[h] = e & ~ov.kmask;
}

// AppendStoppedAlloc (sign +1) / PopUpdate (sign -1, the same steps in reverse order) of one update (one lane).
template <class Args>   // BatchArgs (k_destructive) or SweepArgs (k_destructive_full): the node columns and the group's
__device__ __forceinline__ void ds_stop(const Args& A, const DestructiveArgs& D, uint32_t slot, uint32_t row,
                                        uint32_t flags, int sign) {
    const auto resources = [&]() {
        if (!(flags & kDsLive)) return;
        const PreemptAlloc x = D.palloc[slot];
        NodeRec& r = A.soa.rec[row];
        r.used_cpu -= sign * x.cpu;
        r.used_mem -= sign * x.mem;
        r.used_disk -= sign * x.disk;
        r.used_mbits -= sign * x.mbits;
        r.used_dyn -= sign * x.dyn;
        if (D.dev_free) {
            uint32_t d = 0;
            for (int k = 0; k < 4 && k < (int)x.n_dev; k++) d += byte_of(x.dev_c, k) << (8 * byte_of(x.dev_g, k));
            D.dev_free[row] += sign > 0 ? d : 0u - d;
        }
    };
    const auto counts = [&]() {
        const uint32_t one = sign > 0 ? 0xFFFFFFFFu : 1u;   // -1 / +1
        if (flags & kDsJob) {
            A.soa.coll_job[row] += one;
            if (D.own_existing) D.own_existing[row] += one;
        }
        if (flags & kDsTg) A.tg.coll_tg[row] += one;
    };
    if (sign > 0) {
        resources();
        counts();
        if (flags & kDsLive) D.preempted[slot] = 2;
    } else {
        if (flags & kDsLive) D.preempted[slot] = 0;
        counts();
        resources();
    }
}

// The stop's (or its undo's) stores become visible to every lane's next loads
// of the node columns: one CU's vector L1 serves the whole workgroup, so a
// release / acquire pair at workgroup scope (a wait for the stores, no cache
// maintenance) around the wave's ordering point is all it takes.
__device__ __forceinline__ void ds_publish() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    wave_sync();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Cut the cached window [0, have) at the first cached position that holds `row`.
__device__ __forceinline__ uint32_t ds_cut(uint32_t row, uint32_t rb, uint32_t have, uint32_t rw0, uint32_t rw1,
                                           int lane) {
    if (!have) return have;
    const uint32_t j0 = ((uint32_t)lane - rb) & 127u, j1 = (64u + (uint32_t)lane - rb) & 127u;
    const bool bad0 = j0 < have && rw0 == row;
    const bool bad1 = j1 < have && rw1 == row;
    if (__ballot(bad0 || bad1)) {
        uint32_t cut = min(bad0 ? j0 : 128u, bad1 ? j1 : 128u);
        for (int off = 32; off > 0; off >>= 1) cut = min(cut, (uint32_t)__shfl_xor((int)cut, off));
        if (cut < have) have = cut;
    }
    return have;
}

__global__ void __launch_bounds__(64) k_destructive(BatchArgs A, DestructiveArgs D) {
    __shared__ double aside_score[kMaxSkip];
    __shared__ int aside_pos[kMaxSkip];
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
    const int lane = threadIdx.x;
    const uint32_t n = A.n_visit;
    const uint32_t* perm = A.perms;
    const uint8_t* class_ok = A.tg.class_ok;
    const uint32_t H = 1u << A.hash_bits;
    Overlay ov;
    ov.bits = A.hash_bits;
    ov.mask = H - 1;
    ov.keys = reinterpret_cast<uint32_t*>(dyn_smem);
    ov.k = A.packed_overlay ? nullptr : ov.keys + H;
    ov.kshift = A.packed_overlay;
    ov.kmask = A.packed_overlay ? (1u << A.packed_overlay) - 1u : 0u;
    for (uint32_t i = lane; i < H; i += 64) ov.keys[i] = kEmpty;
    __syncthreads();

    uint32_t offset = n ? A.offset0 % n : 0u;
    uint32_t placed = 0;
    int st0 = kFiltered, st1 = kFiltered;
    double sc0 = 0.0, sc1 = 0.0;
    uint32_t rw0 = kEmpty, rw1 = kEmpty;
    uint32_t rb = 0;     // ring index of the cursor
    uint32_t have = 0;   // relative positions [0, have) are cached (have <= min(n, 128) at loop top)
    uint32_t guard = 0;

    for (uint32_t it = 0; n && it < A.count; it++) {
        // ---- AppendStoppedAlloc(allocs[it]) ----
        const uint32_t s_slot = D.stops[kDsWords * it], s_row = D.stops[kDsWords * it + 1];
        const uint32_t s_flags = D.stops[kDsWords * it + 2];
        if (s_flags) {
            if (s_row >= A.soa.n || ((s_flags & kDsLive) && s_slot >= D.n_slots)) {
                guard = 1u;
                break;
            }
            if (lane == 0) {
                ds_fold_row(A, ov, s_row);
                ds_stop(A, D, s_slot, s_row, s_flags, +1);
            }
            ds_publish();
            have = ds_cut(s_row, rb, have, rw0, rw1, lane);
        }

        // ---- Select: k_window's pull ----
        uint32_t r = 0, a = 0;
        double best_score = -__builtin_inf();
        int best_pos = -1;
        uint32_t n_filtered = 0, n_exhausted = 0;
        uint32_t consumed = n;
        bool stopped = false;
        double lbest_s = -__builtin_inf();
        int lbest_p = -1;
        const uint32_t skew = rb & 63u;
        for (uint32_t k = 0; 64u * k < n + skew; k++) {
            const int j = (int)(64u * k + (uint32_t)lane) - (int)skew;   // relative visit position
            const bool valid = j >= 0 && (uint32_t)j < n;
            const bool s1 = (((rb >> 6) + k) & 1u) != 0;
            int st = s1 ? st1 : st0;
            double sc = s1 ? sc1 : sc0;
            const bool need = valid && (uint32_t)j >= have;
            if (__ballot(need)) {
                // as k_window: this chunk and the next one, all loads first
                const uint32_t j2 = (uint32_t)(j + 64);
                const bool need2 = j2 < n;
                uint32_t p1 = need ? offset + (uint32_t)j : 0u;
                uint32_t p2 = need2 ? offset + j2 : 0u;
                if (p1 >= n) p1 -= n;
                if (p2 >= n) p2 -= n;
                const uint32_t row1 = perm[p1], row2 = perm[p2];
                NodeIn in1, in2;
                load_node(A.soa, A.tg, row1, in1);
                load_node(A.soa, A.tg, row2, in2);
                const uint32_t dk1 = ov_count(ov, row1), dk2 = ov_count(ov, row2);
                NodeEval e1, e2;
                e1.score = 0.0;
                e2.score = 0.0;
                eval_loaded<false, false>(A.soa, A.tg, class_ok, A.ask, dk1, A.penalty_bits, A.log10, nullptr, row1,
                                          in1, &e1);
                eval_loaded<false, false>(A.soa, A.tg, class_ok, A.ask, dk2, A.penalty_bits, A.log10, nullptr, row2,
                                          in2, &e2);
                if (need) {
                    st = e1.status;
                    sc = e1.score;
                    if (s1) { st1 = st; sc1 = sc; rw1 = row1; } else { st0 = st; sc0 = sc; rw0 = row1; }
                }
                if (need2) {
                    if (s1) { st0 = e2.status; sc0 = e2.score; rw0 = row2; }
                    else { st1 = e2.status; sc1 = e2.score; rw1 = row2; }
                }
                have = min(64u * (k + 2) - skew, n);
            }

            const bool is_opt = valid && st == kOption;
            const bool is_np = is_opt && sc <= 0.0;
            uint32_t np_tot;
            const uint32_t np_before = a + block_prefix<64>(is_np, nullptr, &np_tot);
            const bool aside = is_np && np_before < (uint32_t)kMaxSkip;
            const bool ret = is_opt && !aside;
            uint32_t ret_tot;
            const uint32_t ret_before = r + block_prefix<64>(ret, nullptr, &ret_tot);
            const uint64_t sm = __ballot(ret && ret_before == A.limit - 1u);
            const int stop_lane = sm ? (int)__ffsll((long long)sm) - 1 : 64;
            const bool pulled = valid && lane <= stop_lane;
            if (aside && pulled) {
                aside_score[np_before] = sc;
                aside_pos[np_before] = j;
            }
            if (ret && ret_before < A.limit && sc > lbest_s) { lbest_s = sc; lbest_p = j; }
            n_filtered += (uint32_t)__popcll(__ballot(pulled && st == kFiltered));
            n_exhausted += (uint32_t)__popcll(__ballot(pulled && st == kExhausted));
            a += (uint32_t)__popcll(__ballot(aside && pulled));
            if (sm) {
                consumed = 64u * k + (uint32_t)stop_lane - skew + 1u;
                r = A.limit;
                stopped = true;
                break;
            }
            r += ret_tot;
        }
        {
            double cs;
            int cp;
            block_argmax<64>(lbest_p >= 0, lbest_s, lbest_p, nullptr, nullptr, &cs, &cp);
            if (cp != 0x7FFFFFFF) { best_score = cs; best_pos = cp; }
        }
        wave_sync();   // the set-aside options in LDS
        if (!stopped) {
            const uint32_t take = min(a, A.limit - r);
            for (uint32_t i = 0; i < take; i++) {
                if (aside_score[i] > best_score) { best_score = aside_score[i]; best_pos = aside_pos[i]; }
            }
        }
        int win_row = -1;
        if (best_pos >= 0) {
            uint32_t pos = offset + (uint32_t)best_pos;
            if (pos >= n) pos -= n;
            win_row = (int)perm[pos];
        }
        uint32_t no = offset + (consumed % n);
        if (no >= n) no -= n;
        if (lane == 0) {
            emit_placement<false>(A, class_ok, ov, nullptr, 0u, it, win_row, best_score, consumed, n_filtered,
                                  n_exhausted, no);
            if (win_row >= 0) ov_add(ov, (uint32_t)win_row);
            else if (s_flags) ds_stop(A, D, s_slot, s_row, s_flags, -1);   // PopUpdate(allocs[it])
        }
        wave_sync();
        offset = no;
        // slide the cache (as k_window: a full pass restarts the ring)
        if (stopped) {
            rb = (rb + consumed) & 127u;
            have = have > consumed ? have - consumed : 0u;
        } else {
            have = 0;
        }
        if (win_row < 0) break;
        have = ds_cut((uint32_t)win_row, rb, have, rw0, rw1, lane);
        placed++;
    }
    if (lane == 0) {
        A.eval_status[0] = placed;
        A.eval_status[1] = offset;
        A.eval_status[2] = guard;
    }
    ds_publish();   // the last stop (or its undo) before every lane's write-back
    if (A.writeback) writeback_overlay<64, false, false>(A, ov, H, nullptr);
}

// ---- pe_place_destructive_full: the same loop for a group that runs full passes --
// k_fullpass_lds's shape (one workgroup, one build pass over the list, one LDS
// entry per option, the approximate and the exact pass per Select, the exact
// skip rule when no option is positive, the winner evaluated at dk = 0 and with
// the placement added, the commit straight to the SoA) with k_destructive's
// stop before every Select. What the stops add:
// - A stop can turn an exhausted node, or one that distinct_hosts filtered, into
//   an option: the build gives an entry to every option and to every list
//   position the stop list names (one bit per position from the host), whatever
//   its status. After the stop the thread that holds the row's entry evaluates
//   the row again from HBM at dk = 0 and moves the block's filtered and
//   exhausted counters with the status. The launch's placements are in HBM
//   already, so there is nothing to fold.
// - The spread counts under stops (DESIGN.md §38's closed form): per set and
//   value the group's existing and plan allocs with this launch's winners (ep),
//   NodeUpdate's allocs that pass cleared_counts' test with this launch's stops
//   (craw), and whether a plan alloc of the group has the value (prop). The
//   count a Select sees is ep less the cleared count, not below zero, where one
//   cleared alloc is forgiven when prop is set and more than one is cleared
//   (propertyset.go:199-208). One thread advances them between Selects; a
//   target set refreshes the one boost whose count moved, an even set rebuilds
//   its table.
// - A nil Select: the same lane takes the stop back, spread columns first, and
//   the loop ends.
// Every loop is bounded without the data: updates by count, entries by kDfCap.
// A slot, row or position of the stop list out of range raises state[2] and
// ends the call before anything is indexed with it. More entries than kDfCap:
// state[5] = 1 before the first stop is applied.
constexpr int kDfPer = 8;                               // entries per thread
constexpr uint32_t kDfCap = kFullThreads * kDfPer;      // LDS entries (16 B each)

// GetCombinedUseMap of one value: existing + proposed - cleared, not below 0
__device__ __forceinline__ uint32_t df_count(uint32_t ep, uint32_t craw, uint32_t prop) {
    const uint32_t cleared = craw - ((prop && craw > 1u) ? 1u : 0u);
    return ep >= cleared ? ep - cleared : 0u;
}

// Workgroup-wide ordering point for HBM stores of one thread that others load next.
__device__ __forceinline__ void df_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// kMetrics (pe_place_destructive_full_metrics): update k's Select's use counts,
// counts[] after its stop and before its winner's placement (a nil Select's
// before its undo), go to cnt_log[k * pset_cnt_total + i] in device memory:
// what k_spread_tables<true> builds record k's boosts from for the trace of its
// maps, so the closed form above stays in this kernel alone. The launcher checks
// that the log holds count * pset_cnt_total words.
template <int NP, bool kMetrics>   // spread properties scored, at most kAuxPsets
__global__ void __launch_bounds__(kFullThreads) k_destructive_full(const SweepArgs* __restrict__ Ap,
                                                                   DestructiveFullArgs F, const uint32_t* visit,
                                                                   uint32_t n, uint32_t count, pe_ranked_node* out,
                                                                   uint32_t* state, uint32_t* cnt_log) {
    const SweepArgs& A = *Ap;
    extern __shared__ double ent_sum[];                                   // [kDfCap] score_head sums
    uint32_t* ent_meta = reinterpret_cast<uint32_t*>(ent_sum + kDfCap);    // status | k << 2 | spread values
    uint32_t* ent_pos = ent_meta + kDfCap;                                 // visit position
    __shared__ double tab[kAuxPsets * (kAuxValues + 1)];
    __shared__ double desired[kAuxPsets * kAuxValues];
    __shared__ uint32_t counts[kAuxPsets * kAuxValues];     // what each Select's table is built from
    __shared__ uint32_t sp_ep[kAuxPsets * kAuxValues];      // EP0 + ks
    __shared__ uint32_t sp_craw[kAuxPsets * kAuxValues];    // Craw0 + kc (+ the staged stop)
    __shared__ uint32_t sp_prop[kAuxPsets * kAuxValues];    // prop0 || ks > 0
    __shared__ double aff_lds[kAuxValues];
    __shared__ double red_s[kFullWaves];
    __shared__ uint32_t red_r[kFullWaves];
    __shared__ uint32_t red_f[kFullWaves], red_e[kFullWaves];
    __shared__ SweepRec red[kFullWaves];
    __shared__ uint32_t scratch[4];
    __shared__ uint32_t sh_nf, sh_ne, sh_stop, sh_win, sh_m;
    __shared__ uint32_t sh_meta;   // the winner's new entry meta (sh_win stays the skip rule's rank: waves read it late)
    __shared__ double parts1[PE_MAX_SCORES];   // lane 1's parts (unused)
    __shared__ double rcp_k[8];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const TgTables& t = A.tg;
    constexpr int np = NP;
    const uint32_t off = A.offset;
    bool any_even = false;
    for (int p = 0; p < np; p++) any_even = any_even || t.pset_even[p];
    for (int i = tid; i < kAuxValues; i += kFullThreads) aff_lds[i] = A.aff_vals[i];
    if (tid < 8) rcp_k[tid] = tid ? 1.0 / (double)tid : 0.0;
    if (tid == 0) sh_m = 0;
    for (int p = 0; p < np; p++)
        for (int v = tid; v < t.pset_nvals[p]; v += kFullThreads) {
            const uint32_t i = t.pset_cnt_off[p] + (uint32_t)v;
            sp_ep[i] = F.sp[i];
            sp_craw[i] = F.sp[t.pset_cnt_total + i];
            sp_prop[i] = F.sp[2u * t.pset_cnt_total + i];
            counts[i] = df_count(sp_ep[i], sp_craw[i], sp_prop[i]);
            desired[i] = t.pset_even[p] ? 0.0 : t.pset_desired[p][v];
        }
    __syncthreads();
    if (np) build_spread_table<kFullThreads>(t, counts, tab, scratch);
    auto spread_of = [&](uint32_t meta) __attribute__((always_inline)) -> double {   // lookup_scores' total
        double sp = 0.0;
#pragma unroll
        for (int p = 0; p < np; p++) {
            const uint32_t v = (meta >> (8 + 8 * p)) & 255u;
            sp += (v == kAuxMissing) ? -1.0 : tab[t.pset_tab_off[p] + v];
        }
        return sp;
    };
    auto load = [&](uint32_t row, NodeIn& in) __attribute__((always_inline)) -> uint32_t {   // the sweep's AUX fetch
        in.r = A.soa.rec[row];
        in.coll_tg = t.coll_tg[row];
        in.dev_free = t.dev_free ? t.dev_free[row] : 0u;
        const uint32_t aux = A.node_aux[row];
        in.feas = aux >> 31;
        return aux;
    };
    // status and score_head of a loaded node with dk placements added; with a
    // `parts` pointer the parts are written there
    auto head = [&](uint32_t row, const NodeIn& in, uint32_t aux, uint32_t dk, double* parts, double* sum,
                    uint32_t* kk) __attribute__((always_inline)) -> int {
        ScoreIn si;
        const int st = status_loaded(A.soa, t, t.class_ok, A.ask, dk, row, in, &si);
        *kk = 0;
        *sum = 0.0;
        if (st == kOption) {
            si.penalty = A.penalty_bits ? (A.penalty_bits[row >> 5] >> (row & 31)) & 1u : 0u;
            si.aff = aff_lds[aux & 255u];
            si.spread = 0.0;
            *sum = parts ? score_head<true>(A.ask, A.log10, si, parts, *kk)
                         : score_head<false>(A.ask, A.log10, si, nullptr, *kk);
        }
        return st;
    };
    // the final score of an entry (score_option's tail)
    auto final_sum = [&](uint32_t e, uint32_t* kk_out) __attribute__((always_inline)) -> double {
        const uint32_t meta = ent_meta[e];
        double sum = ent_sum[e];
        const double sp = spread_of(meta);
        uint32_t kk = (meta >> 2) & 7u;
        if (sp != 0.0) { sum += sp; kk++; }
        *kk_out = kk;
        return sum;
    };
    // one value's count after its columns moved, and a target set's boost of it
    // (build_spread_table's arithmetic; an even set rebuilds its table)
    auto refresh = [&](int p, uint32_t v) __attribute__((always_inline)) {
        const uint32_t i = t.pset_cnt_off[p] + v;
        const uint32_t c = df_count(sp_ep[i], sp_craw[i], sp_prop[i]);
        counts[i] = c;
        if (!t.pset_even[p]) {
            const double d = desired[i];
            tab[t.pset_tab_off[p] + v] = d != d ? -1.0 : ((d - (double)(c + 1u)) / d) * t.pset_weight_frac[p];
        }
    };
    uint32_t nf = 0, ne = 0;
    for (uint32_t pos = tid; pos < n; pos += kFullThreads) {
        const uint32_t row = visit[pos];
        NodeIn in;
        const uint32_t aux = load(row, in);
        double s;
        uint32_t kk;
        const int st = head(row, in, aux, 0u, nullptr, &s, &kk);
        nf += st == kFiltered;
        ne += st == kExhausted;
        const bool named = (F.named[pos >> 5] >> (pos & 31u)) & 1u;   // a stop of the list can bring it back
        if (st == kOption || named) {
            const uint32_t e = atomicAdd(&sh_m, 1u);
            if (e < kDfCap) {
                ent_sum[e] = s;
                ent_meta[e] = (uint32_t)st | (kk << 2) | (aux & 0x00FFFF00u);
                ent_pos[e] = pos;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        nf += (uint32_t)__shfl_xor((int)nf, o);
        ne += (uint32_t)__shfl_xor((int)ne, o);
    }
    if (lane == 0) { red_f[wid] = nf; red_e[wid] = ne; }
    __syncthreads();
    const uint32_t m = sh_m;
    if (m > kDfCap) {   // uniform: no stop applied yet, the caller's per-call sequence answers
        if (tid == 0) state[5] = 1;
        return;
    }
    if (tid == 0) {
        uint32_t a = 0, b = 0;
        for (int w = 0; w < kFullWaves; w++) { a += red_f[w]; b += red_e[w]; }
        sh_nf = a;
        sh_ne = b;
        sh_stop = 0;
    }
    __syncthreads();
    auto rank_of_pos = [&](uint32_t pos) __attribute__((always_inline)) -> uint32_t {
        return pos >= off ? pos - off : pos + n - off;
    };
    uint32_t placed = 0, guard = 0, nil = 0;
    // the next update's stop words are loaded one Select ahead (the list is in mapped host memory)
    uint32_t nx[kDfWords] = {0, 0, 0, 0};
    if (count)
        for (uint32_t w = 0; w < kDfWords; w++) nx[w] = F.d.stops[w];
    for (uint32_t it = 0; it < count; it++) {
        // ---- AppendStoppedAlloc(allocs[it]) ----
        const uint32_t s_slot = nx[0], s_row = nx[1], s_flags = nx[2], s_pos = nx[3];
        if (it + 1 < count)
            for (uint32_t w = 0; w < kDfWords; w++) nx[w] = F.d.stops[kDfWords * (it + 1) + w];
        uint32_t s_aux = 0;
        if (s_flags) {
            if (s_row >= A.soa.n || ((s_flags & kDsLive) && s_slot >= F.d.n_slots) || (s_pos != PE_NONE && s_pos >= n)) {
                guard = 1u;   // uniform
                break;
            }
            s_aux = A.node_aux[s_row];
            if (tid == 0) {
                ds_stop(A, F.d, s_slot, s_row, s_flags, +1);
                if (s_flags & kDsOwn) {
#pragma unroll
                    for (int p = 0; p < np; p++) {
                        const uint32_t v = (s_aux >> (8 + 8 * p)) & 255u;
                        if (v == kAuxMissing || v >= (uint32_t)t.pset_nvals[p]) continue;
                        sp_craw[t.pset_cnt_off[p] + v]++;
                        refresh(p, v);
                    }
                }
            }
            df_sync();
            if (s_pos != PE_NONE && (s_flags & (kDsLive | kDsJob | kDsTg))) {   // the row's entry from HBM, dk = 0
#pragma unroll
                for (int j = 0; j < kDfPer; j++) {
                    const uint32_t e = (uint32_t)tid + (uint32_t)j * kFullThreads;
                    if (e < m && ent_pos[e] == s_pos) {
                        const uint32_t row = visit[s_pos];
                        NodeIn in;
                        const uint32_t aux = load(row, in);
                        double s;
                        uint32_t kk;
                        const int st = head(row, in, aux, 0u, nullptr, &s, &kk);
                        const int was = (int)(ent_meta[e] & 3u);
                        ent_sum[e] = s;
                        ent_meta[e] = (uint32_t)st | (kk << 2) | (aux & 0x00FFFF00u);
                        sh_nf += (uint32_t)(st == kFiltered) - (uint32_t)(was == kFiltered);   // one entry per position
                        sh_ne += (uint32_t)(st == kExhausted) - (uint32_t)(was == kExhausted);
                    }
                }
            }
            if (any_even && (s_flags & kDsOwn)) build_spread_table<kFullThreads>(t, counts, tab, scratch);
            __syncthreads();
        }

        // ---- Select: k_fullpass_lds's passes ----
        if constexpr (kMetrics && NP > 0) {   // this Select's use counts (they move behind the next barrier only)
            const uint32_t nc = t.pset_cnt_total;
            for (uint32_t i = (uint32_t)tid; i < nc; i += kFullThreads) cnt_log[(size_t)it * nc + i] = counts[i];
        }
        double ap[kDfPer];
        double amax = -__builtin_inff();
#pragma unroll
        for (int j = 0; j < kDfPer; j++) {
            const uint32_t e = (uint32_t)tid + (uint32_t)j * kFullThreads;
            ap[j] = -__builtin_inff();
            if (e < m) {
                uint32_t kk;
                const double sum = final_sum(e, &kk);
                if ((ent_meta[e] & 3u) == (uint32_t)kOption) ap[j] = sum * rcp_k[kk];
            }
            amax = ap[j] > amax ? ap[j] : amax;
        }
        amax = __ockl_wfred_max_f64(amax);
        const double cut = amax - (__builtin_fabs(amax) * 0x1p-48 + 0x1p-1000);
        double best = -__builtin_inff();
        uint32_t best_rank = 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < kDfPer; j++) {
            const bool near = ap[j] >= cut && ap[j] != -__builtin_inff();   // options only
            if (__ballot(near)) {
                if (near) {
                    const uint32_t e = (uint32_t)tid + (uint32_t)j * kFullThreads;
                    uint32_t kk;
                    const double sc = final_sum(e, &kk) / (double)kk;
                    const uint32_t rk = rank_of_pos(ent_pos[e]);
                    if (sc > best || (sc == best && rk < best_rank)) { best = sc; best_rank = rk; }
                }
            }
        }
        {   // the wave's (max, earliest rank) over its few candidate lanes
            uint64_t cand = __ballot(best_rank != 0xFFFFFFFFu);
            double wb = -__builtin_inff();
            uint32_t wr = 0xFFFFFFFFu;
            for (int q = 0; q < 64 && cand; q++) {
                const int l = __builtin_ctzll(cand);
                cand &= cand - 1;
                const double b = readlane_f64(best, l);
                const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)best_rank, l);
                if (b > wb || (b == wb && r < wr)) { wb = b; wr = r; }
            }
            best = wb;
            best_rank = wr;
        }
        if (lane == 0) { red_s[wid] = best; red_r[wid] = best_rank; }
        const uint32_t my_rank = best_rank;   // wave-uniform
        uint32_t c_row = 0;
        if (lane < 2 && my_rank != 0xFFFFFFFFu) {
            uint32_t pos = off + my_rank;
            if (pos >= n) pos -= n;
            c_row = visit[pos];
        }
        __syncthreads();
        // every wave resolves the block's winner itself: the maximum score,
        // then the earliest rank among the waves holding it
        best = lane < kFullWaves ? red_s[lane] : -__builtin_inff();
        best_rank = lane < kFullWaves ? red_r[lane] : 0xFFFFFFFFu;
        best = __ockl_wfred_max_f64(best);
        uint32_t win = __ockl_wfred_min_u32(lane < kFullWaves && red_s[lane] == best ? best_rank : 0xFFFFFFFFu);
        if (win != 0xFFFFFFFFu && !(best > 0.0)) {   // every option non-positive: the skip rule decides
            SweepRec r;
            rec_init(r);
            for (uint32_t e = tid; e < m; e += kFullThreads) {
                if ((ent_meta[e] & 3u) != (uint32_t)kOption) continue;
                uint32_t kk;
                const double sum = final_sum(e, &kk);
                rec_add(r, rank_of_pos(ent_pos[e]), sum / (double)kk);
            }
            rec_block_reduce<kFullThreads>(r, red);
            if (tid == 0) sh_win = rec_winner(r);
            __syncthreads();
            win = sh_win;
        }
        pe_ranked_node* o = out + it;
        // the wave whose candidate won evaluates it; when the skip rule picked
        // a rank no wave held, wave 0 loads it
        bool mine = win != 0xFFFFFFFFu && my_rank == win;
        if (win != 0xFFFFFFFFu && wid == 0 &&
            __ballot(lane < kFullWaves && red_r[lane] == win) == 0) {   // wave-uniform
            mine = true;
            if (lane < 2) {
                uint32_t pos = off + win;
                if (pos >= n) pos -= n;
                c_row = visit[pos];
            }
        }
        if (wid == 0 && win == 0xFFFFFFFFu) {
            if (lane == 0) {   // the nil Select: its record, then PopUpdate(allocs[it]) in reverse order
                o->row = -1;
                o->nodes_evaluated = n;            // a full pass pulls every node
                o->nodes_filtered = sh_nf;
                o->nodes_exhausted = sh_ne;
                o->new_offset = off;
                if (s_flags) {
                    if (s_flags & kDsOwn) {
#pragma unroll
                        for (int p = np - 1; p >= 0; p--) {
                            const uint32_t v = (s_aux >> (8 + 8 * p)) & 255u;
                            if (v == kAuxMissing || v >= (uint32_t)t.pset_nvals[p]) continue;
                            sp_craw[t.pset_cnt_off[p] + v]--;
                        }
                    }
                    ds_stop(A, F.d, s_slot, s_row, s_flags, -1);
                }
                sh_stop = 1;
            }
        } else if (mine && lane < 2) {
            const uint32_t row = c_row;
            NodeIn in;
            const uint32_t aux = load(row, in);
            double s;
            uint32_t kk;
            const int st = head(row, in, aux, (uint32_t)lane, lane == 0 ? o->scores : parts1, &s, &kk);
            const int st1 = __shfl(st, 1);
            const uint32_t meta0 = (aux & 0x00FFFF00u);   // spread values: the entry's
            if (lane == 1) {
                sh_meta = (uint32_t)st | (kk << 2) | meta0;
                parts1[0] = s;
            } else {           // the placement's record, then the commit
                const double sp = spread_of(meta0);
                if (sp != 0.0) {   // SpreadIterator (spread.go:110-174)
                    s += sp;
                    o->scores[kk] = sp;
                    kk++;
                }
                o->row = (int32_t)row;
                o->final_score = s / (double)kk;   // ScoreNormalizationIterator (rank.go:762-767)
                o->n_scores = kk;
                o->nodes_evaluated = n;            // a full pass pulls every node
                o->nodes_filtered = sh_nf;
                o->nodes_exhausted = sh_ne;
                o->new_offset = off;               // and leaves the cursor where it is
                record_offers(A.soa, A.ask, t, row, 0u, o);
                uint32_t offers = 0xFFFFFFFFu;
                if (o->n_device_offers) {
                    offers = 0;
                    for (uint32_t q = 0; q < o->n_device_offers && q < 4; q++)
                        offers |= (o->device_offer_group[q] & 255u) << (8 * q);
                }
                if (A.ask.n_dev == 0 && A.ask.cores == 0) {   // commit_row from the loaded values: stores only
                    NodeRec& r = A.soa.rec[row];
                    r.used_cpu = in.r.used_cpu + A.ask.cpu;
                    r.used_mem = in.r.used_mem + A.ask.mem;
                    r.used_disk = in.r.used_disk + A.ask.disk;
                    r.used_mbits = in.r.used_mbits + A.ask.commit_mbits;
                    r.used_dyn = in.r.used_dyn + A.ask.commit_dyn;
                    A.soa.coll_job[row] += 1;
                    t.coll_tg[row] = in.coll_tg + 1;
                } else {
                    commit_row(A.soa, t, A.ask, row, offers);
                }
#pragma unroll
                for (int p = 0; p < np; p++) {   // the winner's value: one more proposed alloc of the group
                    const uint32_t v = (meta0 >> (8 + 8 * p)) & 255u;
                    if (v == kAuxMissing || v >= (uint32_t)t.pset_nvals[p]) continue;
                    sp_ep[t.pset_cnt_off[p] + v]++;
                    sp_prop[t.pset_cnt_off[p] + v] = 1u;
                    refresh(p, v);
                }
                sh_nf += st1 == kFiltered;
                sh_ne += st1 == kExhausted;
            }
        }
        df_sync();   // the commit (or the undo) before the next stop's or winner's loads
        if (sh_stop) {
            nil = 1u;
            break;
        }
        placed++;
        {   // the winner's entry with this placement added
            uint32_t pos = off + win;
            if (pos >= n) pos -= n;
#pragma unroll
            for (int j = 0; j < kDfPer; j++) {
                const uint32_t e = (uint32_t)tid + (uint32_t)j * kFullThreads;
                if (e < m && ent_pos[e] == pos) {
                    ent_sum[e] = parts1[0];
                    ent_meta[e] = sh_meta;
                }
            }
        }
        if (any_even) build_spread_table<kFullThreads>(t, counts, tab, scratch);
        __syncthreads();
    }
    if (tid == 0) {
        state[0] = nil;
        state[1] = placed;
        state[2] = guard;
    }
}

// inplaceUpdate's loop (util.go:743-760) over a list of snapshot allocs: per
// update AppendStoppedAlloc, a Select on the alloc's node alone, PopUpdate and,
// on an option, the updated alloc in place of the old one. Only updates on one
// node depend on each other: each lane owns one node group (distinct rows, no
// atomics), keeps the node's record in registers and walks the group's updates
// in list order. The old alloc leaves the proposed state (k_plan_stop's
// deltas), the Select is the pipeline every other path runs (status_loaded,
// score_into), an option adds the ask as k_system's commit does and keeps the
// stop, anything else puts the registers back. One record store per group.
// Two node images (current and trial) are live across the pipeline: without
// the hint the allocator takes 130 VGPRs and a fourth wave per SIMD is lost.
//
// kStop (a preempting system stack): at its first update whose
// plain fit is exhausted the group stops. That update and the later ones stay
// unwritten, the node's image goes back to HBM as at the end of the walk, the
// update's index is kept in resume[g] and the group joins the stopped list
// (one atomic per wave; the groups are independent, the list's order is free).
// own_existing drops by the own allocs updated so far: evict_eval's
// placeholders (coll_job - own_existing) stay the job's plan placements.
__device__ __forceinline__ uint32_t wave_slot(uint32_t* counter);

// kMetrics (AllocMetric on): the same walk on the same images,
// so the same outcomes and score bits. Beside them, by list position, what the
// update's Select leaves in its maps: a k_trace code for an outcome that is not
// an option (the folded FeasibilityWrapper verdict or distinct_hosts for a
// filtered node; trace_offers then trace_fit on the trial image for an
// exhausted one, which is the state that Select saw) and an option's ScoreNode
// values in k_trace's layout, from the record's own score_into call, whether or
// not records were asked for. With kStop an exhausted plain fit is not final
// and records nothing.
//
// kCsi (pe_inplace_update_csi): an update whose node passes the
// wrapper's checks and has a code in its record set's column is filtered before
// distinct_hosts and the fit (inplace_csi_code below): status 1, a nil record,
// the metrics form's code kTrCsi with the 16-bit code above it, no commit, and
// with kStop no hand-off, so the eviction walk never sees the group because of
// it. k_inplace_evict applies the same fold to the updates it re-runs.
__device__ __forceinline__ uint32_t inplace_filter_code(const TgTables& t, uint32_t row, const NodeIn& in) {
    bool ok;
    if (t.node_feas) ok = in.feas != 0;
    else {
        ok = t.class_ok[in.r.cls] != 0;
        if (t.node_ok) ok = ok && t.node_ok[row] != 0;
    }
    return ok ? kTrDistinctHosts : kTrWrapper;   // (no property sets on this path)
}

__device__ __forceinline__ uint32_t inplace_exhaust_code(const NodeSoA& s, const TgTables& t, const Ask& a, uint32_t row,
                                                         const NodeIn& in) {
    uint32_t code = trace_offers(t, a, row, in, 0u);
    if (code == kTrOption) code = trace_fit(s, a, row, in.r, 0u, false);
    return code == kTrOption ? (uint32_t)kTrMismatch : code;
}

// pe_inplace_update_csi: the update's PE_CSI_* code where the
// CSI checker is the one that fails its Select, else 0. The checker runs behind
// the wrapper's job and group checks (feasible.go:1141-1149) and reads the
// snapshot alone, so the code is a 2-byte load from the column of the update's
// record set; a node the wrapper filters keeps the wrapper's reason. kCsi is a
// template parameter of the walks and not a null test: the walks sit at a VGPR
// step, and the test alone cost the other forms 32 bytes of scratch per lane.
template <bool kCsi>
__device__ __forceinline__ uint32_t inplace_csi_code(const InplaceArgs& A, uint32_t pos, uint32_t row,
                                                     const NodeIn& in) {
    if (!kCsi) return 0u;
    const uint32_t code = A.csi_codes[(size_t)A.csi_set[pos] * A.csi_rows + row];
    if (!code) return 0u;
    return inplace_filter_code(A.tg, row, in) == kTrWrapper ? 0u : code;
}

// score_into's parts (append order) by scorer, as k_trace names them.
__device__ __forceinline__ void inplace_named(const Ask& a, const ScoreIn& si, const double* parts, double norm,
                                              double* o) {
    uint32_t k = 1;
    o[0] = parts[0];
    o[1] = a.dev_tw != 0.0 ? parts[k++] : 0.0;
    o[2] = (a.anti_aff && si.coll > 0) ? parts[k++] : 0.0;
    if (si.penalty) k++;
    o[3] = si.aff != 0.0 ? parts[k++] : 0.0;
    o[4] = si.spread != 0.0 ? parts[k++] : 0.0;
    o[5] = norm;
}

template <bool kStop, bool kMetrics, bool kCsi>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
k_inplace(InplaceArgs A, InplaceStopArgs S, InplaceMetricsArgs M) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < A.n_groups; g += stride) {
        const uint32_t b = A.group_off[g], e = A.group_off[g + 1];
        if (b >= e) continue;
        const uint32_t row = A.upd[b].row;
        NodeIn in;
        load_node(A.soa, A.tg, row, in);
        if (A.dev_free) in.dev_free = A.dev_free[row];
        uint32_t cj = A.soa.coll_job[row];
        bool dirty = false;
        uint32_t own_drop = 0;
        for (uint32_t u = b; u < e; u++) {
            const InplaceUpd x = A.upd[u];
            NodeIn t = in;
            uint32_t tj = cj;
            if (x.slot != PE_NONE) {   // the old alloc leaves ProposedAllocs
                const PreemptAlloc& p = A.allocs[x.slot];
                t.r.used_cpu -= p.cpu;
                t.r.used_mem -= p.mem;
                t.r.used_disk -= p.disk;
                t.r.used_mbits -= p.mbits;
                t.r.used_dyn -= p.dyn;
                for (int k = 0; k < 4 && k < (int)p.n_dev; k++) t.dev_free += byte_of(p.dev_c, k) << (8 * byte_of(p.dev_g, k));
            }
            if (x.flags & kInplaceOwnJob) tj -= 1u;
            if (x.flags & kInplaceOwnTg) t.coll_tg -= 1u;
            if (tj != cj) A.soa.coll_job[row] = tj;   // DistinctHostsIterator reads the column
            ScoreIn si;
            int st = status_loaded<false>(A.soa, A.tg, A.tg.class_ok, A.ask, 0u, row, t, &si);
            const uint32_t csi = inplace_csi_code<kCsi>(A, x.pos, row, t);
            if (csi) st = kFiltered;   // unavailable: no fit is tried, nothing is handed to the eviction walk
            if (kStop && st == kExhausted) {   // the eviction walk takes the group from here
                if (tj != cj) A.soa.coll_job[row] = cj;
                S.resume[g] = u;
                S.stopped[wave_slot(S.n_stopped)] = g;
                if (own_drop) S.own_existing[row] -= own_drop;
                break;
            }
            A.status[x.pos] = (uint8_t)st;
            if (A.out) {
                EmitRec& o = A.out[x.pos];
                o.row = st == kOption ? (int32_t)row : -1;
                o.n_scores = 0;
                o.final_score = 0.0;
                for (int k = 0; k < PE_MAX_SCORES; k++) o.scores[k] = 0.0;
                o.nodes_evaluated = 1;
                o.nodes_filtered = st == kFiltered;
                o.nodes_exhausted = st == kExhausted;
                o.new_offset = 0;   // a one-node list: the cursor wraps to its start
                o.n_device_offers = 0;
                for (int q = 0; q < kMaxDevReq; q++) o.device_offer_group[q] = 0;
                o.flags = 0;
            }
            if (kMetrics)
                M.code[x.pos] = st == kOption ? (uint32_t)kTrOption
                                : csi        ? (uint32_t)kTrCsi | csi << 8
                                : (st == kFiltered ? inplace_filter_code(A.tg, row, t)
                                                   : inplace_exhaust_code(A.soa, A.tg, A.ask, row, t));
            if (st != kOption) {
                if (tj != cj) A.soa.coll_job[row] = cj;
                continue;
            }
            if (kMetrics) {
                lookup_scores(A.tg, nullptr, nullptr, row, t.r.cls, &si);
                double parts[PE_MAX_SCORES];
                for (int k = 0; k < PE_MAX_SCORES; k++) parts[k] = 0.0;
                uint32_t ns;
                const double fs = score_into<true>(A.ask, A.log10, si, parts, &ns);
                inplace_named(A.ask, si, parts, fs, M.named + (size_t)x.pos * kInplaceNamed);
                if (A.out) {
                    EmitRec& o = A.out[x.pos];
                    o.final_score = fs;
                    o.n_scores = ns;
                    for (int k = 0; k < PE_MAX_SCORES; k++) o.scores[k] = parts[k];
                }
            } else if (A.out) {
                EmitRec& o = A.out[x.pos];
                lookup_scores(A.tg, nullptr, nullptr, row, t.r.cls, &si);
                uint32_t ns;
                o.final_score = score_into<true>(A.ask, A.log10, si, o.scores, &ns);
                o.n_scores = ns;
            }
            if (A.ask.n_dev > 0) {   // the Select's offers, then consumed by the commit
                const DevClass& dc = A.tg.dev_cls[t.r.cls];
                uint32_t groups[kMaxDevReq];
                double m;
                uint32_t fr = t.dev_free;
                if (dev_assign(A.ask, dc, fr, &m, groups)) {
                    t.dev_free = fr;
                    if (A.out) {
                        EmitRec& o = A.out[x.pos];
                        o.n_device_offers = (uint32_t)A.ask.n_dev;
                        for (int q = 0; q < kMaxDevReq; q++)
                            if (q < A.ask.n_dev) o.device_offer_group[q] = (uint16_t)groups[q];
                    }
                }
            }
            // Plan.AppendAlloc of the updated alloc; the stop stays
            t.r.used_cpu += A.ask.cpu;
            t.r.used_mem += A.ask.mem;
            t.r.used_disk += A.ask.disk;
            t.r.used_mbits += A.ask.commit_mbits;
            t.r.used_dyn += A.ask.commit_dyn;
            t.coll_tg += 1u;
            cj = tj + 1u;
            A.soa.coll_job[row] = cj;
            in = t;
            dirty = true;
            if (kStop && (x.flags & kInplaceOwnJob)) own_drop++;
            if (x.slot != PE_NONE) {
                A.preempted[x.slot] = 2;
                if (A.soa.core_used && A.palloc_cores)   // its reserved cores leave the node's used set
                    for (int w = 0; w < 4; w++) A.soa.core_used[4 * row + w] &= ~A.palloc_cores[4 * (size_t)x.slot + w];
            }
        }
        if (!dirty) continue;
        NodeRec& r = A.soa.rec[row];
        r.used_cpu = in.r.used_cpu;
        r.used_mem = in.r.used_mem;
        r.used_disk = in.r.used_disk;
        r.used_mbits = in.r.used_mbits;
        r.used_dyn = in.r.used_dyn;
        A.tg.coll_tg[row] = in.coll_tg;
        if (A.dev_free) A.dev_free[row] = in.dev_free;
    }
}

// ---- system jobs with several task groups in one pass ---

// A distinct slot of `counter` for every active lane: one atomic per wave.
__device__ __forceinline__ uint32_t wave_slot(uint32_t* counter) {
    const uint64_t m = __ballot(1);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)m) - 1u;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = __shfl(base, (int)leader);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// The words of a node's image that an in-place update changes, back to HBM.
__device__ __forceinline__ void inplace_store(const InplaceArgs& A, uint32_t row, const NodeIn& in) {
    NodeRec& r = A.soa.rec[row];
    r.used_cpu = in.r.used_cpu;
    r.used_mem = in.r.used_mem;
    r.used_disk = in.r.used_disk;
    r.used_mbits = in.r.used_mbits;
    r.used_dyn = in.r.used_dyn;
    A.tg.coll_tg[row] = in.coll_tg;
}

// The eviction walk of pe_inplace_update_preempt over the node
// groups k_inplace<true> stopped, one lane per group from its resume index, at
// eviction width W. Per update the plain Select as k_inplace runs it; where
// it is exhausted, BinPack with evict (evict_eval). evict_eval reads HBM, so
// the trial goes there first: the node's record without the old alloc, the
// stop in `preempted`, coll_job, the group's coll_tg and own_existing. On an
// option the record takes the eviction's score parts (as k_evict_record), the
// preempted set goes to the append buffer as [list position, W mask words],
// and the ask is added as k_inplace does: inplaceUpdate never reads
// PreemptedAllocs (util.go:759-802), so the evicted allocs stay in the
// proposed state and nothing joins the plan's preemptions. Otherwise every
// word the trial wrote is put back. HBM holds the group's current image
// whenever evict_eval runs or the lane leaves. A node beyond the width
// commits nothing from that update on: the group keeps its resume index,
// joins the wider list and raises kEvictWider.
//
// kMetrics: the plain step's codes and named scores as
// k_inplace's metrics form writes them; evict_eval also returns an option's
// ScoreNode values and the dimension of an update that stays exhausted (0: it
// gave the node up without ExhaustedNode). All by list position, so a relaunch
// at a wider width rewrites the same words.
template <int W, bool kMetrics, bool kCsi>
__global__ void __launch_bounds__(256) k_inplace_evict(InplaceEvictArgs V, InplaceMetricsArgs M) {
    const InplaceArgs& A = V.I;
    const uint32_t n = *V.n_stopped;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        const uint32_t g = V.stopped[j];
        const uint32_t e = A.group_off[g + 1];
        uint32_t u = V.resume[g];
        if (u >= e) continue;
        const uint32_t row = A.upd[u].row;
        NodeIn in;
        load_node(A.soa, A.tg, row, in);
        if (A.dev_free) in.dev_free = A.dev_free[row];
        uint32_t cj = A.soa.coll_job[row];
        uint32_t oe = V.own_existing[row];
        EvictWs<W> ws;
        for (; u < e; u++) {
            const InplaceUpd x = A.upd[u];
            NodeIn t = in;
            uint32_t tj = cj, toe = oe;
            if (x.slot != PE_NONE) {   // the old alloc leaves ProposedAllocs
                const PreemptAlloc& p = A.allocs[x.slot];
                t.r.used_cpu -= p.cpu;
                t.r.used_mem -= p.mem;
                t.r.used_disk -= p.disk;
                t.r.used_mbits -= p.mbits;
                t.r.used_dyn -= p.dyn;
                for (int k = 0; k < 4 && k < (int)p.n_dev; k++) t.dev_free += byte_of(p.dev_c, k) << (8 * byte_of(p.dev_g, k));
            }
            if (x.flags & kInplaceOwnJob) {
                tj -= 1u;
                toe -= 1u;
            }
            if (x.flags & kInplaceOwnTg) t.coll_tg -= 1u;
            if (tj != cj) A.soa.coll_job[row] = tj;   // DistinctHostsIterator reads the column
            ScoreIn si;
            int st = status_loaded<false>(A.soa, A.tg, A.tg.class_ok, A.ask, 0u, row, t, &si);
            const uint32_t csi = inplace_csi_code<kCsi>(A, x.pos, row, t);
            if (csi) st = kFiltered;   // unavailable: no eviction is tried for this update
            double final_score = 0.0, parts[PE_MAX_SCORES];
            uint32_t ns = 0, exhausted = st == kExhausted;
            uint32_t mcode = kTrOption;   // (kMetrics)
            for (int k = 0; k < PE_MAX_SCORES; k++) parts[k] = 0.0;
            if (st == kOption) {
                lookup_scores(A.tg, nullptr, nullptr, row, t.r.cls, &si);
                final_score = score_into<true>(A.ask, A.log10, si, parts, &ns);
                if (kMetrics) inplace_named(A.ask, si, parts, final_score, M.named + (size_t)x.pos * kInplaceNamed);
            } else if (kMetrics && st == kFiltered) {
                mcode = csi ? (uint32_t)kTrCsi | csi << 8 : inplace_filter_code(A.tg, row, t);
            } else if (st == kExhausted) {
                // the trial, where evict_eval reads it
                inplace_store(A, row, t);
                if (toe != oe) V.own_existing[row] = toe;
                if (x.slot != PE_NONE) A.preempted[x.slot] = 2;
                NodeEval ev;
                AMask<W> mask = AMask<W>::zero();
                uint32_t offers = 0, unsup = 0, nflags = 0, dim = 0;
                double named[7];   // (kMetrics)
                const int es = evict_eval<true, false, W>(V.P, row, &ev, &mask, &offers, &unsup, &ws,
                                                          kMetrics ? named : nullptr, kMetrics ? &nflags : nullptr,
                                                          kMetrics ? &dim : nullptr);
                if (kMetrics && !unsup) {
                    mcode = es == kExhausted ? dim : (uint32_t)kTrOption;   // (a skipped eviction Select: no key)
                    if (es == kOption) {
                        double* o = M.named + (size_t)x.pos * kInplaceNamed;
                        for (int k = 0; k < 5; k++) o[k] = named[k];
                        o[5] = named[6];
                    }
                }
                if (unsup || es != kOption) {   // every word the trial wrote
                    inplace_store(A, row, in);
                    if (toe != oe) V.own_existing[row] = oe;
                    if (x.slot != PE_NONE) A.preempted[x.slot] = 0;
                }
                if (unsup) {
                    atomicOr(V.flags, unsup);
                    if (unsup == kEvictWider) {
                        V.resume[g] = u;
                        V.wider[wave_slot(V.n_wider)] = g;
                    }
                    if (tj != cj) A.soa.coll_job[row] = cj;
                    break;   // nothing more for this group in this launch
                }
                exhausted = es == kExhausted;   // (a skipped eviction Select counts nowhere)
                if (es == kOption) {
                    st = kOption;
                    final_score = ev.score;
                    ns = ev.nscores;
                    for (int k = 0; k < PE_MAX_SCORES; k++) parts[k] = k < (int)ev.nscores ? ev.parts[k] : 0.0;
                    const uint32_t at = wave_slot(V.n_app);
                    if (at < V.app_cap) {
                        uint32_t* rec = V.app + (size_t)at * (1u + W);
                        rec[0] = x.pos;
                        mask.store(rec + 1);
                    } else {
                        atomicOr(V.flags, kSysgOverflow);
                    }
                }
            }
            A.status[x.pos] = (uint8_t)(st == kOption ? kOption : (st == kFiltered ? kFiltered : kExhausted));
            if (kMetrics) M.code[x.pos] = mcode;
            if (A.out) {
                EmitRec& o = A.out[x.pos];
                o.row = st == kOption ? (int32_t)row : -1;
                o.n_scores = ns;
                o.final_score = final_score;
                for (int k = 0; k < PE_MAX_SCORES; k++) o.scores[k] = parts[k];
                o.nodes_evaluated = 1;
                o.nodes_filtered = st == kFiltered;
                o.nodes_exhausted = st == kOption ? 0u : exhausted;
                o.new_offset = 0;   // a one-node list: the cursor wraps to its start
                o.n_device_offers = 0;
                for (int q = 0; q < kMaxDevReq; q++) o.device_offer_group[q] = 0;
                o.flags = 0;
            }
            if (st != kOption) {
                if (tj != cj) A.soa.coll_job[row] = cj;
                continue;
            }
            // Plan.AppendAlloc of the updated alloc; the stop stays
            t.r.used_cpu += A.ask.cpu;
            t.r.used_mem += A.ask.mem;
            t.r.used_disk += A.ask.disk;
            t.r.used_mbits += A.ask.commit_mbits;
            t.r.used_dyn += A.ask.commit_dyn;
            t.coll_tg += 1u;
            cj = tj + 1u;
            A.soa.coll_job[row] = cj;
            oe = toe;
            V.own_existing[row] = oe;
            in = t;
            inplace_store(A, row, in);
            if (A.dev_free) A.dev_free[row] = in.dev_free;
            if (x.slot != PE_NONE) {
                A.preempted[x.slot] = 2;
                if (A.soa.core_used && A.palloc_cores)   // its reserved cores leave the node's used set
                    for (int w = 0; w < 4; w++) A.soa.core_used[4 * row + w] &= ~A.palloc_cores[4 * (size_t)x.slot + w];
            }
        }
    }
}

// ---- pe_inplace_update_spread ---------------------------------
// SpreadIterator never filters (spread.go:110-174), so the walk's statuses do
// not depend on the spread sets: k_inplace runs without them and the kernels
// below add the allocation-spread part in list order.

// GetCombinedUseMap's count of a value (propertyset.go:160-208, 250-273; what
// build_psets and cleared_counts give the Select of one update): `ks` / `kc`
// count the status-0 updates listed before it on the value (all / those whose
// old alloc NodeUpdate counts), `staged` is the update's own stop.
__device__ __forceinline__ uint32_t inplace_spread_count(uint32_t ep0, uint32_t craw0, uint32_t prop0, uint32_t ks,
                                                         uint32_t kc, bool staged) {
    const uint32_t ep = ep0 + ks;
    const uint32_t craw = craw0 + kc + (staged ? 1u : 0u);
    const uint32_t cleared = craw - (((prop0 != 0u || ks > 0u) && craw > 1u) ? 1u : 0u);
    return ep >= cleared ? ep - cleared : 0u;
}

// build_spread_table's two boosts of one value (the same operations, so the same bits).
__device__ __forceinline__ double even_boost_of(uint32_t mn, uint32_t mx, uint32_t present, uint32_t cur) {
    if (present == 0) return 0.0;
    double delta_boost;
    if (mn == 0) delta_boost = -1.0;
    else delta_boost = (double)(int)(mn - cur) / (double)mn;
    if (cur != mn) return delta_boost;
    if (mn == mx) return -1.0;
    if (mn == 0) return 1.0;
    return (double)(int)(mx - mn) / (double)mn;
}

__device__ __forceinline__ double target_boost_of(double desired, uint32_t cnt, double weight_frac) {
    if (desired != desired) return -1.0;   // no target and no implicit "*"
    const double used = (double)(cnt + 1u);
    return ((desired - used) / desired) * weight_frac;
}

// Every chunk's own (ks, kc) histogram into its zeroed row of `pre`.
__global__ void __launch_bounds__(kInplaceSpreadChunk) k_inplace_spread_hist(InplaceSpreadArgs A) {
    const uint32_t c = blockIdx.x, i = c * kInplaceSpreadChunk + threadIdx.x;
    if (c >= A.n_chunks || i >= A.n || A.status[i] != 0) return;
    const uint32_t cols = A.tg.pset_cnt_total;
    uint32_t* ks = A.pre + (size_t)c * 2 * cols;
    uint32_t* kc = ks + cols;
    const bool own = A.own[i] != 0;
    for (int p = 0; p < A.tg.n_spread; p++) {
        const uint32_t v = A.val[(size_t)p * A.n + i];
        if (v >= (uint32_t)A.tg.pset_nvals[p]) continue;   // kMissing
        atomicAdd(&ks[A.tg.pset_cnt_off[p] + v], 1u);
        if (own) atomicAdd(&kc[A.tg.pset_cnt_off[p] + v], 1u);
    }
}

// The histograms' exclusive scan over the chunks, one lane per column.
__global__ void __launch_bounds__(256) k_inplace_spread_scan(InplaceSpreadArgs A) {
    const uint32_t cols = 2 * A.tg.pset_cnt_total;
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < cols; j += gridDim.x * 256) {
        uint32_t acc = 0;
        for (uint32_t c = 0; c < A.n_chunks; c++) {
            uint32_t* w = A.pre + (size_t)c * cols + j;
            const uint32_t t = *w;
            *w = acc;
            acc += t;
        }
    }
}

// One workgroup per chunk; lane i < kInplaceSpreadChunk owns the chunk's i-th
// update and sums its sets' boosts in set order (lookup_scores' sum). A target
// set needs the update's own value only: the lane counts the chunk's earlier
// status-0 updates on it (LDS broadcast reads) on top of the chunk prefix. An
// even set needs min / max / present over all values as that Select saw them:
// the workgroup walks the chunk's updates in order on the set's columns (LDS
// while the set fits kLdsPsetValues values, else the chunk's own row of `pre`
// in HBM), one block reduction per update. Chunks own disjoint list positions:
// no atomics. The record is finished as score_into does: the parts summed left
// to right, then the spread part, then the division.
__global__ void __launch_bounds__(256) k_inplace_spread(InplaceSpreadArgs A) {
    constexpr uint32_t K = kInplaceSpreadChunk;
    __shared__ uint32_t s_val[K], s_flag[K];   // flag bit 0: status 0, bit 1: own
    __shared__ double s_boost[K];
    __shared__ uint32_t s_col[5][kLdsPsetValues];
    __shared__ uint32_t s_red[3][4];
    const uint32_t tid = threadIdx.x, c = blockIdx.x;
    if (c >= A.n_chunks) return;
    const uint32_t base = c * K;
    const uint32_t m = A.n - base < K ? A.n - base : K;
    const uint32_t cols = A.tg.pset_cnt_total;
    uint32_t* pre_ks = A.pre + (size_t)c * 2 * cols;
    uint32_t* pre_kc = pre_ks + cols;
    const bool lane = tid < m;
    const uint32_t i = base + tid;
    uint32_t flag = 0, ns = 0;
    double sc[PE_MAX_SCORES];
    for (int k = 0; k < PE_MAX_SCORES; k++) sc[k] = 0.0;
    if (lane) {   // the walk's record, loaded beside everything else
        flag = (A.status[i] == 0 ? 1u : 0u) | (A.own[i] ? 2u : 0u);
        ns = A.rec[i].n_scores;
        for (int k = 0; k < PE_MAX_SCORES; k++) sc[k] = A.rec[i].scores[k];
    }
    if (tid < K) s_flag[tid] = flag;
    // the chunk positions before this wave's last lane: a wave-uniform loop bound
    const uint32_t jend = (tid | 63u) < m ? (tid | 63u) : m;
    double total = 0.0;
    for (int p = 0; p < A.tg.n_spread; p++) {
        const uint32_t off = A.tg.pset_cnt_off[p], nv = (uint32_t)A.tg.pset_nvals[p];
        uint32_t v = kMissing;
        if (lane) {
            v = A.val[(size_t)p * A.n + i];
            if (v >= nv) v = kMissing;
        }
        __syncthreads();   // the set before is read to its end
        if (tid < K) s_val[tid] = v;
        double b = -1.0;   // a node without a value
        if (A.tg.pset_even[p]) {
            const uint32_t *ep0 = A.ep0 + off, *craw0 = A.craw0 + off, *prop0 = A.prop0 + off;
            uint32_t *ks = pre_ks + off, *kc = pre_kc + off;
            if (nv <= (uint32_t)kLdsPsetValues) {
                for (uint32_t u = tid; u < nv; u += 256) {
                    s_col[0][u] = ep0[u];
                    s_col[1][u] = craw0[u];
                    s_col[2][u] = prop0[u];
                    s_col[3][u] = ks[u];
                    s_col[4][u] = kc[u];
                }
                ep0 = s_col[0];
                craw0 = s_col[1];
                prop0 = s_col[2];
                ks = s_col[3];
                kc = s_col[4];
            }
            __syncthreads();
            for (uint32_t j = 0; j < m; j++) {
                const uint32_t fj = s_flag[j], vj = s_val[j];
                if (!(fj & 1u) || vj == kMissing) continue;   // (uniform)
                const bool ownj = (fj & 2u) != 0;
                uint32_t lmn = 0xFFFFFFFFu, lmx = 0, lpr = 0;
                for (uint32_t u = tid; u < nv; u += 256) {
                    const uint32_t x = inplace_spread_count(ep0[u], craw0[u], prop0[u], ks[u], kc[u], ownj && u == vj);
                    if (x == 0) continue;
                    lpr++;
                    lmn = x < lmn ? x : lmn;
                    lmx = x > lmx ? x : lmx;
                }
                for (int o = 32; o > 0; o >>= 1) {
                    lmn = min(lmn, (uint32_t)__shfl_xor((int)lmn, o));
                    lmx = max(lmx, (uint32_t)__shfl_xor((int)lmx, o));
                    lpr += (uint32_t)__shfl_xor((int)lpr, o);
                }
                if ((tid & 63u) == 0) {
                    s_red[0][tid >> 6] = lmn;
                    s_red[1][tid >> 6] = lmx;
                    s_red[2][tid >> 6] = lpr;
                }
                __syncthreads();
                if (tid == 0) {
                    uint32_t mn = 0xFFFFFFFFu, mx = 0, present = 0;
                    for (int w = 0; w < 4; w++) {
                        mn = min(mn, s_red[0][w]);
                        mx = max(mx, s_red[1][w]);
                        present += s_red[2][w];
                    }
                    if (present == 0) mn = 0;   // no used value: min = max = 0
                    const uint32_t cur = inplace_spread_count(ep0[vj], craw0[vj], prop0[vj], ks[vj], kc[vj], ownj);
                    s_boost[j] = even_boost_of(mn, mx, present, cur);
                    ks[vj] += 1u;   // the update's AppendAlloc, and its stop that stays
                    if (ownj) kc[vj] += 1u;
                }
                __syncthreads();
            }
            if ((flag & 1u) && v != kMissing) b = s_boost[tid];
        } else {
            __syncthreads();
            uint32_t ksl = 0, kcl = 0;
#pragma unroll 8
            for (uint32_t j = 0; j < jend; j++) {
                const uint32_t fj = s_flag[j];
                const bool hit = j < tid && (fj & 1u) && s_val[j] == v;
                ksl += hit ? 1u : 0u;
                kcl += hit ? (fj >> 1) & 1u : 0u;
            }
            if ((flag & 1u) && v != kMissing) {
                const uint32_t cnt = inplace_spread_count(A.ep0[off + v], A.craw0[off + v], A.prop0[off + v],
                                                          pre_ks[off + v] + ksl, pre_kc[off + v] + kcl, (flag & 2u) != 0);
                b = target_boost_of(A.tg.pset_desired[p][v], cnt, A.tg.pset_weight_frac[p]);
            }
        }
        total += b;
    }
    if (!(flag & 1u) || total == 0.0) return;   // without a spread part the walk's record is final
    EmitRec& o = A.rec[i];
    if (ns == 0 || ns >= (uint32_t)PE_MAX_SCORES) return;
    double sum = sc[0];
#pragma unroll
    for (uint32_t k = 1; k < (uint32_t)PE_MAX_SCORES; k++)
        if (k < ns) sum += sc[k];
    sum += total;   // SpreadIterator (spread.go:110-174)
    o.scores[ns] = total;
    ns++;
    const double fs = sum / (double)ns;   // ScoreNormalizationIterator (rank.go:762-767)
    o.n_scores = ns;
    o.final_score = fs;
    if (A.named) {
        A.named[(size_t)i * kInplaceNamed + 4] = total;
        A.named[(size_t)i * kInplaceNamed + 5] = fs;
    }
}

// One plain (node, group) step on a lane's register image: the pipeline every
// other path runs (the same status_loaded / score_into, so the same bits). With
// kNamed (the AllocMetric forms) an option's ScoreNode values
// go to named[0] (binpack) and named[1] (devices, for an ask that scores them)
// as k_trace gives them: score_into's parts, the same sum in the same order.
template <bool kNamed = false>
__device__ __forceinline__ int sysg_plain(const NodeSoA& soa, const SysGroup& G, double log10, uint32_t row, NodeIn& in,
                                          uint32_t& cj, uint32_t& df, double* score, double* named = nullptr) {
    in.coll_tg = G.tg.coll_tg[row];
    in.feas = G.tg.node_feas ? G.tg.node_feas[row] : 1u;
    in.dev_free = df;
    ScoreIn si;
    const int st = status_loaded<false>(soa, G.tg, G.tg.class_ok, G.ask, 0u, row, in, &si);
    *score = 0.0;
    if (st == kOption) {
        lookup_scores(G.tg, nullptr, nullptr, row, in.r.cls, &si);
        uint32_t ns;
        if (kNamed) {
            double parts[PE_MAX_SCORES];
            *score = score_into<true>(G.ask, log10, si, parts, &ns);
            named[0] = parts[0];
            named[1] = ns > 1u ? parts[1] : 0.0;   // (used for an ask with dev_tw != 0: score_head's second part)
        } else {
            *score = score_into<false>(G.ask, log10, si, nullptr, &ns);
        }
        in.r.used_cpu += G.ask.cpu;
        in.r.used_mem += G.ask.mem;
        in.r.used_disk += G.ask.disk;
        in.r.used_mbits += G.ask.commit_mbits;
        in.r.used_dyn += G.ask.commit_dyn;
        cj += 1u;
        soa.coll_job[row] = cj;
        G.tg.coll_tg[row] = in.coll_tg + 1u;
        if (G.ask.n_dev > 0) df = dev_after(G.ask, G.tg.dev_cls[in.r.cls], df, 1);
    }
    return st;
}

// A lane's register image of its node back to HBM.
__device__ __forceinline__ void sysg_store(const SystemGroupsArgs& A, uint32_t row, const NodeIn& in, uint32_t df,
                                           uint32_t df0) {
    NodeRec& r = A.soa.rec[row];
    r.used_cpu = in.r.used_cpu;
    r.used_mem = in.r.used_mem;
    r.used_disk = in.r.used_disk;
    r.used_mbits = in.r.used_mbits;
    r.used_dyn = in.r.used_dyn;
    if (df != df0) A.dev_free[row] = df;
}

// Min of `key` over the wave's 64 lanes; every lane of the wave calls it.
__device__ __forceinline__ unsigned long long wave_min64(unsigned long long key) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off);
        key = o < key ? o : key;
    }
    return key;
}

// SystemScheduler.computePlacements' loop (scheduler_system.go:283-425) over
// every (node, task group) pair of a job with several groups: the nodes are
// independent, the groups of one node are not (an earlier group's ask shrinks
// what a later one finds). One lane per list position (or per snapshot row in
// the row-order form, as k_system_rows) loads the node once, keeps its record
// in registers and walks the chunk's groups in order with the pipeline every
// other path runs (sysg_plain); an option adds the group's ask to the
// registers as k_system's commit does. The groups' tables are one HBM array:
// every lane of a wave reads the same element. coll_job is written through
// (status_loaded reads the column); the record is stored once, only if
// something was placed. Outcomes go to res (sys_box); the per-group outcome
// counts are one ballot per code and wave, summed in LDS, one atomic per
// workgroup and counter. The grid-stride loop is over whole workgroup-sized
// blocks of lanes so that the wave reductions run in uniform control flow; a
// lane without a node (`act` false) walks nothing.
//
// kStop (a preempting stack): at the first group whose plain
// fit is exhausted the lane stops. That entry and the later ones stay
// unwritten and uncounted, the node's image goes back to HBM as at the end of
// the walk, the group is kept in resume[lane] and the lane joins the stopped
// list (one atomic per wave; the list's order is free, the nodes are
// independent). A later chunk skips the lanes an earlier chunk stopped.
//
// kMetrics (AllocMetric on): the same walk on the same register
// image, so the same outcomes and FinalScore bits. Beside them
//  - the named scores of M.dev_group's plain placements, by list position;
//  - without kStop, the first exhausted entry of each group in walk order: at
//    the group where the plain fit is exhausted the lane derives the dimension
//    from its image (trace_offers, trace_fit: what that Select saw after the
//    earlier groups' placements on the node); the key pos << 32 | code is
//    reduced with min over the wave, one LDS atomicMin per wave, one global
//    atomicMin per workgroup and group. In the row-order form pos is
//    rank_of[i], not the lane's index. With kStop an exhausted plain fit is not
//    a final outcome and nothing is recorded for it.
template <bool kStop, bool kMetrics>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
k_system_groups(SystemGroupsArgs A, SysStopArgs S, SysMetricsArgs M) {
    constexpr bool kFirst = kMetrics && !kStop;
    __shared__ uint32_t cnt[3 * kSysGroupsChunk];
    __shared__ unsigned long long first[kFirst ? kSysGroupsChunk : 1];
    if (threadIdx.x < 3 * kSysGroupsChunk) cnt[threadIdx.x] = 0;
    if (kFirst && threadIdx.x < kSysGroupsChunk) first[threadIdx.x] = ~0ull;
    __syncthreads();
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t span = A.rank_of ? A.n_rows : A.n_list;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = blockIdx.x * blockDim.x; base < span; base += stride) {
        const uint32_t i = base + threadIdx.x;
        bool act = i < span;
        uint32_t row = i, pos = i;
        if (act) {
            if (A.rank_of) {
                pos = A.rank_of[i];
                act = pos != PE_NONE;
            } else {
                row = A.list[i];
            }
        }
        if (kStop && act && A.k0 > 0 && S.resume[i] < A.k0) act = false;   // stopped in an earlier chunk
        NodeIn in = {};
        uint32_t cj = 0, df0 = 0;
        if (act) {
            in.r = A.soa.rec[row];
            cj = A.soa.coll_job[row];
            df0 = A.dev_free ? A.dev_free[row] : 0u;
        }
        uint32_t df = df0;
        bool dirty = false;
        uint32_t stop_at = A.n_tg;
        uint64_t* out = A.res + (size_t)i * A.n_tg + A.k0;
        for (uint32_t kk = 0; kk < A.nk; kk++) {
            const SysGroup& G = A.groups[A.k0 + kk];
            int st = -1;   // no outcome: no node, or stopped
            double score = 0.0, named[2];
            if (act && stop_at == A.n_tg) {
                st = sysg_plain<kMetrics>(A.soa, G, A.log10, row, in, cj, df, &score, kMetrics ? named : nullptr);
                if (kStop && st == kExhausted) {
                    stop_at = A.k0 + kk;
                    st = -1;
                }
            }
            if (st >= 0) out[kk] = sys_box(st, score);
            if (st == kOption) {
                dirty = true;
                if (kMetrics && (int32_t)(A.k0 + kk) == M.dev_group) {
                    M.dev_named[pos] = named[0];
                    M.dev_named[(size_t)M.n_list + pos] = named[1];
                }
            }
            const uint64_t m0 = __ballot(st == kOption), m1 = __ballot(st == kFiltered), m2 = __ballot(st == kExhausted);
            if (lane == (uint32_t)__ffsll((unsigned long long)(m0 | m1 | m2)) - 1u) {
                if (m0) atomicAdd(&cnt[3 * kk + 0], (uint32_t)__popcll(m0));
                if (m1) atomicAdd(&cnt[3 * kk + 1], (uint32_t)__popcll(m1));
                if (m2) atomicAdd(&cnt[3 * kk + 2], (uint32_t)__popcll(m2));
            }
            if (kFirst && m2) {   // wave-uniform
                unsigned long long key = ~0ull;
                if (st == kExhausted) {
                    uint32_t code = trace_offers(G.tg, G.ask, row, in, 0u);
                    if (code == kTrOption) code = trace_fit(A.soa, G.ask, row, in.r, 0u, false);
                    key = ((unsigned long long)pos << 32) | code;
                }
                key = wave_min64(key);
                if (lane == 0) atomicMin(&first[kk], key);
            }
        }
        if (kStop && act) {
            if (A.k0 == 0 || stop_at < A.n_tg) S.resume[i] = stop_at;
            if (stop_at < A.n_tg) S.stopped[wave_slot(S.n_stopped)] = i;
        }
        if (act && dirty) sysg_store(A, row, in, df, df0);
    }
    __syncthreads();
    if (threadIdx.x < 3 * A.nk && cnt[threadIdx.x])
        atomicAdd(&A.counts[(size_t)(blockIdx.x % kPlacedSlots) * 3u * A.n_tg + 3u * A.k0 + threadIdx.x], cnt[threadIdx.x]);
    if (kFirst && threadIdx.x < A.nk && first[threadIdx.x] != ~0ull)
        atomicMin(&M.first[A.k0 + threadIdx.x], first[threadIdx.x]);
}

// The eviction walk over the stopped nodes, one lane per node, at eviction
// width W. The group loop is wave-uniform (group k's tables and PreemptArgs are
// read by every lane at once); a lane acts at its resume group and after it:
// BinPack with evict (evict_eval) where the plain fit is exhausted, on an
// option k_commit_evicted's commit of one row and a record [entry, W mask
// words] in the append buffer, then the plain walk as k_system_groups<true, *> to
// the next exhausted group. evict_eval and the commit work on HBM, so the image
// is stored before the call and loaded again after a commit: a lane reads back
// its own stores only. A node beyond the width commits nothing from that group
// on: it keeps its resume group, joins the wider list and raises kEvictWider.
//
// kMetrics (DESIGN.md §34, A.M): evict_eval also returns the dimension of a
// pair that stays exhausted and an option's named scores; plain placements
// take sysg_plain's named form. Every finally
// exhausted entry offers pos << 32 | dimension to its group's first-failure
// word: the lanes of a wave stand at different groups here, so there is no
// wave-wide reduction; a lane compares with the word in LDS (groups below
// kSysFirstLds, flushed with one global atomicMin per workgroup and group) and
// issues the atomicMin only when it would lower it.
template <int W, bool kMetrics = false>
__global__ void __launch_bounds__(256) k_system_groups_evict(SysEvictArgs A) {
    __shared__ unsigned long long first_lds[kMetrics ? kSysFirstLds : 1];
    const SysMetricsArgs* M = &A.M;
    if (kMetrics) {
        for (uint32_t k = threadIdx.x; k < kSysFirstLds; k += blockDim.x) first_lds[k] = ~0ull;
        __syncthreads();
    }
    const SystemGroupsArgs& Gx = A.G;
    const uint32_t n = *A.n_stopped;
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* counts = Gx.counts + (size_t)(blockIdx.x % kPlacedSlots) * 3u * Gx.n_tg;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        const uint32_t i = A.stopped[j];
        uint32_t row = i, pos = i;
        if (Gx.rank_of) pos = Gx.rank_of[i];
        else row = Gx.list[i];
        uint32_t next = A.resume[i];
        bool evict = true;   // the plain fit at the resume group is known: exhausted
        NodeIn in;
        in.r = Gx.soa.rec[row];
        uint32_t cj = Gx.soa.coll_job[row];
        uint32_t df0 = Gx.dev_free ? Gx.dev_free[row] : 0u;
        uint32_t df = df0;
        bool dirty = false;
        uint64_t* out = Gx.res + (size_t)i * Gx.n_tg;
        EvictWs<W> ws;
        for (uint32_t k = 0; k < Gx.n_tg; k++) {
            if (k != next) continue;
            int st = kExhausted;
            double score = 0.0;
            double named[7];   // (kMetrics: sysg_plain fills [0..1], evict_eval all seven)
            uint32_t dim = 0;
            if (!evict) {
                st = sysg_plain<kMetrics>(Gx.soa, Gx.groups[k], Gx.log10, row, in, cj, df, &score,
                                          kMetrics ? named : nullptr);
                dirty = dirty || st == kOption;
                evict = st == kExhausted;
            }
            if (evict) {
                if (dirty) sysg_store(Gx, row, in, df, df0);
                dirty = false;
                const PreemptArgs& P = A.pre[k];
                NodeEval ev;
                AMask<W> mask = AMask<W>::zero();
                uint32_t offers = 0, unsup = 0, nflags = 0;
                const int es = evict_eval<false, false, W>(P, row, &ev, &mask, &offers, &unsup, &ws,
                                                           kMetrics ? named : nullptr, kMetrics ? &nflags : nullptr,
                                                           kMetrics ? &dim : nullptr);
                if (es != kExhausted) dim = 0;   // (a skipped eviction Select records no dimension)
                if (unsup) {
                    atomicOr(A.flags, unsup);
                    if (unsup == kEvictWider) {
                        A.resume[i] = k;
                        A.wider[wave_slot(A.n_wider)] = i;
                    }
                    next = PE_NONE;   // nothing more for this node in this launch
                    continue;
                }
                if (es == kOption) {
                    commit_evicted_row(P, row, mask, &offers, A.preempted, A.pcount, A.dev_free_all);
                    in.r = Gx.soa.rec[row];
                    cj = Gx.soa.coll_job[row];
                    df0 = Gx.dev_free ? Gx.dev_free[row] : 0u;
                    df = df0;
                    st = kOption;
                    score = ev.score;
                    const uint32_t at = wave_slot(A.n_app);
                    if (at < A.app_cap) {
                        uint32_t* rec = A.app + (size_t)at * (1u + W);
                        rec[0] = pos * Gx.n_tg + k;
                        mask.store(rec + 1);
                    } else {
                        atomicOr(A.flags, kSysgOverflow);
                    }
                }
            }
            out[k] = sys_box(st, score);
            if (kMetrics) {
                if (st == kOption && (int32_t)k == M->dev_group) {
                    M->dev_named[pos] = named[0];
                    M->dev_named[(size_t)M->n_list + pos] = named[1];
                }
                if (st == kExhausted) {
                    const unsigned long long key = ((unsigned long long)pos << 32) | dim;
                    if (k < kSysFirstLds) {
                        if (key < first_lds[k]) atomicMin(&first_lds[k], key);
                    } else if (key < M->first[k]) {
                        atomicMin(&M->first[k], key);
                    }
                }
            }
            const uint64_t m0 = __ballot(st == kOption), m1 = __ballot(st == kFiltered), m2 = __ballot(st == kExhausted);
            if (lane == (uint32_t)__ffsll((unsigned long long)(m0 | m1 | m2)) - 1u) {
                if (m0) atomicAdd(&counts[3 * k + 0], (uint32_t)__popcll(m0));
                if (m1) atomicAdd(&counts[3 * k + 1], (uint32_t)__popcll(m1));
                if (m2) atomicAdd(&counts[3 * k + 2], (uint32_t)__popcll(m2));
            }
            evict = false;
            next = k + 1u;
        }
        if (dirty) sysg_store(Gx, row, in, df, df0);
    }
    if (kMetrics) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < kSysFirstLds && k < Gx.n_tg; k += blockDim.x)
            if (first_lds[k] != ~0ull) atomicMin(&M->first[k], first_lds[k]);
    }
}

// The outcome of entry e (position-major, group-minor) from res: 0 placed,
// 1 filtered, 2 exhausted; *v its boxed word.
__device__ __forceinline__ uint32_t sysg_entry(const SysCompactArgs& A, uint32_t e, uint64_t* v) {
    size_t at = e;
    if (A.list) {
        const uint32_t pos = e / A.n_tg;
        at = (size_t)A.list[pos] * A.n_tg + (e - pos * A.n_tg);
    }
    const uint64_t x = A.res[at];
    *v = x;
    return (x & 0xFFFFFFFFFFFFFFF0ull) == 0x7FF8000000000000ull ? (uint32_t)(x & 3u) : (uint32_t)kOption;
}

// Compaction, step one: each lane packs its four entries into one outcome byte
// (coalesced byte stores); the tile's placed count goes to tile_off[tile].
__global__ void __launch_bounds__(256) k_sysg_pack(SysCompactArgs A) {
    __shared__ uint32_t red[4];
    const uint32_t e0 = blockIdx.x * kSysTile + threadIdx.x * 4u;
    uint32_t byte = 0, placed = 0;
    for (uint32_t j = 0; j < 4; j++) {
        if (e0 + j >= A.n_entries) break;
        uint64_t v;
        const uint32_t code = sysg_entry(A, e0 + j, &v);
        byte |= code << (2u * j);
        placed += code == (uint32_t)kOption;
    }
    if (e0 < A.n_entries) A.status2[e0 >> 2] = (uint8_t)byte;
    for (int off = 32; off > 0; off >>= 1) placed += __shfl_xor(placed, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = placed;
    __syncthreads();
    if (threadIdx.x == 0) A.tile_off[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// Step two, one workgroup: the exclusive scan of the tile counts in place, the
// total and the summed per-group counters into the mapped header words.
__global__ void __launch_bounds__(256) k_sysg_scan(SysCompactArgs A) {
    __shared__ uint32_t sh[256];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < A.n_tiles; base += 256) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t own = t < A.n_tiles ? A.tile_off[t] : 0u;
        sh[threadIdx.x] = own;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {
            const uint32_t add = threadIdx.x >= d ? sh[threadIdx.x - d] : 0u;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (t < A.n_tiles) A.tile_off[t] = carry + sh[threadIdx.x] - own;
        carry += sh[255];
        __syncthreads();
    }
    // one wave per counter, one lane per slot; the slots are left zero for the next call
    static_assert(kPlacedSlots == 64, "one lane per counter slot");
    for (uint32_t c = threadIdx.x >> 6; c < 3u * A.n_tg; c += 4) {
        uint32_t* slot = &A.counts[(size_t)(threadIdx.x & 63u) * 3u * A.n_tg + c];
        uint32_t sum = *slot;
        *slot = 0;
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if ((threadIdx.x & 63u) == 0) A.hdr[1 + c] = sum;
    }
    if (threadIdx.x == 0) A.hdr[0] = carry;
    __threadfence_system();
}

// Step three: the placed entries' scores to their dense positions, the tile's
// offset plus a ballot / popcount prefix over the lanes below.
__global__ void __launch_bounds__(256) k_sysg_scatter(SysCompactArgs A) {
    __shared__ uint32_t wave_n[4];
    const uint32_t e0 = blockIdx.x * kSysTile + threadIdx.x * 4u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t v[4];
    bool hit[4];
    uint32_t below = 0, total = 0;
    for (uint32_t j = 0; j < 4; j++) {
        hit[j] = false;
        v[j] = 0;
        if (e0 + j < A.n_entries) hit[j] = sysg_entry(A, e0 + j, &v[j]) == (uint32_t)kOption;
        const uint64_t m = __ballot(hit[j]);
        below += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        total += (uint32_t)__popcll(m);
    }
    if (lane == 0) wave_n[wave] = total;
    __syncthreads();
    uint32_t at = A.tile_off[blockIdx.x] + below;
    for (uint32_t w = 0; w < wave; w++) at += wave_n[w];
    for (uint32_t j = 0; j < 4; j++)
        if (hit[j]) A.score[at++] = __longlong_as_double((long long)v[j]);
}

// (defined last: the kernels above keep their places in the code object)
// pe_place_csi_full's count loop: a CSI group that runs full passes (node
// affinities, spreads, or a limit latched to MaxInt32). k_place's full-pass
// shape (one workgroup, lanes stride over relative positions from the cursor,
// the spread tables rebuilt per placement, the overlay and the counts in LDS)
// with k_csi_loop's wrapper bit, code column and stop test, and csi_limit.h's
// fold at an unbounded limit: no serial loop over options.
// Per placement:
//   1 every position is evaluated without CSI and classified (filtered,
//     exhausted, option, stop); its class and score go to ev_kind / ev_score,
//     written and read back by the same lane. A block prefix per chunk of BLOCK
//     positions collects, in position order, the first kCsiFullNils stops and the
//     first kCsiFullOptions non-positive options. Chunks past the kCsiFullNils-th
//     stop are not evaluated: no Select consumes them.
//   2 the specials, merged by position, delimit at most kCsiFullSpecials + 1
//     segments. Every lane reduces its positions of each segment (first strict
//     maximum, option / non-positive / filtered / exhausted counts), every wave
//     its lanes by shuffles; the per-wave partials of all segments meet in LDS.
//   3 lane 0 merges the partials and steps csi_full_fold over specials and
//     collapsed segments. A Select at this limit ends at a special or at the end
//     of the list, so consumed / filtered / exhausted are sums over whole segments.
//   4 record, commit, next placement.
// Every loop is bounded without the data: positions by n, specials and segments
// by csi_limit.h's constants, placements by count. A bound that does not hold
// writes no record and raises eval_status[2], as k_csi_loop.
// kMetrics (pe_place_csi_full_metrics): k_csi_loop<true>'s trace log, one byte per
// consumed position of the call at index walked + j (csi_reason.h). The length a
// Select consumes is known after the fold only, so pass 1 stores the byte of
// every position it classifies; the bytes past `consumed` are stored again by
// the next placement, whose log starts at walked + consumed, behind the barriers
// between placements, or belong to no record. walked + j < count * n_visit.
constexpr int kCsiFullBlock = 512;
enum : uint8_t { kFullFiltered = 0, kFullExhausted = 1, kFullOption = 2, kFullStop = 3 };

template <int BLOCK>
struct CsiFullShared {
    uint32_t scratch[4];                         // build_spread_table
    uint32_t wave_cnt[BLOCK / 64];               // pass 1: stops | non-positive options << 16 of each wave
    uint32_t stop_pos[kCsiFullNils];
    uint32_t np_pos[kCsiFullOptions];
    double np_score[kCsiFullOptions];
    CsiSpecial sp[kCsiFullSpecials];
    CsiSegment seg[kCsiFullSpecials + 1];
    uint32_t seg_filt[kCsiFullSpecials + 1], seg_exh[kCsiFullSpecials + 1];
    uint32_t n_spec, end_pos, closed;
    // pass 2: per segment and wave
    double part_score[kCsiFullSpecials + 1][BLOCK / 64];
    uint32_t part_pos[kCsiFullSpecials + 1][BLOCK / 64];
    uint32_t part_cnt[kCsiFullSpecials + 1][BLOCK / 64][4];   // options, non-positive, filtered, exhausted
    // the Select's outcome
    int best_pos;
    uint32_t consumed, n_filtered, n_exhausted, err;
    double best_score;
};

template <int BLOCK, bool kMetrics>
__global__ void __launch_bounds__(BLOCK) k_csi_full(BatchArgs A, CsiLoopArgs C, double* ev_score, uint8_t* ev_kind,
                                                    uint8_t* log, uint32_t log_cap) {
    __shared__ CsiFullShared<BLOCK> sh;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
    constexpr int W = BLOCK / 64;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t n = A.n_visit;
    const uint32_t* perm = A.perms;
    const uint8_t* class_ok = A.tg.class_ok;

    // the spread tables, the counts and the overlay out of dynamic LDS (as k_place<*, true, *>)
    const uint32_t H = 1u << A.hash_bits;
    unsigned char* p = dyn_smem;
    double* spread_tab = nullptr;
    uint32_t* counts = nullptr;
    if (A.pset_g_tab) {   // tables beyond the LDS budget: the HBM copy
        spread_tab = A.pset_g_tab;
        counts = A.pset_g_cnt;
    } else {
        spread_tab = reinterpret_cast<double*>(p);
        counts = reinterpret_cast<uint32_t*>(p + sizeof(double) * A.tg.pset_tab_total);
        p += A.pset_lds;
    }
    Overlay ov;
    ov.bits = A.hash_bits;
    ov.mask = H - 1;
    ov.keys = reinterpret_cast<uint32_t*>(p); p += 4 * H;
    ov.k = reinterpret_cast<uint32_t*>(p); p += 4 * H;
    for (uint32_t i = tid; i < H; i += BLOCK) ov.keys[i] = kEmpty;
    for (int q = 0; q < A.tg.n_psets; q++)
        for (int v = tid; v < A.tg.pset_nvals[q]; v += BLOCK) counts[A.tg.pset_cnt_off[q] + v] = A.tg.pset_counts[q][v];
    __syncthreads();

    uint32_t offset = n ? A.offset0 % n : 0u;
    uint32_t placed = 0;
    uint64_t walked = 0;   // positions consumed since the call began
    uint32_t fold_err = 0;

    for (uint32_t it = 0; n && it < A.count; it++) {
        if (A.tg.n_psets > 0) build_spread_table<BLOCK>(A.tg, counts, spread_tab, sh.scratch);
        const uint32_t set = min((uint32_t)C.set_of[it], C.n_sets - 1u);
        const uint16_t* codes = C.codes + (size_t)set * C.n_rows;

        // ---- 1: classify every position; the first stops and non-positive options in position order
        uint32_t n_stop = 0, n_np = 0;
        for (uint32_t base = 0; base < n && n_stop < (uint32_t)kCsiFullNils; base += BLOCK) {
            const uint32_t j = base + (uint32_t)tid;
            uint8_t kind = kFullFiltered;
            double score = 0.0;
            if (j < n) {
                uint32_t pos = offset + j;
                if (pos >= n) pos -= n;
                const uint32_t row = perm[pos];
                const uint32_t c = A.soa.rec[row].cls;
                // FeasibilityWrapper's verdict without CSI: the node reaches the availability checker
                const bool reach = class_ok[c] != 0 && (!A.tg.node_ok || A.tg.node_ok[row] != 0);
                const bool unavailable = reach && row < C.n_rows && codes[row] != 0;
                if (unavailable && !C.escaped) {
                    const uint8_t cs = c < C.ncls ? C.cls_state[c] : (uint8_t)kCsiClsNever;
                    if (cs == kCsiClsEligible || (cs == kCsiClsOpen && walked + (uint64_t)j > (uint64_t)C.first[c]))
                        kind = kFullStop;
                }
                if (reach && !unavailable) {
                    NodeEval ev;
                    ev.score = 0.0;
                    eval_node<false>(A.soa, A.tg, class_ok, A.ask, ov, A.penalty_bits, A.log10, spread_tab, row, &ev);
                    if (ev.status == kOption) {
                        kind = kFullOption;
                        score = ev.score;
                    } else if (ev.status == kExhausted) {
                        kind = kFullExhausted;
                    }
                }
                ev_kind[j] = kind;
                ev_score[j] = score;
                if constexpr (kMetrics) {
                    const uint64_t at = walked + (uint64_t)j;
                    if (at < (uint64_t)log_cap)
                        log[at] = csi_log_pack(unavailable ? (uint32_t)codes[row] : 0u, kind == kFullStop);
                }
            }
            const bool is_stop = kind == kFullStop;
            const bool is_np = kind == kFullOption && score <= 0.0;
            const uint64_t ms = __ballot(is_stop), mn = __ballot(is_np);
            if (lane == 0) sh.wave_cnt[wid] = (uint32_t)__popcll(ms) | (uint32_t)__popcll(mn) << 16;
            __syncthreads();
            uint32_t before = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < W; w++) {
                const uint32_t x = sh.wave_cnt[w];
                before += w < wid ? x : 0u;
                tot += x;
            }
            const uint32_t rank_s = n_stop + (before & 0xFFFFu) + lanes_below(ms, lane);
            const uint32_t rank_n = n_np + (before >> 16) + lanes_below(mn, lane);
            if (is_stop && rank_s < (uint32_t)kCsiFullNils) sh.stop_pos[rank_s] = j;
            if (is_np && rank_n < (uint32_t)kCsiFullOptions) {
                sh.np_pos[rank_n] = j;
                sh.np_score[rank_n] = score;
            }
            n_stop += tot & 0xFFFFu;
            n_np += tot >> 16;
            __syncthreads();
        }

        // ---- the specials by position
        if (tid == 0) {
            const uint32_t ns = min(n_stop, (uint32_t)kCsiFullNils), nn = min(n_np, (uint32_t)kCsiFullOptions);
            const bool closed = n_stop >= (uint32_t)kCsiFullNils;
            const uint32_t end = closed ? sh.stop_pos[kCsiFullNils - 1] + 1u : n;
            uint32_t a = 0, b = 0, k = 0;
            for (int t = 0; t < kCsiFullSpecials; t++) {
                const uint32_t pa = a < ns ? sh.stop_pos[a] : 0xFFFFFFFFu;
                const uint32_t pb = b < nn && sh.np_pos[b] < end ? sh.np_pos[b] : 0xFFFFFFFFu;
                if (pa == 0xFFFFFFFFu && pb == 0xFFFFFFFFu) break;
                if (pa < pb) {
                    sh.sp[k].pos = pa;
                    sh.sp[k].kind = kCsiNil;
                    sh.sp[k].score = 0.0;
                    a++;
                } else {
                    sh.sp[k].pos = pb;
                    sh.sp[k].kind = kCsiOption;
                    sh.sp[k].score = sh.np_score[b];
                    b++;
                }
                k++;
            }
            sh.n_spec = k;
            sh.end_pos = end;
            sh.closed = closed ? 1u : 0u;
        }
        __syncthreads();

        // ---- 2: every segment's partials per wave
        const uint32_t n_spec = sh.n_spec, end_pos = sh.end_pos;
        const bool closed = sh.closed != 0;
        const uint32_t n_seg = n_spec + (closed ? 0u : 1u);
        for (uint32_t g = 0; g < n_seg && g <= (uint32_t)kCsiFullSpecials; g++) {
            const uint32_t lo = g ? sh.sp[g - 1].pos + 1u : 0u;
            const uint32_t hi = g < n_spec ? sh.sp[g].pos : end_pos;
            if (lo >= hi) continue;   // (uniform)
            double bs = -__builtin_inf();
            uint32_t bp = 0xFFFFFFFFu;
            uint32_t c_opt = 0, c_np = 0, c_filt = 0, c_exh = 0;
            // this lane's positions of [lo, hi): j = tid (mod BLOCK), increasing, so `>` keeps the first maximum
            for (uint32_t j = lo + (((uint32_t)tid + (uint32_t)BLOCK - lo % (uint32_t)BLOCK) % (uint32_t)BLOCK); j < hi;
                 j += BLOCK) {
                const uint8_t kind = ev_kind[j];
                if (kind == kFullOption) {
                    const double sc = ev_score[j];
                    c_opt++;
                    c_np += sc <= 0.0 ? 1u : 0u;
                    if (sc > bs) { bs = sc; bp = j; }
                } else if (kind == kFullExhausted) {
                    c_exh++;
                } else {
                    c_filt++;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double os = __shfl_xor(bs, off);
                const uint32_t op = (uint32_t)__shfl_xor((int)bp, off);
                if (os > bs || (os == bs && op < bp)) { bs = os; bp = op; }
                c_opt += (uint32_t)__shfl_xor((int)c_opt, off);
                c_np += (uint32_t)__shfl_xor((int)c_np, off);
                c_filt += (uint32_t)__shfl_xor((int)c_filt, off);
                c_exh += (uint32_t)__shfl_xor((int)c_exh, off);
            }
            if (lane == 0) {
                sh.part_score[g][wid] = bs;
                sh.part_pos[g][wid] = bp;
                sh.part_cnt[g][wid][0] = c_opt;
                sh.part_cnt[g][wid][1] = c_np;
                sh.part_cnt[g][wid][2] = c_filt;
                sh.part_cnt[g][wid][3] = c_exh;
            }
        }
        __syncthreads();

        // ---- 3: the segments, and the fold over specials and collapsed segments
        if (tid == 0) {
            for (uint32_t g = 0; g <= (uint32_t)kCsiFullSpecials; g++) {
                CsiSegment sg = {0u, 0u, -1, 0u, 0.0};
                uint32_t f = 0, x = 0;
                const uint32_t lo = g && g <= n_spec ? sh.sp[g - 1].pos + 1u : 0u;
                const uint32_t hi = g < n_spec ? sh.sp[g].pos : end_pos;
                if (g < n_seg && lo < hi) {
                    double bs = -__builtin_inf();
                    uint32_t bp = 0xFFFFFFFFu;
                    for (int w = 0; w < W; w++) {
                        const double os = sh.part_score[g][w];
                        const uint32_t op = sh.part_pos[g][w];
                        if (os > bs || (os == bs && op < bp)) { bs = os; bp = op; }
                        sg.options += sh.part_cnt[g][w][0];
                        sg.nonpos += sh.part_cnt[g][w][1];
                        f += sh.part_cnt[g][w][2];
                        x += sh.part_cnt[g][w][3];
                    }
                    if (sg.options) { sg.score = bs; sg.id = (int32_t)bp; }
                }
                sh.seg[g] = sg;
                sh.seg_filt[g] = f;
                sh.seg_exh[g] = x;
            }
            CsiLimit L;
            uint32_t ended_at = 0;
            const int frc = csi_full_fold(L, sh.seg, sh.sp, n_spec, closed, &ended_at);
            uint32_t nf = 0, nx = 0;
            // the segments up to the end, and the stops among the specials consumed (a stop counts as filtered)
            for (uint32_t g = 0; g <= (uint32_t)kCsiFullSpecials; g++) {
                const bool seg_in = frc == 0 ? g <= ended_at : g < n_seg;
                const bool sp_in = g < n_spec && (frc == 0 ? g <= ended_at : true);
                if (seg_in) { nf += sh.seg_filt[g]; nx += sh.seg_exh[g]; }
                if (sp_in && g < (uint32_t)kCsiFullSpecials && sh.sp[g].kind == kCsiNil) nf++;
            }
            sh.err = frc < 0 ? 1u : 0u;
            sh.consumed = frc == 0 ? sh.sp[min(ended_at, (uint32_t)kCsiFullSpecials - 1u)].pos + 1u : n;
            sh.n_filtered = nf;
            sh.n_exhausted = nx;
            sh.best_pos = L.best_id;
            sh.best_score = L.best_score;
        }
        __syncthreads();
        if (sh.err) {   // csi_limit.h's bounds do not hold: no record, the host fails the call
            fold_err = 1u;
            break;
        }

        // ---- 4: the record, the commit
        const int best_pos = sh.best_pos;
        const double best_score = sh.best_score;
        const uint32_t consumed = sh.consumed, n_filtered = sh.n_filtered, n_exhausted = sh.n_exhausted;
        int win_row = -1;
        if (best_pos >= 0 && (uint32_t)best_pos < n) {
            uint32_t pos = offset + (uint32_t)best_pos;
            if (pos >= n) pos -= n;
            win_row = (int)perm[pos];
        }
        uint32_t no = offset + (consumed % n);
        if (no >= n) no -= n;
        if (tid == 0) {
            emit_placement(A, class_ok, ov, spread_tab, 0u, it, win_row, best_score, consumed, n_filtered, n_exhausted,
                           no);
            if (win_row >= 0 && A.commit) commit_overlay(A.soa, A.tg, ov, counts, (uint32_t)win_row);
        }
        offset = no;
        walked += consumed;
        __syncthreads();
        if (win_row < 0) break;   // nil option: the loop ends, its record written
        placed++;
    }
    if (tid == 0) {
        A.eval_status[0] = placed;
        A.eval_status[1] = offset;
        A.eval_status[2] = fold_err;
    }
    if (A.writeback) writeback_overlay<BLOCK, true, true>(A, ov, H, counts);
}

}  // namespace pe

#include "probe.inc"

// ---- launch wrappers (host) ------------------------------------------------
hipError_t pe_launch_static_gate(const uint8_t* blocked, const uint32_t* coll_tg, uint32_t* gate, uint32_t n,
                                 hipStream_t st);
size_t pe_place_lds_bytes(bool full, int hash_bits, bool packed, size_t pset_bytes) {
    size_t b = (size_t)(packed ? 4u : 8u) * ((size_t)1 << hash_bits);
    if (full) b += pset_bytes;
    return b;
}

hipError_t pe_launch_place(const pe::BatchArgs* a, uint32_t n_evals, bool full, hipStream_t st) {
    if (full && a->packed_overlay) return hipErrorInvalidValue;   // packed entries: windowed kernel only
    const size_t lds = pe_place_lds_bytes(full, a->hash_bits, a->packed_overlay != 0, a->pset_lds);
    if (full) {
        // few evaluations: 1024-lane workgroups keep more rows in flight per pass
        // reserved cores are a separate instantiation (their code costs the others registers)
        const bool cores = a->ask.cores > 0;
        if (n_evals <= 64) {
            if (cores) hipLaunchKernelGGL((pe::k_place<1024, true, true>), dim3(n_evals), dim3(1024), lds, st, *a);
            else hipLaunchKernelGGL((pe::k_place<1024, true, false>), dim3(n_evals), dim3(1024), lds, st, *a);
        } else {
            if (cores) hipLaunchKernelGGL((pe::k_place<256, true, true>), dim3(n_evals), dim3(256), lds, st, *a);
            else hipLaunchKernelGGL((pe::k_place<256, true, false>), dim3(n_evals), dim3(256), lds, st, *a);
        }
    } else {
        hipLaunchKernelGGL(pe::k_window, dim3(n_evals), dim3(64), lds, st, *a);
    }
    return hipGetLastError();
}

// Phase-static windowed loop: k_base over the snapshot, then k_chain with a
// persistent grid of at most `max_blocks` workgroups (one evaluation each at a time).
uint32_t pe_chain_max_n() { return pe::kChainMaxN; }
uint32_t pe_emit_grid(uint32_t count) { return count ? (count + pe::kEmitBlock - 1) / pe::kEmitBlock : 1u; }
uint32_t pe_chain_max_limit() { return pe::kMaxChainLimit; }

size_t pe_chain_lds_bytes(int hash_bits, bool packed, uint32_t n) {
    if (n > pe::kChainMaxN) n = pe::kChainMaxN;   // nb / nx cover one window
    return (size_t)(packed ? 4u : 8u) * ((size_t)1 << hash_bits) + 4u * (((size_t)n + 3u) & ~(size_t)1);
}

int pe_chain_blocks_per_cu(size_t lds) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, pe::k_chain<pe::kChainItems, false>, pe::kChainBlock, lds) !=
            hipSuccess || nb <= 0)
        nb = 1;
    return nb;
}

// Shape of a launch: the fewest positions per lane that hold one window of
// the list. `forced` = 4 / 16 asks for a larger shape (tests run every shape
// on the same list); a smaller one than the list needs is never used.
int pe_chain_shape(uint32_t n_visit, int forced) {
    int items = n_visit > pe::kChainBlock * 4u ? 16 : (n_visit > pe::kChainBlock ? 4 : 1);
    if (forced > items) items = forced >= 16 ? 16 : 4;
    return items;
}

// Largest list / count / class table a fused launch (BatchArgs::fused) takes.
uint32_t pe_chain_fused_max_n() { return pe::kChainBlock * 4u; }
uint32_t pe_chain_fused_max_count() { return 256u; }
uint32_t pe_chain_fused_max_classes() { return pe::kFusedMaxClasses; }

// k_phases: dynamic LDS of a launch (its compact entries), and what a
// workgroup of the current device may add to the kernel's static LDS (0: no
// device); a launch past that keeps the two k_phase launches
static int lds_per_workgroup(int dev);

size_t pe_chain_one_lds_bytes(uint32_t n_visit, uint32_t count, uint32_t limit) {
    return pe::one_lds_bytes(pe::one_entries(n_visit, count, limit));
}

size_t pe_chain_one_max_dyn() {
    constexpr int kDevs = 64;
    static int v[kDevs];
    static bool init[kDevs];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kDevs) {
        (void)hipGetLastError();
        return 0;
    }
    if (!init[dev]) {
        hipFuncAttributes fa;
        if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&pe::k_phases)) != hipSuccess) {
            (void)hipGetLastError();
            return 0;
        }
        const int d = lds_per_workgroup(dev) - (int)fa.sharedSizeBytes;
        v[dev] = d > 0 ? d : 0;
        init[dev] = true;
    }
    return (size_t)v[dev];
}

bool pe_chain_one_fits(uint32_t n_visit, uint32_t count, uint32_t limit) {
    return n_visit != 0 && n_visit <= pe::kChainMaxN && count != 0 && limit != 0 && limit <= pe::kMaxChainLimit &&
           pe_chain_one_lds_bytes(n_visit, count, limit) <= pe_chain_one_max_dyn();
}

// split (or null): five events recorded before k_base and after k_base,
// k_chain, k_emit and k_emit_writeback (per-kernel device time, PE_KERNEL_SPLIT);
// wide_one: an armed launch resolves both wide phases in one k_phases launch
// (the caller checked pe_chain_one_fits)
hipError_t pe_launch_chain(const pe::BatchArgs* a, uint32_t n_evals, uint32_t max_blocks, int forced_items,
                           hipStream_t st, hipEvent_t* split, bool wide_one) {
    if (!a->base || !a->chain_vs || (a->n_visit > pe::kChainMaxN && n_evals != 1) || a->class_ok_stride ||
        a->limit > pe::kMaxChainLimit || a->count >= (1u << 18))   // redo entries pack count | position << 18
        return hipErrorInvalidValue;
    if (a->base_by_pos && n_evals != 1) return hipErrorInvalidValue;
    if (a->perm_src && (!a->base_by_pos || !a->perm_dst)) return hipErrorInvalidValue;
    if (a->fold.feas && (!a->fold.class_src || !a->fold.class_dst || a->fold.ncls > pe::kFoldMaxClasses))
        return hipErrorInvalidValue;
    // list_covers: k_base's pass over the list is the only writer of node_feas
    if (a->fold.list_covers && (!a->fold.feas || a->fused || !a->base_by_pos || a->n_visit != a->soa.n))
        return hipErrorInvalidValue;
    // wide phases: the unfused, by-position, single-evaluation chain with
    // deferred records and a writeback, no device asks or reserved cores
    const pe::ChainWide& wd = a->wide;
    if (wd.bits &&
        (n_evals != 1 || a->fused || !a->base_by_pos || !a->base1 || !a->emit || !a->emit_ov || !a->emit_n ||
         a->out || a->full_out || !a->commit || !a->writeback || a->ask.n_dev != 0 || a->ask.cores != 0 ||
         a->n_visit == 0 || a->n_visit > pe::kChainMaxN || wd.words != (a->n_visit + 31u) / 32u || !wd.won ||
         !wd.slot || !wd.seed || !wd.err || !wd.stats || wd.phases < 1 || wd.phases > 2))
        return hipErrorInvalidValue;
    const size_t lds = pe_chain_lds_bytes(a->hash_bits, a->packed_overlay != 0, a->n_visit);
    uint32_t grid = n_evals < max_blocks ? n_evals : max_blocks;
    if (grid == 0) grid = 1;
    const int items = pe_chain_shape(a->n_visit, forced_items);
    if (wd.bits && items != 1 && items != 4 && items != pe::kChainItems) return hipErrorInvalidValue;
    if (a->fused) {
        // one launch: fold, first-phase values, chain, records, writeback
        if (n_evals != 1 || !a->base_by_pos || a->base1 || !a->emit || !a->emit_out || items > 4 ||
            a->count > pe_chain_fused_max_count() || (a->fold.feas && a->fold.ncls > pe::kFusedMaxClasses))
            return hipErrorInvalidValue;
        if (split) for (int k = 0; k < 2; k++) (void)hipEventRecord(split[k], st);
        if (items == 1) hipLaunchKernelGGL((pe::k_chain<1, true>), dim3(1), dim3(pe::kChainBlock), lds, st, *a, 1u);
        else hipLaunchKernelGGL((pe::k_chain<4, true>), dim3(1), dim3(pe::kChainBlock), lds, st, *a, 1u);
        if (split) for (int k = 2; k < 5; k++) (void)hipEventRecord(split[k], st);
        return hipGetLastError();
    }
    const uint32_t m = a->base_by_pos ? a->n_visit : a->soa.n;
    uint32_t blocks = ((a->base1 ? 2u * m : m) + pe::kBaseBlock - 1) / pe::kBaseBlock;
    if (blocks > 8192) blocks = 8192;
    if (blocks == 0) blocks = 1;
    if (split) (void)hipEventRecord(split[0], st);
    if (wd.bits) {
        if (a->fold.feas) hipLaunchKernelGGL((pe::k_base<true, true>), dim3(blocks), dim3(pe::kBaseBlock), 0, st, *a);
        else hipLaunchKernelGGL((pe::k_base<false, true>), dim3(blocks), dim3(pe::kBaseBlock), 0, st, *a);
    } else if (a->fold.feas) {
        hipLaunchKernelGGL(pe::k_base<true>, dim3(blocks), dim3(pe::kBaseBlock), 0, st, *a);
    } else {
        hipLaunchKernelGGL(pe::k_base<false>, dim3(blocks), dim3(pe::kBaseBlock), 0, st, *a);
    }
    if (split) (void)hipEventRecord(split[1], st);
    if (wd.bits && wide_one) {
        // both rotations in one workgroup, the options compacted by rank in LDS
        if (!pe_chain_one_fits(a->n_visit, a->count, a->limit)) return hipErrorInvalidValue;
        static bool attr[64];   // per device: the attribute is set on the current device's function
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
        if (!attr[dev]) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&pe::k_phases),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)pe_chain_one_max_dyn());
            if (e != hipSuccess) return e;
            attr[dev] = true;
        }
        hipLaunchKernelGGL(pe::k_phases, dim3(1), dim3(pe::kOneBlock),
                           pe_chain_one_lds_bytes(a->n_visit, a->count, a->limit), st, *a);
    } else if (wd.bits) {
        // one Select per lane; the second rotation only when the count reaches it
        const uint32_t wg = (a->count + pe::kWideBlock - 1) / pe::kWideBlock;
        for (uint32_t ph = 0; ph < wd.phases; ph++)
            hipLaunchKernelGGL(pe::k_phase, dim3(wg ? wg : 1), dim3(pe::kWideBlock), 0, st, *a, ph);
    }
    if (wd.bits) {
        // an armed launch runs the instantiation that starts from the seed
        // (the shape was checked above: no other one can take its place)
        switch (items) {
        case 1: hipLaunchKernelGGL((pe::k_chain<1, false, true>), dim3(1), dim3(pe::kChainBlock), lds, st, *a, 1u); break;
        case 4: hipLaunchKernelGGL((pe::k_chain<4, false, true>), dim3(1), dim3(pe::kChainBlock), lds, st, *a, 1u); break;
        default:
            hipLaunchKernelGGL((pe::k_chain<pe::kChainItems, false, true>), dim3(1), dim3(pe::kChainBlock), lds, st, *a,
                               1u);
        }
    } else {
        switch (items) {
        case 1: hipLaunchKernelGGL((pe::k_chain<1, false>), dim3(grid), dim3(pe::kChainBlock), lds, st, *a, n_evals); break;
        case 4: hipLaunchKernelGGL((pe::k_chain<4, false>), dim3(grid), dim3(pe::kChainBlock), lds, st, *a, n_evals); break;
        default:
            hipLaunchKernelGGL((pe::k_chain<pe::kChainItems, false>), dim3(grid), dim3(pe::kChainBlock), lds, st, *a,
                               n_evals);
        }
    }
    if (split) (void)hipEventRecord(split[2], st);
    if (a->emit) {
        if (n_evals != 1 || !a->emit_out || !a->emit_ov || !a->emit_n) return hipErrorInvalidValue;
        hipLaunchKernelGGL(pe::k_emit, dim3(pe_emit_grid(a->count)), dim3(pe::kEmitBlock), 0, st, *a);
        if (split) (void)hipEventRecord(split[3], st);
        const uint32_t wb = (a->count + 255) / 256;   // overlay rows <= placements
        hipLaunchKernelGGL(pe::k_emit_writeback, dim3(wb ? wb : 1), dim3(256), 0, st, *a);
    } else if (split) {
        (void)hipEventRecord(split[3], st);
    }
    if (split) (void)hipEventRecord(split[4], st);
    return hipGetLastError();
}

hipError_t pe_launch_rank_of(const uint32_t* list, uint32_t n_list, uint32_t* rank_of, uint32_t n_rows, hipStream_t st) {
    hipError_t e = hipMemsetAsync(rank_of, 0xFF, sizeof(uint32_t) * (size_t)n_rows, st);
    if (e != hipSuccess || !n_list) return e;
    hipLaunchKernelGGL(pe::k_rank_of, dim3((n_list + 255) / 256), dim3(256), 0, st, list, n_list, rank_of);
    return hipGetLastError();
}

hipError_t pe_launch_system(const pe::SystemArgs* a, hipStream_t st) {
    if (a->rank_of && a->res) {   // row order: coalesced evaluation, then the list-order gather
        uint32_t b1 = (a->n_rows + 255) / 256;
        if (b1 > 8192) b1 = 8192;
        if (b1 == 0) b1 = 1;
        hipLaunchKernelGGL(pe::k_system_rows, dim3(b1), dim3(256), 0, st, *a);   // outcomes by row into res
        if (a->n_list)
            hipLaunchKernelGGL(pe::k_system_gather, dim3((a->n_list + 255) / 256), dim3(256), 0, st, a->list,
                               a->n_list, a->res, a->out_score, a->out_status);
        return hipGetLastError();
    }
    uint32_t blocks = (a->n_list + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(pe::k_system, dim3(blocks), dim3(256), 0, st, *a);
    return hipGetLastError();
}

// The code columns of pe_inplace_update_csi come with their set index and span the snapshot's rows.
static bool inplace_csi_args_ok(const pe::InplaceArgs* a) {
    return !a->csi_codes || (a->csi_set && a->csi_rows == a->soa.n);
}

// `m` (or null): the metrics form (pe_inplace_update_metrics with AllocMetric on).
hipError_t pe_launch_inplace(const pe::InplaceArgs* a, const pe::InplaceMetricsArgs* m, hipStream_t st) {
    if (!a->n_groups) return hipSuccess;
    if (!inplace_csi_args_ok(a)) return hipErrorInvalidValue;
    uint32_t blocks = (a->n_groups + 255) / 256;
    if (blocks > 2048) blocks = 2048;   // grid-stride beyond
    const pe::InplaceStopArgs none{nullptr, nullptr, nullptr, nullptr};
    const pe::InplaceMetricsArgs nom{nullptr, nullptr};
    if (m && (!m->code || !m->named)) return hipErrorInvalidValue;
    if (a->csi_codes) {   // pe_inplace_update_csi
        if (m) hipLaunchKernelGGL((pe::k_inplace<false, true, true>), dim3(blocks), dim3(256), 0, st, *a, none, *m);
        else hipLaunchKernelGGL((pe::k_inplace<false, false, true>), dim3(blocks), dim3(256), 0, st, *a, none, nom);
    } else if (m) {
        hipLaunchKernelGGL((pe::k_inplace<false, true, false>), dim3(blocks), dim3(256), 0, st, *a, none, *m);
    } else {
        hipLaunchKernelGGL((pe::k_inplace<false, false, false>), dim3(blocks), dim3(256), 0, st, *a, none, nom);
    }
    return hipGetLastError();
}

// The stopping form (a preempting system stack): *s->n_stopped is zero before.
hipError_t pe_launch_inplace_stop(const pe::InplaceArgs* a, const pe::InplaceStopArgs* s,
                                  const pe::InplaceMetricsArgs* m, hipStream_t st) {
    if (!a->n_groups) return hipSuccess;
    if (!s->resume || !s->stopped || !s->n_stopped || !s->own_existing) return hipErrorInvalidValue;
    if (m && (!m->code || !m->named)) return hipErrorInvalidValue;
    if (!inplace_csi_args_ok(a)) return hipErrorInvalidValue;
    uint32_t blocks = (a->n_groups + 255) / 256;
    if (blocks > 2048) blocks = 2048;   // grid-stride beyond
    const pe::InplaceMetricsArgs nom{nullptr, nullptr};
    if (a->csi_codes) {   // pe_inplace_update_csi
        if (m) hipLaunchKernelGGL((pe::k_inplace<true, true, true>), dim3(blocks), dim3(256), 0, st, *a, *s, *m);
        else hipLaunchKernelGGL((pe::k_inplace<true, false, true>), dim3(blocks), dim3(256), 0, st, *a, *s, nom);
    } else if (m) {
        hipLaunchKernelGGL((pe::k_inplace<true, true, false>), dim3(blocks), dim3(256), 0, st, *a, *s, *m);
    } else {
        hipLaunchKernelGGL((pe::k_inplace<true, false, false>), dim3(blocks), dim3(256), 0, st, *a, *s, nom);
    }
    return hipGetLastError();
}

// pe_inplace_update_spread's second stage behind pe_launch_inplace on the same
// stream: the chunks' histograms, their scan, then the spread parts.
hipError_t pe_launch_inplace_spread(const pe::InplaceSpreadArgs* a, hipStream_t st) {
    if (!a->n || a->tg.n_spread <= 0) return hipSuccess;
    const uint32_t cols = a->tg.pset_cnt_total;
    if (a->tg.n_psets != a->tg.n_spread || a->n_chunks != (a->n + pe::kInplaceSpreadChunk - 1) / pe::kInplaceSpreadChunk ||
        !a->status || !a->val || !a->own || !a->rec || (cols && (!a->ep0 || !a->craw0 || !a->prop0 || !a->pre)))
        return hipErrorInvalidValue;
    if (cols) {
        const hipError_t e = hipMemsetAsync(a->pre, 0, sizeof(uint32_t) * 2 * (size_t)cols * a->n_chunks, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(pe::k_inplace_spread_hist, dim3(a->n_chunks), dim3(pe::kInplaceSpreadChunk), 0, st, *a);
        uint32_t blocks = (2 * cols + 255) / 256;
        if (blocks > 1024) blocks = 1024;   // grid-stride beyond
        hipLaunchKernelGGL(pe::k_inplace_spread_scan, dim3(blocks), dim3(256), 0, st, *a);
    }
    hipLaunchKernelGGL(pe::k_inplace_spread, dim3(a->n_chunks), dim3(256), 0, st, *a);
    return hipGetLastError();
}

static bool sysg_metrics_ok(const pe::SysMetricsArgs& m, const pe::SystemGroupsArgs& a) {
    return m.first && (m.dev_group < 0 || m.dev_named) && m.dev_group < (int32_t)a.n_tg && m.n_list == a.n_list;
}

// The chunked walk: one launch per chunk of kSysGroupsChunk listed groups, in
// list order on the stream (a later chunk's lanes read what the earlier
// chunk's stored, and skip the lanes it stopped). `s` set: the stopping form;
// `m` set: the AllocMetric form.
hipError_t pe_launch_system_groups(const pe::SystemGroupsArgs* a, const pe::SysStopArgs* s,
                                   const pe::SysMetricsArgs* m, hipStream_t st) {
    const uint32_t span = a->rank_of ? a->n_rows : a->n_list;
    if (!span || !a->n_tg) return hipSuccess;
    if (s && (!s->resume || !s->stopped || !s->n_stopped)) return hipErrorInvalidValue;
    if (m && !sysg_metrics_ok(*m, *a)) return hipErrorInvalidValue;
    uint32_t blocks = (span + 255) / 256;
    if (blocks > 8192) blocks = 8192;   // grid-stride beyond
    auto* kernel = s ? (m ? pe::k_system_groups<true, true> : pe::k_system_groups<true, false>)
                     : (m ? pe::k_system_groups<false, true> : pe::k_system_groups<false, false>);
    const pe::SysStopArgs sv = s ? *s : pe::SysStopArgs{nullptr, nullptr, nullptr};
    const pe::SysMetricsArgs mv = m ? *m : pe::SysMetricsArgs{nullptr, -1, 0u, nullptr};
    pe::SystemGroupsArgs c = *a;
    for (uint32_t k0 = 0; k0 < a->n_tg; k0 += pe::kSysGroupsChunk) {
        c.k0 = k0;
        c.nk = a->n_tg - k0 < pe::kSysGroupsChunk ? a->n_tg - k0 : pe::kSysGroupsChunk;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, c, sv, mv);
    }
    return hipGetLastError();
}

// The eviction walk at width `words` over the lanes listed in a->stopped
// (their count is read on the device; at most `max_lanes`); `metrics`: its
// AllocMetric form, which fills a->M.
hipError_t pe_launch_system_groups_evict(const pe::SysEvictArgs* a, uint32_t words, uint32_t max_lanes, bool metrics,
                                         hipStream_t st) {
    if (!max_lanes || !a->G.n_tg) return hipSuccess;
    if (!a->pre || !a->resume || !a->stopped || !a->n_stopped || !a->wider || !a->n_wider || !a->app || !a->n_app ||
        !a->flags || !a->preempted || !a->pcount || !a->dev_free_all)
        return hipErrorInvalidValue;
    if (metrics && !sysg_metrics_ok(a->M, a->G)) return hipErrorInvalidValue;
    uint32_t blocks = (max_lanes + 255) / 256;
    if (blocks > 1024) blocks = 1024;   // grid-stride beyond
    void (*kernel)(pe::SysEvictArgs) = nullptr;
    if (words == 1u) kernel = metrics ? pe::k_system_groups_evict<1, true> : pe::k_system_groups_evict<1>;
    else if (words == 8u) kernel = metrics ? pe::k_system_groups_evict<8, true> : pe::k_system_groups_evict<8>;
    else if (words == 32u) kernel = metrics ? pe::k_system_groups_evict<32, true> : pe::k_system_groups_evict<32>;
    else return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, *a);
    return hipGetLastError();
}

// Pack, scan, scatter: ordered across workgroups by the kernel boundaries only.
hipError_t pe_launch_system_compact(const pe::SysCompactArgs* a, hipStream_t st) {
    if (!a->n_entries || a->n_tiles != (a->n_entries + pe::kSysTile - 1) / pe::kSysTile) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pe::k_sysg_pack, dim3(a->n_tiles), dim3(256), 0, st, *a);
    hipLaunchKernelGGL(pe::k_sysg_scan, dim3(1), dim3(256), 0, st, *a);
    hipLaunchKernelGGL(pe::k_sysg_scatter, dim3(a->n_tiles), dim3(256), 0, st, *a);
    return hipGetLastError();
}

hipError_t pe_launch_commit(const pe::NodeSoA* s, const pe::TgTables* t, const pe::Ask* a, uint32_t row,
                            uint32_t offers, hipStream_t st) {
    hipLaunchKernelGGL(pe::k_commit, dim3(1), dim3(64), 0, st, *s, *t, *a, row, offers);
    return hipGetLastError();
}

hipError_t pe_launch_apply_commits(const pe::NodeSoA* s, const pe::TgTables* t, const pe::Ask* a, const uint32_t* rows,
                                   const uint32_t* offers, uint32_t n, int sign, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(pe::k_apply_commits, dim3((n + 255) / 256), dim3(256), 0, st, *s, *t, *a, rows, offers, n, sign);
    return hipGetLastError();
}

// Select with Preempt: per-position evict evaluation, then the window resolve.
hipError_t pe_launch_resolve(const pe::EvictResolveArgs* r, hipStream_t st) {
    hipLaunchKernelGGL(pe::k_evict_resolve, dim3(1), dim3(pe::kResolveBlock), 0, st, *r);
    return hipGetLastError();
}

// Eviction widths (evict.inc): W = 1 (<= 32 allocs per node), 8 (<= 256) or
// 32 (<= 1024 allocs, ProposedAllocs <= 2048). A wide launch keeps its
// per-lane lists in scratch (lane-interleaved, so the lanes' accesses to one
// list element coalesce; W = 32 is ~19 KB per lane): the grid is capped lower
// so that the scratch reservation stays small (32 x 256 lanes: ~150 MB).
static inline bool evict_width_ok(uint32_t w) { return w == 1u || w == 8u || w == 32u; }
static inline uint32_t evict_blocks(uint32_t n, uint32_t w) {
    uint32_t blocks = (n + 255) / 256;
    const uint32_t cap = w == 1u ? 2048u : w == 8u ? 256u : 32u;
    if (blocks > cap) blocks = cap;
    return blocks ? blocks : 1u;
}

// The eviction walk of pe_inplace_update_preempt at width `words` over the
// groups listed in a->stopped (their count is read on the device; at most
// `max_groups`).
hipError_t pe_launch_inplace_evict(const pe::InplaceEvictArgs* a, const pe::InplaceMetricsArgs* m, uint32_t words,
                                   uint32_t max_groups, hipStream_t st) {
    if (!max_groups) return hipSuccess;
    if (!evict_width_ok(words) || !a->own_existing || !a->resume || !a->stopped || !a->n_stopped || !a->wider ||
        !a->n_wider || !a->app || !a->n_app || !a->flags || !a->I.status || !a->I.preempted || !a->I.allocs)
        return hipErrorInvalidValue;
    if (m && (!m->code || !m->named)) return hipErrorInvalidValue;
    if (!inplace_csi_args_ok(&a->I)) return hipErrorInvalidValue;
    const uint32_t blocks = evict_blocks(max_groups, words);
    const pe::InplaceMetricsArgs none{nullptr, nullptr};
    const pe::InplaceMetricsArgs& ma = m ? *m : none;
#define PE_INPLACE_EVICT(W, MET, CSI) \
    hipLaunchKernelGGL((pe::k_inplace_evict<W, MET, CSI>), dim3(blocks), dim3(256), 0, st, *a, ma)
    if (a->I.csi_codes) {   // pe_inplace_update_csi
        if (m) {
            if (words == 1u) PE_INPLACE_EVICT(1, true, true);
            else if (words == 8u) PE_INPLACE_EVICT(8, true, true);
            else PE_INPLACE_EVICT(32, true, true);
        } else {
            if (words == 1u) PE_INPLACE_EVICT(1, false, true);
            else if (words == 8u) PE_INPLACE_EVICT(8, false, true);
            else PE_INPLACE_EVICT(32, false, true);
        }
    } else if (m) {
        if (words == 1u) PE_INPLACE_EVICT(1, true, false);
        else if (words == 8u) PE_INPLACE_EVICT(8, true, false);
        else PE_INPLACE_EVICT(32, true, false);
    } else {
        if (words == 1u) PE_INPLACE_EVICT(1, false, false);
        else if (words == 8u) PE_INPLACE_EVICT(8, false, false);
        else PE_INPLACE_EVICT(32, false, false);
    }
#undef PE_INPLACE_EVICT
    return hipGetLastError();
}

hipError_t pe_launch_evict(const pe::PreemptArgs* a, const pe::EvictResolveArgs* r, hipStream_t st) {
    if (!evict_width_ok(a->mask_words)) return hipErrorInvalidValue;
    const uint32_t blocks = evict_blocks(a->n_visit, a->mask_words);
    if (a->mask_words == 1u) hipLaunchKernelGGL((pe::k_evict<false, 1>), dim3(blocks), dim3(256), 0, st, *a);
    else if (a->mask_words == 8u) hipLaunchKernelGGL((pe::k_evict<false, 8>), dim3(blocks), dim3(256), 0, st, *a);
    else hipLaunchKernelGGL((pe::k_evict<false, 32>), dim3(blocks), dim3(256), 0, st, *a);
    hipLaunchKernelGGL(pe::k_evict_resolve, dim3(1), dim3(pe::kResolveBlock), 0, st, *r);
    return hipGetLastError();
}

hipError_t pe_launch_census(const pe::BatchArgs* a, uint32_t* counts, uint8_t* status, double* score,
                            hipStream_t st, double* parts, uint8_t* nparts) {
    uint32_t blocks = (a->n_visit + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks == 0) blocks = 1;
    if (parts) {
        if (!nparts || !status) return hipErrorInvalidValue;
        hipLaunchKernelGGL(pe::k_census<true>, dim3(blocks), dim3(256), 0, st, *a, counts, status, score, parts, nparts);
    } else {
        hipLaunchKernelGGL(pe::k_census<false>, dim3(blocks), dim3(256), 0, st, *a, counts, status, score, parts,
                           nparts);
    }
    return hipGetLastError();
}

hipError_t pe_launch_evict_only(const pe::PreemptArgs* a, hipStream_t st) {
    if (!evict_width_ok(a->mask_words)) return hipErrorInvalidValue;
    const uint32_t blocks = evict_blocks(a->n_visit, a->mask_words);
    const uint32_t w = a->mask_words;
    if (a->parts_out) {
        if (!a->nparts_out || !a->mask_out || !a->offers_out) return hipErrorInvalidValue;
        if (w == 1u) hipLaunchKernelGGL((pe::k_evict<true, 1>), dim3(blocks), dim3(256), 0, st, *a);
        else if (w == 8u) hipLaunchKernelGGL((pe::k_evict<true, 8>), dim3(blocks), dim3(256), 0, st, *a);
        else hipLaunchKernelGGL((pe::k_evict<true, 32>), dim3(blocks), dim3(256), 0, st, *a);
    } else {
        if (w == 1u) hipLaunchKernelGGL((pe::k_evict<false, 1>), dim3(blocks), dim3(256), 0, st, *a);
        else if (w == 8u) hipLaunchKernelGGL((pe::k_evict<false, 8>), dim3(blocks), dim3(256), 0, st, *a);
        else hipLaunchKernelGGL((pe::k_evict<false, 32>), dim3(blocks), dim3(256), 0, st, *a);
    }
    return hipGetLastError();
}

// mask: mask_words + 1 words (the preempted set, then the kEvict* flags)
hipError_t pe_launch_evict_record(const pe::PreemptArgs* a, uint32_t row, pe_ranked_node* out, uint32_t* mask,
                                  hipStream_t st) {
    if (!evict_width_ok(a->mask_words)) return hipErrorInvalidValue;
    if (a->mask_words == 1u) hipLaunchKernelGGL(pe::k_evict_record<1>, dim3(1), dim3(64), 0, st, *a, row, out, mask);
    else if (a->mask_words == 8u) hipLaunchKernelGGL(pe::k_evict_record<8>, dim3(1), dim3(64), 0, st, *a, row, out, mask);
    else hipLaunchKernelGGL(pe::k_evict_record<32>, dim3(1), dim3(64), 0, st, *a, row, out, mask);
    return hipGetLastError();
}

hipError_t pe_launch_commit_evicted(const pe::PreemptArgs* a, uint8_t* preempted, uint32_t* pcount,
                                    uint32_t* dev_free, uint32_t* placed, hipStream_t st) {
    if (!evict_width_ok(a->mask_words)) return hipErrorInvalidValue;
    uint32_t blocks = (a->n_visit + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks == 0) blocks = 1;
    if (a->mask_words == 1u)
        hipLaunchKernelGGL(pe::k_commit_evicted<1>, dim3(blocks), dim3(256), 0, st, *a, preempted, pcount, dev_free,
                           placed);
    else if (a->mask_words == 8u)
        hipLaunchKernelGGL(pe::k_commit_evicted<8>, dim3(blocks), dim3(256), 0, st, *a, preempted, pcount, dev_free,
                           placed);
    else
        hipLaunchKernelGGL(pe::k_commit_evicted<32>, dim3(blocks), dim3(256), 0, st, *a, preempted, pcount, dev_free,
                           placed);
    return hipGetLastError();
}

// mask: mask_words words in device memory
hipError_t pe_launch_commit_preempt(const pe::PreemptArgs* a, uint32_t row, const uint32_t* mask, uint8_t* preempted,
                                    uint32_t* pcount, uint32_t* dev_free, hipStream_t st) {
    if (!evict_width_ok(a->mask_words)) return hipErrorInvalidValue;
    if (a->mask_words == 1u)
        hipLaunchKernelGGL(pe::k_commit_preempt<1>, dim3(1), dim3(64), 0, st, *a, row, mask, preempted, pcount,
                           dev_free);
    else if (a->mask_words == 8u)
        hipLaunchKernelGGL(pe::k_commit_preempt<8>, dim3(1), dim3(64), 0, st, *a, row, mask, preempted, pcount,
                           dev_free);
    else
        hipLaunchKernelGGL(pe::k_commit_preempt<32>, dim3(1), dim3(64), 0, st, *a, row, mask, preempted, pcount,
                           dev_free);
    return hipGetLastError();
}

hipError_t pe_launch_upload(void* dst, const void* src_mapped, size_t bytes, hipStream_t st) {
    if (!bytes) return hipSuccess;
    if (((uintptr_t)dst | (uintptr_t)src_mapped) & 15) return hipErrorInvalidValue;
    size_t blocks = (bytes / 16 + 255) / 256;
    if (blocks > 256) blocks = 256;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(pe::k_upload, dim3((uint32_t)blocks), dim3(256), 0, st, static_cast<unsigned char*>(dst),
                       static_cast<const unsigned char*>(src_mapped), bytes);
    return hipGetLastError();
}

hipError_t pe_launch_scatter_rows(void* dst, uint32_t words, const void* payload_mapped, uint32_t n, hipStream_t st) {
    if (!n || !words) return hipSuccess;
    if (((uintptr_t)dst | (uintptr_t)payload_mapped) & 3) return hipErrorInvalidValue;
    uint64_t blocks = ((uint64_t)n * words + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(pe::k_scatter_rows, dim3((uint32_t)blocks), dim3(256), 0, st, static_cast<uint32_t*>(dst), words,
                       static_cast<const uint32_t*>(payload_mapped), n);
    return hipGetLastError();
}

hipError_t pe_launch_counts(const pe::CountDsts* d, uint32_t nd, uint32_t n, const uint2* ents, uint32_t m,
                            const pe::ResetArgs* r, hipStream_t st) {
    if (nd > (uint32_t)pe::kMaxCountDst || (m && !ents) || n >= (1u << 27)) return hipErrorInvalidValue;
    pe::ResetArgs R;
    std::memset(&R, 0, sizeof(R));
    if (r && r->rec) {
        if (!r->base_rec || !r->dev_free || !r->dev_free_base || (r->m && !r->preempted) || (r->keys && !r->pcount))
            return hipErrorInvalidValue;
        R = *r;
    }
    const uint32_t span = std::max(n, std::max(R.n, std::max(R.m, R.keys)));
    if (!span) return hipSuccess;
    uint32_t blocks = (span + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(pe::k_counts, dim3(blocks), dim3(256), 0, st, *d, nd, n, ents, m, R);
    return hipGetLastError();
}

hipError_t pe_launch_plan_stop(pe::NodeRec* rec, uint32_t* dev_free, const pe::PreemptAlloc* allocs,
                               uint8_t* preempted, const uint32_t* slots, const uint32_t* rows, uint32_t n, int sign,
                               uint64_t* core_used, const uint64_t* palloc_cores, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(pe::k_plan_stop, dim3((n + 63) / 64), dim3(64), 0, st, rec, dev_free, allocs, preempted, slots,
                       rows, n, sign, core_used, palloc_cores);
    return hipGetLastError();
}

hipError_t pe_launch_evict_trace(const pe::PreemptArgs* a, const uint32_t* rows, uint32_t n, uint32_t* code,
                                 double* named, hipStream_t st) {
    if (!n) return hipSuccess;
    if (!evict_width_ok(a->mask_words)) return hipErrorInvalidValue;
    if (a->mask_words == 1u)
        hipLaunchKernelGGL(pe::k_evict_trace<1>, dim3((n + 63) / 64), dim3(64), 0, st, *a, rows, n, code, named);
    else if (a->mask_words == 8u)
        hipLaunchKernelGGL(pe::k_evict_trace<8>, dim3((n + 63) / 64), dim3(64), 0, st, *a, rows, n, code, named);
    else
        hipLaunchKernelGGL(pe::k_evict_trace<32>, dim3((n + 63) / 64), dim3(64), 0, st, *a, rows, n, code, named);
    return hipGetLastError();
}

hipError_t pe_launch_commit_rows(const pe::NodeSoA* s, const pe::TgTables* t, const pe::Ask* a, const uint32_t* rows,
                                 uint32_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(pe::k_commit_rows, dim3((n + 255) / 256), dim3(256), 0, st, *s, *t, *a, rows, n);
    return hipGetLastError();
}

hipError_t pe_launch_reset_plan(pe::NodeRec* rec, const pe::NodeRec* base_rec, uint32_t* dev_free,
                                const uint32_t* dev_free_base, uint32_t n, uint8_t* preempted, uint32_t m,
                                uint32_t* pcount, uint32_t keys, hipStream_t st) {
    uint32_t w = n > m ? n : m;
    w = w > keys ? w : keys;
    uint32_t blocks = (w + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(pe::k_reset_plan, dim3(blocks), dim3(256), 0, st, rec, base_rec, dev_free, dev_free_base, n,
                       preempted, m, pcount, keys);
    return hipGetLastError();
}

hipError_t pe_launch_fold_feas(const pe::NodeSoA* s, const uint8_t* class_ok, const uint8_t* node_ok, uint8_t* feas,
                               hipStream_t st) {
    uint32_t blocks = (s->n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(pe::k_fold_feas, dim3(blocks), dim3(256), 0, st, *s, class_ok, node_ok, feas);
    return hipGetLastError();
}

hipError_t pe_launch_csi_avail(const pe::CsiArgs* a, hipStream_t st) {
    if (a->n_req > (uint32_t)pe::kMaxCsiReq || !a->plug_off || !a->nvol_off || !a->rec || !a->class_ok || !a->codes ||
        !a->node_ok || !a->node_feas)
        return hipErrorInvalidValue;
    uint32_t blocks = (a->n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(pe::k_csi_avail, dim3(blocks), dim3(256), 0, st, *a);
    return hipGetLastError();
}

// The codes alone into a column of pe_place_csi (CsiArgs::node_ok and node_feas null).
hipError_t pe_launch_csi_codes(const pe::CsiArgs* a, hipStream_t st) {
    if (a->n_req > (uint32_t)pe::kMaxCsiReq || !a->plug_off || !a->nvol_off || !a->codes || a->node_ok || a->node_feas)
        return hipErrorInvalidValue;
    uint32_t blocks = (a->n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(pe::k_csi_avail, dim3(blocks), dim3(256), 0, st, *a);
    return hipGetLastError();
}

hipError_t pe_launch_csi_first(const pe::BatchArgs* a, const pe::CsiLoopArgs* c, hipStream_t st) {
    if (!a->perms || !a->soa.rec || !c->cls_state || !c->first || a->n_visit == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pe::k_csi_first, dim3((a->n_visit + 255u) / 256u), dim3(256), 0, st, a->perms, a->n_visit,
                       a->offset0 % a->n_visit, a->soa.rec, *c);
    return hipGetLastError();
}

// One evaluation, one wave; the overlay must hold the launch's placements.
hipError_t pe_launch_csi_loop(const pe::BatchArgs* a, const pe::CsiLoopArgs* c, hipStream_t st, uint8_t* log,
                              uint32_t log_cap) {
    if (!a->perms || a->n_visit == 0 || !a->full_out || !a->eval_status || !c->codes || !c->set_of || !c->cls_state ||
        !c->first || c->n_sets == 0 || c->n_sets > (uint32_t)pe::kMaxCsiSets || c->n_rows != a->soa.n ||
        a->tg.node_feas || a->hash_bits < 0 || a->hash_bits > 30 ||
        ((uint64_t)1 << a->hash_bits) < 2ull * a->count)
        return hipErrorInvalidValue;
    if (a->ask.n_dev > 0 && (!a->tg.dev_cls || !a->tg.dev_free)) return hipErrorInvalidValue;   // a device ask reads both
    // the trace log holds every position the call can consume (a Select consumes at most n_visit)
    if (log && ((uint64_t)a->count * a->n_visit > (uint64_t)log_cap || (uint64_t)log_cap > pe::kCsiLogCap))
        return hipErrorInvalidValue;
    const size_t lds = pe_place_lds_bytes(false, a->hash_bits, a->packed_overlay != 0, 0);
    if (log) hipLaunchKernelGGL(pe::k_csi_loop<true>, dim3(1), dim3(64), lds, st, *a, *c, log, log_cap);
    else hipLaunchKernelGGL(pe::k_csi_loop<false>, dim3(1), dim3(64), lds, st, *a, *c, (uint8_t*)nullptr, 0u);
    return hipGetLastError();
}

// One evaluation, one wave; the overlay must hold the launch's placements, the
// stop list kDsWords words per update.
hipError_t pe_launch_destructive(const pe::BatchArgs* a, const pe::DestructiveArgs* d, hipStream_t st) {
    if (!a->perms || a->n_visit == 0 || !a->full_out || !a->eval_status || !a->soa.rec || !a->soa.coll_job ||
        !a->tg.coll_tg || !d->stops || (d->n_slots && (!d->palloc || !d->preempted)) || a->hash_bits < 0 ||
        a->hash_bits > 30 ||
        ((uint64_t)1 << a->hash_bits) < 2ull * a->count || a->ask.cores > 0 || a->tg.n_psets != 0)
        return hipErrorInvalidValue;
    if (a->ask.n_dev > 0 && (!a->tg.dev_cls || !a->tg.dev_free)) return hipErrorInvalidValue;   // a device ask reads both
    const size_t lds = pe_place_lds_bytes(false, a->hash_bits, a->packed_overlay != 0, 0);
    hipLaunchKernelGGL(pe::k_destructive, dim3(1), dim3(64), lds, st, *a, *d);
    return hipGetLastError();
}

uint32_t pe_destructive_full_cap() { return pe::kDfCap; }

// One workgroup; dynamic LDS = 16 B per entry. cnt_log (or null): every update's use counts for the
// trace of its maps (k_destructive_full<*, true>), cnt_log_words >= count * pset_cnt_total words of device memory.
hipError_t pe_launch_destructive_full(const pe::SweepArgs* a, const pe::SweepArgs* a_dev, int np,
                                      const pe::DestructiveFullArgs* f, const uint32_t* visit, uint32_t n,
                                      uint32_t count, pe_ranked_node* out, uint32_t* state, hipStream_t st,
                                      uint32_t* cnt_log, size_t cnt_log_words) {
    const pe::DestructiveArgs& d = f->d;
    if (!a_dev || !visit || n == 0 || !out || !state || !a->soa.rec || !a->soa.coll_job || !a->tg.coll_tg ||
        !a->node_aux || !a->aff_vals || !d.stops || !f->named || (d.n_slots && (!d.palloc || !d.preempted)) ||
        a->ask.cores > 0 || np < 0 || np > pe::kAuxPsets || np != a->tg.n_psets || (np && !f->sp) ||
        a->tg.pset_cnt_total > (uint32_t)(pe::kAuxPsets * pe::kAuxValues) ||
        a->tg.pset_tab_total > (uint32_t)(pe::kAuxPsets * (pe::kAuxValues + 1)))
        return hipErrorInvalidValue;
    for (int p = 0; p < np; p++)
        if (a->tg.pset_nvals[p] > (int)pe::kAuxMissing ||
            a->tg.pset_cnt_off[p] + (uint32_t)a->tg.pset_nvals[p] > a->tg.pset_cnt_total ||
            a->tg.pset_tab_off[p] + (uint32_t)a->tg.pset_nvals[p] + 1u > a->tg.pset_tab_total)
            return hipErrorInvalidValue;
    if (a->ask.n_dev > 0 && (!a->tg.dev_cls || !a->tg.dev_free)) return hipErrorInvalidValue;   // a device ask reads both
    if (cnt_log && (uint64_t)count * a->tg.pset_cnt_total > (uint64_t)cnt_log_words) return hipErrorInvalidValue;
    const bool log = cnt_log && np > 0;   // no spread set: nothing to store, the plain form
    const size_t lds = (size_t)pe::kDfCap * (sizeof(double) + 2 * sizeof(uint32_t));
    // (the plain forms are named first here and below: they are instantiated first and keep their place in the code object)
    static bool attr = false;
    if (!attr) {
        for (const void* fn : {reinterpret_cast<const void*>(&pe::k_destructive_full<0, false>),
                               reinterpret_cast<const void*>(&pe::k_destructive_full<1, false>),
                               reinterpret_cast<const void*>(&pe::k_destructive_full<2, false>),
                               reinterpret_cast<const void*>(&pe::k_destructive_full<1, true>),
                               reinterpret_cast<const void*>(&pe::k_destructive_full<2, true>)}) {
            const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        attr = true;
    }
    uint32_t* const none = nullptr;
    switch (np) {
        case 0:
            hipLaunchKernelGGL((pe::k_destructive_full<0, false>), dim3(1), dim3(pe::kFullThreads), lds, st, a_dev, *f,
                               visit, n, count, out, state, none);
            break;
        case 1:
            if (!log)
                hipLaunchKernelGGL((pe::k_destructive_full<1, false>), dim3(1), dim3(pe::kFullThreads), lds, st, a_dev,
                                   *f, visit, n, count, out, state, none);
            else
                hipLaunchKernelGGL((pe::k_destructive_full<1, true>), dim3(1), dim3(pe::kFullThreads), lds, st, a_dev,
                                   *f, visit, n, count, out, state, cnt_log);
            break;
        default:
            if (!log)
                hipLaunchKernelGGL((pe::k_destructive_full<2, false>), dim3(1), dim3(pe::kFullThreads), lds, st, a_dev,
                                   *f, visit, n, count, out, state, none);
            else
                hipLaunchKernelGGL((pe::k_destructive_full<2, true>), dim3(1), dim3(pe::kFullThreads), lds, st, a_dev,
                                   *f, visit, n, count, out, state, cnt_log);
            break;
    }
    return hipGetLastError();
}

size_t pe_fold_feas_max_classes() { return pe::kFoldMaxClasses; }

hipError_t pe_launch_fold_feas_staged(const pe::NodeSoA* s, const unsigned char* class_src, uint8_t* class_dst,
                                      uint32_t ncls, const uint8_t* node_ok, uint8_t* feas, hipStream_t st) {
    if (ncls > pe::kFoldMaxClasses || !class_src || !class_dst) return hipErrorInvalidValue;
    uint32_t blocks = (s->n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(pe::k_fold_feas_staged, dim3(blocks), dim3(256), 0, st, *s, class_src, class_dst, ncls,
                       node_ok, feas);
    return hipGetLastError();
}

hipError_t pe_launch_fold_aux(const pe::NodeSoA* s, const pe::TgTables* t, const uint8_t* aff_idx_class,
                              const uint8_t* aff_idx_node, uint32_t* aux, hipStream_t st) {
    uint32_t blocks = (s->n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(pe::k_fold_aux, dim3(blocks), dim3(256), 0, st, *s, *t, aff_idx_class, aff_idx_node, aux);
    return hipGetLastError();
}

// k_sweep over `blocks` workgroups: the folded-aux form when the caller built node_aux.
static void launch_k_sweep(const pe::SweepArgs* a, uint32_t blocks, hipStream_t st) {
    if (a->node_aux) hipLaunchKernelGGL((pe::k_sweep<256, true>), dim3(blocks), dim3(256), 0, st, *a);
    else hipLaunchKernelGGL((pe::k_sweep<256, false>), dim3(blocks), dim3(256), 0, st, *a);
}

hipError_t pe_launch_sweep(const pe::SweepArgs* a, uint32_t blocks, pe::SweepRec* merged, hipStream_t st) {
    launch_k_sweep(a, blocks, st);
    hipLaunchKernelGGL(pe::k_sweep_merge, dim3(1), dim3(512), 0, st, (const pe::SweepRec*)a->recs, blocks, merged);
    return hipGetLastError();
}

hipError_t pe_launch_trace_top(const uint32_t* codes, const double* sc, const pe::TraceSrc* src, uint32_t flags,
                               pe_metric_score* out, uint8_t* n_out, hipStream_t st, uint32_t n_entries,
                               uint32_t* n_other, uint2* other_list) {
    if (!src->n_rec) return hipSuccess;
    // waves per record: about 2048 entries each, 1 to kTopWaves
    const uint32_t avg = n_entries / src->n_rec;
    const uint32_t waves = std::max<uint32_t>(1u, std::min<uint32_t>(pe::kTopWaves, (avg + 2047u) / 2048u));
    hipLaunchKernelGGL(pe::k_trace_top, dim3(src->n_rec), dim3(64 * waves), 0, st, codes, sc, *src, flags, out,
                       n_out, n_other, other_list);
    return hipGetLastError();
}

// A shard's sweep merged to one record (a->merged: the sharded count loop's
// exchange payload): k_sweep, then k_sweep_merge queued behind it.
hipError_t pe_launch_sweep_local(const pe::SweepArgs* a, uint32_t blocks, hipStream_t st) {
    if (!a->merged) return hipErrorInvalidValue;
    return pe_launch_sweep(a, blocks, a->merged, st);
}

// Resident k_sweep<256> workgroups per CU (grid = one full wave of residency).
int pe_sweep_blocks_per_cu(bool aux) {
    int nb = 0;
    const hipError_t e = aux ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, pe::k_sweep<256, true>, 256, 0)
                             : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, pe::k_sweep<256, false>, 256, 0);
    if (e != hipSuccess || nb <= 0) nb = 4;
    return nb;
}

hipError_t pe_launch_node_record(const pe::SweepArgs* a, uint32_t row, pe_ranked_node* out, hipStream_t st) {
    hipLaunchKernelGGL(pe::k_node_record, dim3(1), dim3(64), 0, st, *a, row, out);
    return hipGetLastError();
}

uint32_t pe_rec_winner(const pe::SweepRec* r) { return pe::rec_winner(*r); }
void pe_rec_init(pe::SweepRec* r) { pe::rec_init(*r); }
void pe_rec_merge(pe::SweepRec* a, const pe::SweepRec* b) { pe::rec_merge(*a, *b); }

hipError_t pe_launch_spread_table(const pe::TgTables* t, double* tab, hipStream_t st) {
    hipLaunchKernelGGL(pe::k_spread_table, dim3(1), dim3(256), 0, st, *t, tab);
    return hipGetLastError();
}

void pe_rec_merge_host(pe::SweepRec* a, const pe::SweepRec* b) { pe::rec_merge(*a, *b); }
void pe_rec_init_host(pe::SweepRec* a) { pe::rec_init(*a); }

hipError_t pe_launch_trace(const pe::NodeSoA* s, const pe::TgTables* t, const pe::Ask* a, const uint32_t* rows,
                           uint32_t n, uint32_t* out, const uint32_t* penalty_bits, double log10,
                           const double* spread_tab, double* scores, hipStream_t st, const uint16_t* dks) {
    if (n == 0) return hipSuccess;
    pe::TraceSrc src{};
    src.rows = rows;
    src.dks = dks;
    hipLaunchKernelGGL(pe::k_trace<false>, dim3((n + 255) / 256), dim3(256), 0, st, *s, *t, *a, src, n, out,
                       penalty_bits, log10, spread_tab, scores, pe::TraceStops{});
    return hipGetLastError();
}

// Every record of a speculative run in one launch (TraceSrc batched form).
hipError_t pe_launch_trace_batch(const pe::NodeSoA* s, const pe::TgTables* t, const pe::Ask* a,
                                 const pe::TraceSrc* src, uint32_t n, uint32_t* out, double log10,
                                 const double* spread_tab, double* scores, hipStream_t st,
                                 const pe::TraceStops* stops) {
    if (n == 0) return hipSuccess;
    if (stops)
        hipLaunchKernelGGL(pe::k_trace<true>, dim3((n + 255) / 256), dim3(256), 0, st, *s, *t, *a, *src, n, out,
                           nullptr, log10, spread_tab, scores, *stops);
    else
        hipLaunchKernelGGL(pe::k_trace<false>, dim3((n + 255) / 256), dim3(256), 0, st, *s, *t, *a, *src, n, out,
                           nullptr, log10, spread_tab, scores, pe::TraceStops{});
    return hipGetLastError();
}

// Spread boost tables of every record of a speculative run (k_spread_tables).
// absolute: `delta` holds every record's counts themselves (k_spread_tables<true>).
hipError_t pe_launch_spread_tables(const pe::TgTables* t, uint32_t n_rec, uint32_t* delta, double* tab,
                                   hipStream_t st, bool absolute) {
    if (n_rec == 0) return hipSuccess;
    if (!absolute)
        hipLaunchKernelGGL(pe::k_spread_tables<false>, dim3(n_rec), dim3(256), 0, st, *t, delta, tab);
    else
        hipLaunchKernelGGL(pe::k_spread_tables<true>, dim3(n_rec), dim3(256), 0, st, *t, delta, tab);
    return hipGetLastError();
}

// One placement of the device-resident count loop: k_sweep (no merge) over
// `blocks` workgroups, then k_sweep_step.
hipError_t pe_launch_sweep_step(const pe::SweepArgs* a, uint32_t blocks, const uint32_t* visit, uint32_t n,
                                uint32_t offset, pe_ranked_node* out, uint32_t* state, hipStream_t st) {
    launch_k_sweep(a, blocks, st);
    hipLaunchKernelGGL(pe::k_sweep_step, dim3(1), dim3(256), 0, st, *a, blocks, visit, n, offset, out, state);
    return hipGetLastError();
}

// The LDS-resident full-pass loop (one workgroup); dynamic LDS = 12 B per node.
size_t pe_fullpass_lds_bytes(uint32_t) { return (size_t)pe::kFullCap * (sizeof(double) + 2 * sizeof(uint32_t)); }

hipError_t pe_launch_fullpass_lds(const pe::SweepArgs* a_dev, int np, const uint32_t* visit, uint32_t n,
                                  uint32_t count, pe_ranked_node* out, uint32_t* state, unsigned long long* prof,
                                  hipStream_t st) {
    const size_t lds = pe_fullpass_lds_bytes(n);
    static bool attr = false;
    if (!attr) {
        for (const void* f : {reinterpret_cast<const void*>(&pe::k_fullpass_lds<0>),
                              reinterpret_cast<const void*>(&pe::k_fullpass_lds<1>),
                              reinterpret_cast<const void*>(&pe::k_fullpass_lds<2>)}) {
            const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)pe_fullpass_lds_bytes(0));
            if (e != hipSuccess) return e;
        }
        attr = true;
    }
    switch (np) {
        case 0:
            hipLaunchKernelGGL(pe::k_fullpass_lds<0>, dim3(1), dim3(pe::kFullThreads), lds, st, a_dev, visit, n, count,
                               out, state, prof);
            break;
        case 1:
            hipLaunchKernelGGL(pe::k_fullpass_lds<1>, dim3(1), dim3(pe::kFullThreads), lds, st, a_dev, visit, n, count,
                               out, state, prof);
            break;
        default:
            hipLaunchKernelGGL(pe::k_fullpass_lds<2>, dim3(1), dim3(pe::kFullThreads), lds, st, a_dev, visit, n, count,
                               out, state, prof);
            break;
    }
    return hipGetLastError();
}

size_t pe_fullpass_svc_bytes() { return (size_t)pe::kSvcCap * (2 * sizeof(double) + 4 * sizeof(uint32_t)); }
uint32_t pe_fullpass_svc_cap() { return pe::kSvcCap; }

hipError_t pe_launch_fullpass_svc(const pe::SweepArgs* a_dev, int np, bool lean, const uint32_t* visit, uint32_t n,
                                  uint32_t count, pe_ranked_node* out, uint32_t* state, hipStream_t st) {
    const size_t lds = pe_fullpass_svc_bytes();
    static bool attr = false;
    if (!attr) {
        for (const void* f : {reinterpret_cast<const void*>(&pe::k_fullpass_svc<0, false>),
                              reinterpret_cast<const void*>(&pe::k_fullpass_svc<1, false>),
                              reinterpret_cast<const void*>(&pe::k_fullpass_svc<2, false>),
                              reinterpret_cast<const void*>(&pe::k_fullpass_svc<0, true>),
                              reinterpret_cast<const void*>(&pe::k_fullpass_svc<1, true>),
                              reinterpret_cast<const void*>(&pe::k_fullpass_svc<2, true>)}) {
            const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        attr = true;
    }
#define PE_SVC_LAUNCH(NPV, L)                                                                                         \
    hipLaunchKernelGGL((pe::k_fullpass_svc<NPV, L>), dim3(1), dim3(pe::kFullThreads), lds, st, a_dev, visit, n, count, \
                       out, state)
    if (lean) {
        if (np == 0) PE_SVC_LAUNCH(0, true);
        else if (np == 1) PE_SVC_LAUNCH(1, true);
        else PE_SVC_LAUNCH(2, true);
    } else {
        if (np == 0) PE_SVC_LAUNCH(0, false);
        else if (np == 1) PE_SVC_LAUNCH(1, false);
        else PE_SVC_LAUNCH(2, false);
    }
#undef PE_SVC_LAUNCH
    return hipGetLastError();
}

// The sweep alone (per-workgroup records into a->recs, no merge).
hipError_t pe_launch_sweep_only(const pe::SweepArgs* a, uint32_t blocks, hipStream_t st) {
    launch_k_sweep(a, blocks, st);
    return hipGetLastError();
}

// The step alone (sharded loop: its records are the ranks' gathered ones).
hipError_t pe_launch_step_only(const pe::SweepArgs* a, uint32_t nrecs, const uint32_t* visit, uint32_t n,
                               uint32_t offset, pe_ranked_node* out, uint32_t* state, hipStream_t st) {
    hipLaunchKernelGGL(pe::k_sweep_step, dim3(1), dim3(256), 0, st, *a, nrecs, visit, n, offset, out, state);
    return hipGetLastError();
}

// Device-resident count loop over sparse options (one workgroup); dynamic LDS
// = 2 bits per position for each of the two outcome passes + 1 dependency bit,
// in what the workgroup's 160 KB leave beside the kernel's static LDS (which
// grows with the eviction width).
constexpr uint32_t kPLoopMaxN = 229376;
static size_t pe_ploop_lds_bytes(uint32_t n) { return (2u * ((n + 15u) / 16u) + (n + 31u) / 32u) * sizeof(uint32_t); }

static const void* ploop_fn(int wi) {
    return wi == 0 ? reinterpret_cast<const void*>(&pe::k_ploop<1>) : reinterpret_cast<const void*>(&pe::k_ploop<8>);
}

// The current device's LDS per workgroup (the opt-in limit where it reports
// one, else the default limit): 160 KB on gfx950.
static int lds_per_workgroup(int dev) {
    int optin = 0, dflt = 0;
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess) optin = 0;
    if (hipDeviceGetAttribute(&dflt, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) dflt = 0;
    (void)hipGetLastError();
    return std::max(optin, dflt);
}

// dynamic LDS bytes the launch may use on the current device (0: none / no
// device), cached per device
static int ploop_max_dyn(int wi) {
    constexpr int kDevs = 64;
    static int v[kDevs][2];
    static bool init[kDevs][2];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kDevs) {
        (void)hipGetLastError();
        return 0;
    }
    if (!init[dev][wi]) {
        hipFuncAttributes fa;
        if (hipFuncGetAttributes(&fa, ploop_fn(wi)) != hipSuccess) {
            (void)hipGetLastError();
            return 0;
        }
        const int d = lds_per_workgroup(dev) - (int)fa.sharedSizeBytes;
        v[dev][wi] = d > 0 ? d : 0;
        init[dev][wi] = true;
    }
    return v[dev][wi];
}

uint32_t pe_ploop_max_n(uint32_t words) {
    if (words != 1u && words != 8u) return 0;   // k_ploop<1> / <8> only (pe::kPLoopMaxWords)
    const size_t d = (size_t)ploop_max_dyn(words == 1u ? 0 : 1);
    uint32_t n = (uint32_t)std::min<size_t>(kPLoopMaxN, d * 8u / 5u) & ~31u;   // 5/8 byte per position
    while (n && pe_ploop_lds_bytes(n) > d) n -= 32u;
    return n;
}

hipError_t pe_launch_ploop(const pe::PLoopArgs* a, hipStream_t st) {
    const uint32_t n = a->P.n_visit;
    if (n == 0 || n > pe_ploop_max_n(a->P.mask_words)) return hipErrorInvalidValue;
    const int wi = a->P.mask_words == 1u ? 0 : 1;
    {   // per device: the attribute is set on the current device's function
        static bool attr[64][2];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
        if (!attr[dev][wi]) {
            const hipError_t e = hipFuncSetAttribute(ploop_fn(wi), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     ploop_max_dyn(wi));
            if (e != hipSuccess) return e;
            attr[dev][wi] = true;
        }
    }
    const size_t lds = pe_ploop_lds_bytes(n);
    if (wi == 0) hipLaunchKernelGGL(pe::k_ploop<1>, dim3(1), dim3(pe::kPLoopBlock), lds, st, *a);
    else hipLaunchKernelGGL(pe::k_ploop<8>, dim3(1), dim3(pe::kPLoopBlock), lds, st, *a);
    return hipGetLastError();
}

hipError_t pe_launch_static_gate(const uint8_t* blocked, const uint32_t* coll_tg, uint32_t* gate, uint32_t n,
                                 hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(pe::k_static_gate, dim3((n + 255) / 256), dim3(256), 0, st, blocked, coll_tg, gate, n);
    return hipGetLastError();
}

hipError_t pe_launch_md_gate(pe::MdNet* md, const uint32_t* coll_tg, uint32_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(pe::k_md_gate, dim3((n + 255) / 256), dim3(256), 0, st, md, coll_tg, n);
    return hipGetLastError();
}

// One workgroup; the overlay must hold the launch's placements. ev_score / ev_kind: n_visit entries each, the
// per-position classes and scores a placement's passes hand on (device memory, no contents expected).
uint32_t pe_csi_full_threads() { return pe::kCsiFullBlock; }

// log (or null): pe_place_csi_full_metrics' trace log (k_csi_full<*, true>), as pe_launch_csi_loop's.
hipError_t pe_launch_csi_full(const pe::BatchArgs* a, const pe::CsiLoopArgs* c, double* ev_score, uint8_t* ev_kind,
                              hipStream_t st, uint8_t* log, uint32_t log_cap) {
    if (!a->perms || a->n_visit == 0 || a->n_visit >= 0x7FFFFFFFu - (uint32_t)pe::kCsiFullBlock || !a->full_out ||
        !a->eval_status || !c->codes || !c->set_of || !c->cls_state || !c->first || c->n_sets == 0 ||
        c->n_sets > (uint32_t)pe::kMaxCsiSets || c->n_rows != a->soa.n || a->tg.node_feas || a->packed_overlay ||
        !ev_score || !ev_kind || a->hash_bits < 0 || a->hash_bits > 30 || ((uint64_t)1 << a->hash_bits) < 2ull * a->count)
        return hipErrorInvalidValue;
    if (a->ask.n_dev > 0 && (!a->tg.dev_cls || !a->tg.dev_free)) return hipErrorInvalidValue;   // a device ask reads both
    if (a->tg.n_psets > 0 && !a->pset_lds && (!a->pset_g_tab || !a->pset_g_cnt)) return hipErrorInvalidValue;
    // the trace log holds every position the call can consume (a Select consumes at most n_visit)
    if (log && ((uint64_t)a->count * a->n_visit > (uint64_t)log_cap || (uint64_t)log_cap > pe::kCsiLogCap))
        return hipErrorInvalidValue;
    const size_t lds = pe_place_lds_bytes(true, a->hash_bits, false, a->pset_lds);
    if (lds > 96u * 1024u) return hipErrorInvalidValue;   // (max_hash_bits' budget)
    static bool attr[2] = {false, false};   // per instantiation
    const int mi = log ? 1 : 0;
    if (!attr[mi] && lds > 32u * 1024u) {
        // (the plain form is named first here and below: it is instantiated first and keeps its place in the code object)
        const void* fn = !log ? reinterpret_cast<const void*>(&pe::k_csi_full<pe::kCsiFullBlock, false>)
                              : reinterpret_cast<const void*>(&pe::k_csi_full<pe::kCsiFullBlock, true>);
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        if (e != hipSuccess) return e;
        attr[mi] = true;
    }
    if (!log)
        hipLaunchKernelGGL((pe::k_csi_full<pe::kCsiFullBlock, false>), dim3(1), dim3(pe::kCsiFullBlock), lds, st, *a, *c,
                           ev_score, ev_kind, (uint8_t*)nullptr, 0u);
    else
        hipLaunchKernelGGL((pe::k_csi_full<pe::kCsiFullBlock, true>), dim3(1), dim3(pe::kCsiFullBlock), lds, st, *a, *c,
                           ev_score, ev_kind, log, log_cap);
    return hipGetLastError();
}
