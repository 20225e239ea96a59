// Host launchers of the engine's kernels: defined in kernels.hip, called from
// engine.cpp. Both include this header, so the compiler checks each definition
// against the one declaration, and the default arguments live here only.
#pragma once
#include <hip/hip_runtime.h>
#include "engine_types.h"

size_t pe_place_lds_bytes(bool full, int hash_bits, bool packed, size_t pset_bytes);
hipError_t pe_launch_place(const pe::BatchArgs* a, uint32_t n_evals, bool full, hipStream_t st);
hipError_t pe_launch_system(const pe::SystemArgs* a, hipStream_t st);
hipError_t pe_launch_inplace(const pe::InplaceArgs* a, const pe::InplaceMetricsArgs* m_or_null, hipStream_t st);
hipError_t pe_launch_inplace_stop(const pe::InplaceArgs* a, const pe::InplaceStopArgs* s,
                                  const pe::InplaceMetricsArgs* m_or_null, hipStream_t st);
hipError_t pe_launch_inplace_spread(const pe::InplaceSpreadArgs* a, hipStream_t st);
hipError_t pe_launch_inplace_evict(const pe::InplaceEvictArgs* a, const pe::InplaceMetricsArgs* m_or_null,
                                   uint32_t words, uint32_t max_groups, hipStream_t st);
hipError_t pe_launch_system_groups(const pe::SystemGroupsArgs* a, const pe::SysStopArgs* s_or_null,
                                   const pe::SysMetricsArgs* m_or_null, hipStream_t st);
hipError_t pe_launch_system_groups_evict(const pe::SysEvictArgs* a, uint32_t words, uint32_t max_lanes, bool metrics,
                                         hipStream_t st);
hipError_t pe_launch_system_compact(const pe::SysCompactArgs* a, hipStream_t st);
hipError_t pe_launch_rank_of(const uint32_t* list, uint32_t n_list, uint32_t* rank_of, uint32_t n_rows, hipStream_t st);
hipError_t pe_launch_upload(void* dst, const void* src_mapped, size_t bytes, hipStream_t st);
hipError_t pe_launch_scatter_rows(void* dst, uint32_t words, const void* payload_mapped, uint32_t n, hipStream_t st);
hipError_t pe_launch_counts(const pe::CountDsts* d, uint32_t nd, uint32_t n, const uint2* ents, uint32_t m,
                            const pe::ResetArgs* r, hipStream_t st);
size_t pe_fullpass_lds_bytes(uint32_t n);
hipError_t pe_launch_fullpass_svc(const pe::SweepArgs* a_dev, int np, bool lean, const uint32_t* visit, uint32_t n,
                                  uint32_t count, pe_ranked_node* out, uint32_t* state, hipStream_t st);
hipError_t pe_launch_fullpass_lds(const pe::SweepArgs* a_dev, int np, const uint32_t* visit, uint32_t n,
                                  uint32_t count, pe_ranked_node* out, uint32_t* state, unsigned long long* prof,
                                  hipStream_t st);
hipError_t pe_launch_sweep_only(const pe::SweepArgs* a, uint32_t blocks, hipStream_t st);
hipError_t pe_launch_sweep_local(const pe::SweepArgs* a, uint32_t blocks, hipStream_t st);
hipError_t pe_launch_trace_top(const uint32_t* codes, const double* sc, const pe::TraceSrc* src, uint32_t flags,
                               pe_metric_score* out, uint8_t* n_out, hipStream_t st, uint32_t n_entries,
                               uint32_t* n_other = nullptr, uint2* other_list = nullptr);
hipError_t pe_launch_step_only(const pe::SweepArgs* a, uint32_t nrecs, const uint32_t* visit, uint32_t n,
                               uint32_t offset, pe_ranked_node* out, uint32_t* state, hipStream_t st);
hipError_t pe_launch_commit_rows(const pe::NodeSoA* s, const pe::TgTables* t, const pe::Ask* a, const uint32_t* rows,
                                 uint32_t n, hipStream_t st);
hipError_t pe_launch_evict_trace(const pe::PreemptArgs* a, const uint32_t* rows, uint32_t n, uint32_t* code,
                                 double* named, hipStream_t st);
hipError_t pe_launch_plan_stop(pe::NodeRec* rec, uint32_t* dev_free, const pe::PreemptAlloc* allocs,
                               uint8_t* preempted, const uint32_t* slots, const uint32_t* rows, uint32_t n, int sign,
                               uint64_t* core_used, const uint64_t* palloc_cores, hipStream_t st);
hipError_t pe_launch_reset_plan(pe::NodeRec* rec, const pe::NodeRec* base_rec, uint32_t* dev_free,
                                const uint32_t* dev_free_base, uint32_t n, uint8_t* preempted, uint32_t m,
                                uint32_t* pcount, uint32_t keys, hipStream_t st);
hipError_t pe_launch_commit(const pe::NodeSoA* s, const pe::TgTables* t, const pe::Ask* a, uint32_t row,
                            uint32_t offers, hipStream_t st);
hipError_t pe_launch_evict(const pe::PreemptArgs* a, const pe::EvictResolveArgs* r, hipStream_t st);
hipError_t pe_launch_apply_commits(const pe::NodeSoA* s, const pe::TgTables* t, const pe::Ask* a, const uint32_t* rows,
                                   const uint32_t* offers, uint32_t n, int sign, hipStream_t st);
hipError_t pe_launch_evict_record(const pe::PreemptArgs* a, uint32_t row, pe_ranked_node* out, uint32_t* mask,
                                  hipStream_t st);
hipError_t pe_launch_commit_preempt(const pe::PreemptArgs* a, uint32_t row, const uint32_t* mask, uint8_t* preempted,
                                    uint32_t* pcount, uint32_t* dev_free, hipStream_t st);
hipError_t pe_launch_evict_only(const pe::PreemptArgs* a, hipStream_t st);
hipError_t pe_launch_census(const pe::BatchArgs* a, uint32_t* counts, uint8_t* status, double* score,
                            hipStream_t st, double* parts = nullptr, uint8_t* nparts = nullptr);
hipError_t pe_launch_resolve(const pe::EvictResolveArgs* r, hipStream_t st);
hipError_t pe_launch_ploop(const pe::PLoopArgs* a, hipStream_t st);
hipError_t pe_launch_md_gate(pe::MdNet* md, const uint32_t* coll_tg, uint32_t n, hipStream_t st);
hipError_t pe_launch_static_gate(const uint8_t* blocked, const uint32_t* coll_tg, uint32_t* gate, uint32_t n,
                                 hipStream_t st);
uint32_t pe_ploop_max_n(uint32_t words);
hipError_t pe_launch_commit_evicted(const pe::PreemptArgs* a, uint8_t* preempted, uint32_t* pcount,
                                    uint32_t* dev_free, uint32_t* placed, hipStream_t st);
hipError_t pe_launch_csi_avail(const pe::CsiArgs* a, hipStream_t st);
hipError_t pe_launch_csi_codes(const pe::CsiArgs* a, hipStream_t st);
hipError_t pe_launch_csi_first(const pe::BatchArgs* a, const pe::CsiLoopArgs* c, hipStream_t st);
// log (or null): the trace log of pe_place_csi_metrics (k_csi_loop<true>), mapped
// page-locked memory of log_cap >= count * n_visit bytes
hipError_t pe_launch_csi_loop(const pe::BatchArgs* a, const pe::CsiLoopArgs* c, hipStream_t st,
                              uint8_t* log = nullptr, uint32_t log_cap = 0);
// pe_place_destructive's loop (k_destructive): the stop list holds a->count updates.
hipError_t pe_launch_destructive(const pe::BatchArgs* a, const pe::DestructiveArgs* d, hipStream_t st);
// pe_place_destructive_full's loop (k_destructive_full): a_dev is a device copy of
// `a` (a group's folded SweepArgs with np spread sets), the stop list holds
// `count` updates of kDfWords words, `out` and `state` (8 words, zeroed) may be
// mapped page-locked memory. pe_destructive_full_cap: the LDS entries it holds.
// cnt_log (or null): pe_place_destructive_full_metrics' use counts per update
// (k_destructive_full<*, true>), count * pset_cnt_total words of device memory.
uint32_t pe_destructive_full_cap();
hipError_t pe_launch_destructive_full(const pe::SweepArgs* a, const pe::SweepArgs* a_dev, int np,
                                      const pe::DestructiveFullArgs* f, const uint32_t* visit, uint32_t n,
                                      uint32_t count, pe_ranked_node* out, uint32_t* state, hipStream_t st,
                                      uint32_t* cnt_log = nullptr, size_t cnt_log_words = 0);
// pe_place_csi_full's loop (k_csi_full): ev_score / ev_kind hold n_visit entries each.
// log (or null): the trace log of pe_place_csi_full_metrics (k_csi_full<*, true>), as pe_launch_csi_loop's
uint32_t pe_csi_full_threads();
hipError_t pe_launch_csi_full(const pe::BatchArgs* a, const pe::CsiLoopArgs* c, double* ev_score, uint8_t* ev_kind,
                              hipStream_t st, uint8_t* log = nullptr, uint32_t log_cap = 0);
size_t pe_fold_feas_max_classes();
hipError_t pe_launch_fold_feas_staged(const pe::NodeSoA* s, const unsigned char* class_src, uint8_t* class_dst,
                                      uint32_t ncls, const uint8_t* node_ok, uint8_t* feas, hipStream_t st);
hipError_t pe_launch_fold_feas(const pe::NodeSoA* s, const uint8_t* class_ok, const uint8_t* node_ok, uint8_t* feas,
                               hipStream_t st);
hipError_t pe_launch_sweep(const pe::SweepArgs* a, uint32_t blocks, pe::SweepRec* merged, hipStream_t st);
hipError_t pe_launch_node_record(const pe::SweepArgs* a, uint32_t row, pe_ranked_node* out, hipStream_t st);
hipError_t pe_launch_spread_table(const pe::TgTables* t, double* tab, hipStream_t st);
uint32_t pe_rec_winner(const pe::SweepRec* r);
void pe_rec_init(pe::SweepRec* r);
void pe_rec_merge(pe::SweepRec* a, const pe::SweepRec* b);
int pe_sweep_blocks_per_cu(bool aux);
hipError_t pe_launch_fold_aux(const pe::NodeSoA* s, const pe::TgTables* t, const uint8_t* aff_idx_class,
                              const uint8_t* aff_idx_node, uint32_t* aux, hipStream_t st);
uint32_t pe_chain_max_n();
uint32_t pe_chain_fused_max_n();
int pe_chain_shape(uint32_t n_visit, int forced);
uint32_t pe_chain_fused_max_count();
uint32_t pe_chain_fused_max_classes();
uint32_t pe_emit_grid(uint32_t count);
uint32_t pe_chain_max_limit();
size_t pe_chain_lds_bytes(int hash_bits, bool packed, uint32_t n);
int pe_chain_blocks_per_cu(size_t lds);
size_t pe_chain_one_lds_bytes(uint32_t n_visit, uint32_t count, uint32_t limit);
size_t pe_chain_one_max_dyn();
bool pe_chain_one_fits(uint32_t n_visit, uint32_t count, uint32_t limit);
hipError_t pe_launch_chain(const pe::BatchArgs* a, uint32_t n_evals, uint32_t max_blocks, int forced_items,
                           hipStream_t st, hipEvent_t* split = nullptr, bool wide_one = false);
hipError_t pe_launch_sweep_step(const pe::SweepArgs* a, uint32_t blocks, const uint32_t* visit, uint32_t n,
                                uint32_t offset, pe_ranked_node* out, uint32_t* state, hipStream_t st);
hipError_t pe_launch_trace(const pe::NodeSoA* s, const pe::TgTables* t, const pe::Ask* a, const uint32_t* rows,
                           uint32_t n, uint32_t* out, const uint32_t* penalty_bits, double log10,
                           const double* spread_tab, double* scores, hipStream_t st, const uint16_t* dks = nullptr);
hipError_t pe_launch_trace_batch(const pe::NodeSoA* s, const pe::TgTables* t, const pe::Ask* a,
                                 const pe::TraceSrc* src, uint32_t n, uint32_t* out, double log10,
                                 const double* spread_tab, double* scores, hipStream_t st,
                                 const pe::TraceStops* stops = nullptr);   // stops: k_trace<true>, a destructive loop's records
hipError_t pe_launch_spread_tables(const pe::TgTables* t, uint32_t n_rec, uint32_t* delta, double* tab,
                                   hipStream_t st, bool absolute = false);   // absolute: delta holds the counts themselves
