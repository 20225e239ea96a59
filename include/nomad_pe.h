/*
 * nomad_pe.h — C ABI of the MI355X placement engine for Nomad's scheduler hot path.
 *
 * The engine replaces the placement stack behind `scheduler.Stack`
 * (reference: scheduler/stack.go:23-32 — SetNodes / SetJob / Select) for the
 * GenericStack (stack.go:41-179, 336-431) and SystemStack (stack.go:181-333).
 * The Go callers (GenericScheduler.computePlacements, generic_sched.go:472-652;
 * SystemScheduler.computePlacements, scheduler_system.go:283-425) stay
 * unchanged; a cgo shim flattens structs.Node / structs.Job
 * into the POD tables below and calls these entry points.
 *
 * Conventions
 *  - Plain pointers and sizes only; every pointer is borrowed for the duration
 *    of the call (cgo pointer rules) and copied by the engine.
 *  - Strings are interned by the caller: one table per state snapshot
 *    (pe_strtab), every string field is a uint32 id into it; equal strings must
 *    share one id. PE_NONE marks "absent" where a field is optional.
 *  - Every function returns 0 on success or a negative PE_E* code; the message
 *    is available from pe_last_error(handle). "No feasible node" is NOT an
 *    error: Select writes row = -1, exactly like a nil *RankedNode.
 *  - A handle is used by one thread at a time (one Stack per eval worker,
 *    nomad/worker.go:244-274). Handles are independent.
 */
#ifndef NOMAD_PE_H
#define NOMAD_PE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PE_ABI_VERSION 9u
#define PE_NONE 0xFFFFFFFFu
#define PE_MAX_SCORES 8
#define PE_MAX_PREEMPT 16   /* PreemptedAllocs carried inline per RankedNode (the
                               full list of a longer one: pe_preempted_of) */
#define PE_MAX_DEVICE_REQ 4 /* device requests of a task group on the device path */
#define PE_MAX_DEVICES 8    /* GPUs one handle drives (pe_config.device_ids) */

/* ---- status codes ------------------------------------------------------ */
#define PE_OK 0
#define PE_EINVAL (-1)       /* malformed input */
#define PE_ESTATE (-2)       /* call order violated (e.g. Select before SetJob) */
#define PE_EHIP (-3)         /* HIP runtime failure */
#define PE_EUNSUPPORTED (-4) /* feature not on the device path (CSI, cores, ...):
                                the shim falls back to the Go chain for this Select */
#define PE_ENOMEM (-5)
#define PE_EINTERNAL (-6)    /* an engine invariant failed on the device (a kernel bounds guard tripped);
                                the call is abandoned, the handle must be reset (pe_set_state) */

/* ---- interned strings -------------------------------------------------- */
typedef struct pe_strtab {
    const char* bytes;        /* concatenated bytes */
    const uint32_t* offsets;  /* count+1 entries; string i = bytes[offsets[i], offsets[i+1]) */
    uint32_t count;
} pe_strtab;

/* ---- typed device attribute (plugins/shared/structs/attribute.go:39-61) -- */
#define PE_ATTR_INT 1
#define PE_ATTR_FLOAT 2
#define PE_ATTR_STRING 3
#define PE_ATTR_BOOL 4
typedef struct pe_attr {
    uint32_t kind;    /* PE_ATTR_* */
    uint32_t unit;    /* str id of the unit ("" if none) */
    int64_t i;        /* int / bool value */
    double f;         /* float value */
    uint32_t s;       /* str id for string values */
    uint32_t _pad;
} pe_attr;

/* ---- node table: the structs.Node fields the hot path reads -------------
 * (nomad/structs/structs.go:1812-1914). One row per node of the State
 * snapshot. CSR lists use off[n+1].                                         */
typedef struct pe_node_table {
    uint32_t n;
    const uint32_t* id;              /* Node.ID                     */
    const uint32_t* name;            /* Node.Name                   */
    const uint32_t* datacenter;      /* Node.Datacenter             */
    const uint32_t* node_class;      /* Node.NodeClass              */
    const uint32_t* computed_class;  /* Node.ComputedClass (node_class.go:31) */
    const int64_t* cpu_shares;       /* NodeResources.Cpu.CpuShares */
    const int64_t* memory_mb;        /* NodeResources.Memory.MemoryMB */
    const int64_t* disk_mb;          /* NodeResources.Disk.DiskMB   */
    const int64_t* reserved_cpu;     /* ReservedResources.Cpu.CpuShares */
    const int64_t* reserved_memory_mb;
    const int64_t* reserved_disk_mb;
    /* Attributes / Meta maps */
    const uint32_t* attr_off; const uint32_t* attr_key; const uint32_t* attr_val;
    const uint32_t* meta_off; const uint32_t* meta_key; const uint32_t* meta_val;
    /* Drivers map: flags bit0 Detected, bit1 Healthy, bit2 DriverInfo==nil */
    const uint32_t* drv_off; const uint32_t* drv_name; const uint8_t* drv_flags;
    /* NodeResources.Networks: mode ("" = host), device, MBits */
    const uint32_t* net_off; const uint32_t* net_mode; const uint32_t* net_device;
    const int32_t* net_mbits;
    /* NodeResources.NodeNetworks[*].Addresses[*].Alias (host networks) */
    const uint32_t* alias_off; const uint32_t* alias_name;
    /* node-reserved host ports that fall in the dynamic range [20000,32000) */
    const int32_t* reserved_dyn_ports;
    /* HostVolumes map */
    const uint32_t* hv_off; const uint32_t* hv_name; const uint8_t* hv_read_only;
    /* NodeResources.Devices (device groups) */
    const uint32_t* dev_off;
    const uint32_t* dev_vendor; const uint32_t* dev_type; const uint32_t* dev_name;
    const uint32_t* dev_healthy;     /* healthy instance count */
    const uint32_t* dev_attr_off;    /* CSR over device groups */
    const uint32_t* dev_attr_key; const pe_attr* dev_attr_val;
    /* NodeResources.Cpu.ReservableCpuCores (CSR over nodes) and TotalCpuCores;
       ReservedResources.Cpu.ReservedCpuCores (CSR). NULL: no core sets */
    const uint32_t* core_off; const uint16_t* core_id;
    const uint32_t* total_cores;
    const uint32_t* rsv_core_off; const uint16_t* rsv_core_id;
    /* NodeResources.NodeNetworks[*].Addresses[*] in node order (CSR): Alias,
       Address and its ReservedPorts spec (ParsePortRanges syntax, PE_NONE =
       none); ReservedResources.Networks.ReservedHostPorts per node (PE_NONE =
       none). NULL: no addresses (static port asks then find none) */
    const uint32_t* addr_off; const uint32_t* addr_alias; const uint32_t* addr_ip;
    const uint32_t* addr_rsv_ports;
    const uint32_t* rsv_host_ports;
    /* NodeResources.Networks[*] addresses (str ids, per net_off entry): the IP
       field (PE_NONE = "") and the one address AssignNetwork yields from the
       CIDR (yieldIP, network.go:294-315; PE_NONE when the CIDR does not parse;
       an IPv4 block of several addresses may be given as its text "a.b.c.d/len",
       which the engine treats as not one address). NULL: unknown (task-level static ports
       are then not on the device path) */
    const uint32_t* net_ip; const uint32_t* net_cidr_ip;
} pe_node_table;

/* ---- existing allocations of the snapshot (state AllocsByNode) ---------- */
typedef struct pe_alloc_table {
    uint32_t count;
    const uint32_t* node_row;        /* row in pe_node_table          */
    const uint32_t* ns;              /* Allocation.Namespace          */
    const uint32_t* job_id;          /* Allocation.JobID              */
    const uint32_t* task_group;      /* Allocation.TaskGroup          */
    const uint8_t* terminal;         /* Allocation.TerminalStatus()   */
    const int32_t* priority;         /* Allocation.Job.Priority       */
    const int64_t* cpu_shares;       /* ComparableResources().Flattened.Cpu.CpuShares */
    const int64_t* memory_mb;        /* ...Flattened.Memory.MemoryMB  */
    const int64_t* disk_mb;          /* ...Shared.DiskMB              */
    const int32_t* net_mbits;        /* bandwidth held on the node's host device */
    const int32_t* dyn_ports;        /* ports held in [20000,32000)  */
    /* device instances held: CSR over allocs, (device group index on its node, count) */
    const uint32_t* dev_off; const uint32_t* dev_group; const uint32_t* dev_count;
    /* TaskGroup.Migrate.MaxParallel of the alloc's job, or NULL = 0 for every
       alloc (Preemptor.SetCandidates, scheduler/preemption.go:141-154) */
    const int32_t* max_parallel;
    /* ComparableResources().Flattened.Cpu.ReservedCores (CSR over allocs), or NULL */
    const uint32_t* core_off; const uint16_t* core_id;
    /* ports the alloc holds (NetworkIndex.AddAllocs: AllocatedPorts HostIP /
       Value, or the pre-0.12 networks' IP and ports), CSR over allocs, or NULL */
    const uint32_t* port_off; const uint32_t* port_ip; const int32_t* port_value;
    /* ComparableResources().Flattened.Networks is non-empty (the alloc takes
       part in PreemptForNetwork, preemption.go:302-331), or NULL: derived as
       net_mbits > 0 || dyn_ports > 0 || the alloc holds ports */
    const uint8_t* has_network;
    /* the Device of the alloc's networks (NetworkResource.Device; string id),
       or PE_NONE / NULL: the node's first host network device. Bandwidth is
       kept per device (NetworkIndex.UsedBandwidth[device], network.go:196-230);
       a Select with Preempt whose PreemptForNetwork candidates sit on two
       devices returns PE_EUNSUPPORTED (the reference ranges over a Go map) */
    const uint32_t* net_device;
} pe_alloc_table;

/* ---- job specification (structs.Job / TaskGroup / Task) ----------------- */
typedef struct pe_constraint { uint32_t ltarget, rtarget, operand; } pe_constraint;
typedef struct pe_affinity { uint32_t ltarget, rtarget, operand; int32_t weight; } pe_affinity;
typedef struct pe_spread_target { uint32_t value; int32_t percent; } pe_spread_target;
typedef struct pe_spread {
    uint32_t attribute; int32_t weight;       /* weight is an int8 in structs.Spread */
    uint32_t target_off, target_count;        /* into pe_job.spread_targets */
} pe_spread;
typedef struct pe_device_request {           /* structs.RequestedDevice */
    uint32_t name; uint32_t _pad; uint64_t count;
    uint32_t constraint_off, constraint_count; /* into pe_job.device_constraints */
    uint32_t affinity_off, affinity_count;     /* into pe_job.device_affinities  */
} pe_device_request;
#define PE_LC_MAIN 0
#define PE_LC_PRESTART 1
#define PE_LC_PRESTART_SIDECAR 2
#define PE_LC_POSTSTOP 3
#define PE_LC_POSTSTART 4   /* not counted by AllocatedResources.Comparable() */
typedef struct pe_task {
    uint32_t name, driver;
    int64_t cpu, memory_mb, memory_max_mb;
    int32_t cores;                            /* Resources.Cores: reserved cores (rank.go:437-466) */
    uint32_t lifecycle;                       /* PE_LC_* */
    int32_t has_network, net_mbits, net_dyn_ports, net_reserved_ports;
    uint32_t constraint_off, constraint_count;
    uint32_t affinity_off, affinity_count;
    uint32_t device_off, device_count;
    uint32_t rport_off;                       /* the task network's ReservedPorts (static ports):
                                                 pe_job.rport_value / rport_label [rport_off,
                                                 rport_off + net_reserved_ports) */
} pe_task;
typedef struct pe_task_group {
    uint32_t name; int32_t count;
    int64_t ephemeral_disk_mb;
    uint32_t constraint_off, constraint_count;
    uint32_t affinity_off, affinity_count;
    uint32_t spread_off, spread_count;
    uint32_t task_off, task_count;
    int32_t has_network; uint32_t net_mode;   /* tg Networks[0] */
    int32_t net_dyn_ports, net_reserved_ports;
    uint32_t net_host_network;                /* host network alias of the ports ("default") */
    uint32_t volume_off, volume_count;        /* host volume requests */
    int32_t has_csi_volumes;                  /* CSI: not on the device path */
    uint32_t rport_off, rport_count;          /* tg network ReservedPorts (static ports): into
                                                 pe_job.rport_value / rport_label */
} pe_task_group;
#define PE_JOB_SERVICE 0
#define PE_JOB_BATCH 1
#define PE_JOB_SYSTEM 2
#define PE_JOB_SYSBATCH 3
typedef struct pe_job {
    uint32_t id, ns, type; int32_t priority;
    uint64_t version;
    uint32_t constraint_off, constraint_count;
    uint32_t affinity_off, affinity_count;
    uint32_t spread_off, spread_count;
    uint32_t tg_count;
    const pe_task_group* task_groups;
    const pe_task* tasks;
    const pe_constraint* constraints;        /* job, tg and task constraints */
    const pe_affinity* affinities;
    const pe_spread* spreads;
    const pe_spread_target* spread_targets;
    const pe_device_request* devices;
    const pe_constraint* device_constraints;
    const pe_affinity* device_affinities;
    const uint32_t* volume_source;           /* host volume requests: source name */
    const uint8_t* volume_read_only;
    const int32_t* rport_value;              /* static ports: Port.Value and Port.Label */
    const uint32_t* rport_label;
} pe_job;

/* ---- stack configuration (SchedulerConfiguration, operator.go:128-210) --- */
#define PE_STACK_GENERIC 0
#define PE_STACK_SYSTEM 1
#define PE_ALGO_BINPACK 0
#define PE_ALGO_SPREAD 1
typedef struct pe_config {
    uint32_t stack_kind;      /* PE_STACK_* */
    uint32_t batch;           /* GenericStack batch flag (limit 2) */
    uint32_t algorithm;       /* PE_ALGO_* */
    uint32_t memory_oversubscription;
    uint32_t preempt;         /* SystemStack: BinPack eviction enabled (stack.go:267-278).
                                 GenericStack: PreemptionConfig.{Service,Batch}SchedulerEnabled:
                                 pe_place retries a nil Select with Preempt=true
                                 (selectNextOption, generic_sched.go:773-792) */
    int32_t device;           /* HIP device ordinal (device_count <= 1) */
    /* One handle over several GPUs of this process (SURVEY.md §8b "device
     * count/ids"): device_ids[0] holds the handle's own state, the others
     * replicas of it; full-pass count loops (pe_place of task groups with
     * affinities / spreads) and pe_system_place split the rows over all of
     * them, exchanging per-placement records with ncclAllGather over
     * communicators from ncclCommInitAll. Ids that all name one GPU run the
     * same split with device copies instead of RCCL (loopback, for tests).
     * 0 or 1: the single `device`. */
    uint32_t device_count;
    int32_t device_ids[PE_MAX_DEVICES];
} pe_config;

typedef struct pe_select_options {              /* SelectOptions, stack.go:34-39 */
    const uint32_t* penalty_rows; uint32_t penalty_count;
    const uint32_t* preferred_rows; uint32_t preferred_count;
    uint32_t preempt;
} pe_select_options;

typedef struct pe_ranked_node {                 /* RankedNode, rank.go:21-36 */
    int32_t row;              /* chosen node row, -1 = nil */
    uint32_t n_scores;
    double final_score;
    double scores[PE_MAX_SCORES];   /* rank order: binpack, device-aff, anti-aff,
                                       penalty, node-aff, spread, preemption */
    /* AllocMetric side outputs (structs.go:9826-10026) */
    uint32_t nodes_evaluated, nodes_filtered, nodes_exhausted;
    uint32_t new_offset;      /* StaticIterator cursor after the Select */
    /* PreemptedAllocs (rank.go:511-513): rows of the pe_alloc_table snapshot;
       n_preempted is the whole count, the first PE_MAX_PREEMPT are inline */
    uint32_t n_preempted;
    uint32_t preempted[PE_MAX_PREEMPT];
    /* TaskResources device offers (rank.go:404-405): per device request of the
       task group (tasks in order), the index of the chosen device group on the node */
    uint32_t n_device_offers;
    uint32_t device_offer_group[PE_MAX_DEVICE_REQ];
    /* Cpu.ReservedCores of the task group's tasks (rank.go:437-466): bit c =
       core c; tasks asking cores take them in task order, lowest ids first */
    uint64_t reserved_cores[4];
} pe_ranked_node;

typedef struct pe_placement {                   /* compact per-placement record (batches) */
    int32_t row;              /* chosen node row, -1 = nil (count loop stopped) */
    uint32_t nodes_evaluated;
    double final_score;
} pe_placement;

/* ---- entry points -------------------------------------------------------- */
typedef struct pe_stack pe_stack;

uint32_t pe_abi_version(void);
/* NewGenericStack (stack.go:336) / NewSystemStack (stack.go:207) */
pe_stack* pe_stack_create(const pe_config* cfg);
void pe_stack_destroy(pe_stack* s);
const char* pe_last_error(const pe_stack* s);
/* State snapshot: nodes + non-terminal allocs (scheduler.State, scheduler.go:66-110).
 * Uploads the node SoA to HBM; stays resident across evals until replaced. */
int pe_set_state(pe_stack* s, const pe_strtab* strs, const pe_node_table* nodes,
                 const pe_alloc_table* allocs);
/* Start a new evaluation on the resident snapshot: drop the plan (proposed
 * allocs), the EvalEligibility memo and the job (NewEvalContext, context.go:86).
 * The node SoA stays in HBM; only the dynamic columns are restored. */
/* Apply an allocation delta of the state store to the resident snapshot
 * without reloading the nodes (client-status changes that make allocs
 * terminal, allocs placed by other workers' applied plans; nomad/state
 * UpsertAllocs / UpsertPlanResults). Entry i overwrites snapshot alloc
 * index[i], or is appended when index[i] == PE_NONE (or index == NULL); the
 * appended ones take the next indices in order. `strs` extends the snapshot's
 * string table (same ids for the strings it already had). Equivalent to
 * pe_set_state with the updated table: the plan, the memo and the job are
 * reset (a state change starts a new evaluation). */
int pe_update_allocs(pe_stack* s, const pe_strtab* strs, const pe_alloc_table* allocs, const uint32_t* index);
int pe_reset_plan(pe_stack* s);
/* Node upserts into the resident snapshot (state_store.go UpsertNode and the
 * node_endpoint.go Register / UpdateStatus / UpdateDrain paths, with
 * Node.ComputeClass computed by the caller, node_class.go:31-104): row i of
 * `nodes` replaces snapshot row index[i], or is appended when index is NULL
 * or index[i] == PE_NONE (appended rows take the next row numbers in order).
 * The allocs stay; a node's allocs keep their rows. Like pe_update_allocs it
 * starts a new evaluation context (pe_set_job / pe_set_nodes again). */
int pe_update_nodes(pe_stack* s, const pe_strtab* strs, const pe_node_table* nodes, const uint32_t* index);
/* Stack.SetJob (stack.go:93-115 / 290-299). `strs` extends the table given to
 * pe_set_state (same ids for its first entries, job strings appended). */
int pe_set_job(pe_stack* s, const pe_strtab* strs, const pe_job* job);
/* Stack.SetNodes (stack.go:71-91 / 285-288). `rows` is the node list AFTER the
 * caller's shuffleNodes (util.go:366-372): the engine draws no randomness.
 * Writes the LimitIterator limit to *limit_out (may be NULL). */
int pe_set_nodes(pe_stack* s, const uint32_t* rows, uint32_t n, uint32_t* limit_out);
/* Stack.Select (stack.go:117-179 / 301-333) */
int pe_select(pe_stack* s, uint32_t tg_index, const pe_select_options* opts,
              pe_ranked_node* out);
/* Plan.AppendAlloc (structs.go:10707-10714) of an allocation of task group
 * `tg_index` on node `row`: the proposed state seen by later Selects.
 *
 * Speculation (transparent to the caller): the first plain Select of a task
 * group (no preferred / penalty nodes, no Preempt, metrics off) runs the
 * device count loop for the group's remaining placements and returns its first
 * record; while every pe_commit names the row the previous Select returned,
 * later plain Selects of that group are answered from the loop's records with
 * no device work. Any other call first restores the device state to the
 * committed prefix, so results always equal one-at-a-time Selects.
 * PE_SPECULATE=0 in the environment disables it. */
int pe_commit(pe_stack* s, uint32_t tg_index, int32_t row);
/* Apply queued device work now: the speculative count loop's confirmed
 * placements and the SystemScheduler fast path's queued commits (every entry
 * point that reads the device state does this itself; callers use it to
 * settle the device at a point of their choosing). */
int pe_flush(pe_stack* s);
/* SystemStack fast path counters: out[0] k_system passes over the snapshot
 * that filled the per-row cache, out[1] single-node Selects answered from it. */
int pe_system_spec_stats(const pe_stack* s, uint64_t* out2);
/* GPUs this handle drives (pe_config.device_count; 1 for a single device). */
uint32_t pe_device_count(const pe_stack* s);
/* Multi-GPU: one engine handle per GPU and process, joined by
 * an RCCL communicator (ncclGetUniqueId on one rank, the 128 bytes shared by
 * the caller, ncclCommInitRank on every rank). */
int pe_comm_unique_id(uint8_t* out, size_t cap);
/* The RCCL library the collectives call, bound at first use: the one the
 * process already has mapped (soname librccl.so.1, e.g. torch's), else
 * /opt/rocm/lib/librccl.so.1, followed by " (RCCL major.minor.patch)"; ""
 * when none loads or its major version differs from the rccl.h the engine is
 * built against (the communicator calls then fail with that reason). */
const char* pe_comm_library(void);
int pe_comm_init(pe_stack* s, int nranks, int rank, const uint8_t* id);
/* A caller-provided transport instead of RCCL (ranks on hosts without an
 * RCCL path between them, or the CPU rehearsal of the per-GPU processes):
 * exchange(ctx, send, recv, bytes) is an all-gather in rank order, `bytes`
 * from this rank into recv[rank * bytes], returning 0 on success. It is called
 * from the thread inside pe_place_sharded once per placement, on host buffers
 * (the record crosses PCIe both ways). Replaces any RCCL communicator. */
typedef int (*pe_exchange_fn)(void* ctx, const void* send, void* recv, size_t bytes);
int pe_comm_init_host(pe_stack* s, int nranks, int rank, pe_exchange_fn exchange, void* ctx);
/* The full-pass count loop (task groups with affinities / spreads, limit >=
 * list) sharded over the ranks: every rank holds the whole snapshot, job and
 * SetNodes list and sweeps its rows [row_begin, row_end) into one 80-byte
 * record (the sweep's last workgroup merges the rank's workgroup records);
 * per placement one ncclAllGather of the ranks' records on the engine stream
 * (nranks x 80 B), then every rank resolves and commits the same winner.
 * Every rank receives the same records. Windowed task groups return
 * PE_EUNSUPPORTED (replicas only). */
int pe_place_sharded(pe_stack* s, uint32_t tg_index, uint32_t count, uint32_t row_begin, uint32_t row_end,
                     pe_ranked_node* out, uint32_t* placed);
/* Device time of the all-gather in the last pe_place_sharded (microseconds,
 * mean over every placement; includes waiting for peer ranks). */
double pe_last_exchange_us(const pe_stack* s);
/* The same as out4 = {mean, min, max} microseconds and the placements timed
 * (0 at one rank: no exchange runs). */
int pe_last_exchange_stats(const pe_stack* s, double* out4);
/* Counters of the speculative loop: out[0] runs started, [1] Selects answered
 * from records, [2] rollbacks (the caller deviated), [3] records computed. */
int pe_speculation_stats(const pe_stack* s, uint64_t* out4);
/* Counters of the chain's wide phase launches (PE_CHAIN_WIDE): out[0] phases
 * they resolved, [1] phases they declined (left to k_chain). */
int pe_chain_wide_stats(const pe_stack* s, uint64_t* out2);
/* Chain launches with wide phases, by kind: out[0] with two k_phase launches,
 * [1] with both phases in one k_phases launch (PE_CHAIN_WIDE_ONE=0: never). */
int pe_chain_wide_launches(const pe_stack* s, uint64_t* out2);
/* The one-launch gate for a list of n_visit positions, a launch of `count`
 * Selects and a limit: out[0] the dynamic LDS bytes the launch needs, [1] what
 * a workgroup of the current device may hold. Returns 1 if k_phases takes the
 * launch, 0 if the two k_phase launches do, a negative PE_E* on an error. */
int pe_chain_wide_one_lds(uint32_t n_visit, uint32_t count, uint32_t limit, uint64_t* out2);
/* Plan.AppendAlloc plus Plan.AppendPreemptedAlloc of each preempted alloc
 * (handlePreemptions, generic_sched.go:794-816): `preempted` are alloc-table
 * rows, as returned in pe_ranked_node.preempted by a Select with Preempt. */
int pe_commit_preempt(pe_stack* s, uint32_t tg_index, int32_t row, const uint32_t* preempted,
                      uint32_t n_preempted);
/* The full PreemptedAllocs of record `record` of the last pe_select (record 0)
 * or pe_place (record k) when it holds more than PE_MAX_PREEMPT (rank.go:511-513
 * has no cap): writes min(cap, n) alloc-table rows, the first PE_MAX_PREEMPT
 * equal to the inline ones, and returns n; PE_ESTATE when that record carries
 * its whole list inline. Valid until the next pe_select / pe_place /
 * pe_system_place. The Go shim calls it when n_preempted > PE_MAX_PREEMPT,
 * before pe_commit_preempt(row, list, n). Replaces reading
 * RankedNode.PreemptedAllocs past the inline array (rank.go:511-513). */
int pe_preempted_of(const pe_stack* s, uint32_t record, uint32_t* out, uint32_t cap);
/* Plan.AppendStoppedAlloc (structs.go:10628-10660) of `n` snapshot allocs
 * (alloc-table rows): each becomes a NodeUpdate entry of its node, and a
 * non-terminal one leaves the proposed state of the node
 * (EvalContext.ProposedAllocs, context.go:120-157: resources, devices, the
 * job's collision counts; the property sets count it as cleared,
 * propertyset.go:159-209). The stops of computeJobAllocs
 * (generic_sched.go:382), of a destructive update's previous alloc (:546), of
 * inplaceUpdate / genericAllocUpdateFn (util.go:749, 1037) and of the
 * SystemScheduler (scheduler_system.go:230-241). Undone by pe_reset_plan. */
int pe_plan_stop(pe_stack* s, const uint32_t* allocs, uint32_t n);
/* Plan.PopUpdate (structs.go:10691-10702): drops the last NodeUpdate entry of
 * the alloc's node when it is this alloc (generic_sched.go:644, util.go:756,
 * 1043); otherwise nothing happens. */
int pe_plan_pop_update(pe_stack* s, uint32_t alloc);
/* computePlacements' loop over its `destructive` list (generic_sched.go:493-649)
 * for `n` updates of task group `tg_index`: allocs[i] is the alloc-table row of
 * update i's previous allocation. In list order, for i in [0, n):
 * AppendStoppedAlloc(allocs[i]) (:543-547), a plain Select of the group on the
 * current SetNodes list from the current cursor (:552), AppendAlloc on the
 * option's node (:627); on nil PopUpdate(allocs[i]) (:639-645) and the loop
 * ends (:521-525). out[0..*placed) are the placements; when *placed < n,
 * out[*placed] is the nil Select's record, as pe_place writes it.
 *
 * One upload of the stop list, one launch of the loop kernel (k_destructive)
 * and one synchronisation whatever `n`. Records and every later observable
 * state equal those of the per-call sequence pe_plan_stop(&allocs[i], 1),
 * pe_select(tg, NULL), then pe_commit, or pe_plan_pop_update(allocs[i]) and a
 * break: node records, the job's and the group's collision counts, device free
 * counts, dynamic ports and bandwidth; the stop flags, NodeUpdate with its
 * order, the plan; the cursor, the limit, the EvalEligibility memo and its
 * log. An alloc that is terminal, or already stopped or preempted in the plan,
 * contributes its NodeUpdate entry and no resource change, as pe_plan_stop
 * treats it. What pe_plan_stop invalidates per stop (static-port gates, the
 * property sets) is invalidated once, at the end of the call.
 *
 * Penalty and preferred nodes are out of scope: getSelectOptions (:695-716)
 * gives a penalty set only when the previous alloc failed or carries reschedule
 * events, and a preferred node only with a sticky disk. The caller sends those
 * updates through the per-call sequence, and the batched call through each
 * maximal run of the rest.
 *
 * PE_EINVAL (nothing changed): tg_index or an alloc row out of range, an alloc
 * listed twice. PE_ESTATE: not a generic stack, no job, no node list. n == 0:
 * PE_OK with *placed == 0. PE_EUNSUPPORTED, checked before anything changes
 * (cursor, limit, memo, plan and NodeUpdate untouched; the per-call sequence
 * answers instead): a group that runs full passes (node affinities, spreads,
 * distinct_property, or a limit a sibling group's Select latched to MaxInt32);
 * pe_set_metrics on; a preempting stack; a handle over several devices; a
 * reserved-cores ask, or a listed alloc that holds reserved cores; static port
 * asks in the group; a task network on a snapshot with multi-device nodes; a
 * group with CSI requests; two task groups of one name; the group's own
 * unsupported reason; n beyond what the overlay of one launch holds.
 * PE_EINTERNAL: a bounds guard of the kernel tripped (the updates before it
 * stand, as *placed and the mirrors say). */
int pe_place_destructive(pe_stack* s, uint32_t tg_index, const uint32_t* allocs, uint32_t n, pe_ranked_node* out,
                         uint32_t* placed);
/* Measurement aid: what the last pe_place_destructive issued. out3[0] kernel
 * launches (the loop, and a copy launch when the SetNodes list was not on the
 * device yet), [1] stream synchronisations, [2] uploads (the stop list, and
 * that list). After pe_place_destructive_metrics with metrics on the counts
 * include the checkpoint's device copies and the trace's upload, two launches,
 * copy back and synchronisation; none of them depends on `n`. */
int pe_place_destructive_stats(const pe_stack* s, uint64_t* out3);
/* inplaceUpdate (util.go:692-806) for `n` snapshot allocs (alloc-table rows) against task group
 * `tg_index`, in list order. For each: AppendStoppedAlloc, SetNodes([its node]), Select(tg),
 * PopUpdate; when the Select returns an option, the updated alloc replaces the old one
 * (the stop stays in NodeUpdate and the task group's ask is committed on the node).
 * status[i] = 0 updated in place, 1 filtered, 2 exhausted (pe_system_place's codes);
 * out[i] (may be NULL) is the record pe_select would have returned for that Select.
 * *updated = number of status 0.
 *
 * One launch and one synchronisation whatever `n`: results and every later
 * observable state (node records, collision and device free counts, dynamic
 * ports and bandwidth, NodeUpdate, the plan, the EvalEligibility memo) equal
 * those of the per-call sequence pe_plan_stop, pe_set_nodes (one row),
 * pe_select, pe_plan_pop_update and, on an option, pe_plan_stop + pe_commit.
 * The node list is unspecified afterwards: call pe_set_nodes before the next
 * Select (computePlacements does, generic_sched.go:485). Updates of several
 * task groups: one call per maximal run of one group, in order.
 * PE_EINVAL (nothing changed): tg_index or an alloc row out of range, an alloc
 * listed twice. PE_EUNSUPPORTED (nothing changed; the per-call sequence
 * answers): spreads or distinct_property, reserved-cores asks, static ports,
 * multi-device network nodes, a handle over several devices, pe_set_metrics on
 * (pe_inplace_update_metrics below answers that one), a system stack with
 * preemption enabled (pe_inplace_update_preempt below answers that one). */
int pe_inplace_update(pe_stack* s, uint32_t tg_index, const uint32_t* allocs, uint32_t n,
                      pe_ranked_node* out, uint8_t* status, uint32_t* updated);
/* pe_inplace_update for a system stack with preemption enabled, the reference's
 * default for system jobs (nomad/config.go:448-455): the Select of every update
 * is SystemStack.Select's, BinPack with evict (stack.go:267-278) where the
 * plain fit fails. Arguments, result layout, status codes and the node-list
 * rule are pe_inplace_update's; out[i] of an evicting Select carries the
 * eviction's FinalScore and score parts, n_preempted the whole count and the
 * first PE_MAX_PREEMPT alloc-table rows inline (the whole lists:
 * pe_inplace_update_preempted). inplaceUpdate never reads
 * option.PreemptedAllocs (util.go:759-802): the evicted allocs stay in the
 * proposed state, Plan.NodePreemptions and its counts do not move, and a later
 * update on the node may evict the same alloc again, all as the per-call
 * sequence (pe_select then pe_commit, never pe_commit_preempt) leaves it. On a
 * generic stack, or a system stack without preemption, the call is
 * pe_inplace_update. One launch pair and one synchronisation, plus one of each
 * per wider eviction width some listed node needs.
 *
 * PE_EINVAL as pe_inplace_update. PE_EUNSUPPORTED (checked before anything
 * changes): everything pe_inplace_update refuses except preemption itself, and
 * on a preempting system stack: a device ask in the group (the in-place
 * update keeps the old alloc's instances, util.go:767-782, which the packed
 * free counts cannot hold beside evicted holders that stay in the plan);
 * several task networks in the group; a snapshot outside the on-device
 * eviction limits; a listed node of more than 1024 allocs, or whose allocs
 * plus the plan's placements on it plus the listed updates on it exceed 2048. */
int pe_inplace_update_preempt(pe_stack* s, uint32_t tg_index, const uint32_t* allocs, uint32_t n,
                              pe_ranked_node* out, uint8_t* status, uint32_t* updated);
/* The preempted allocs of the last pe_inplace_update_preempt, a CSR in the
 * engine's page-locked staging, valid until the next pe_inplace_update* call on
 * the handle: updates[n_entries] holds the list positions whose Select
 * preempted something, increasing; allocs[off[i] .. off[i + 1]) their
 * alloc-table rows in the order pe_select's record lists them (increasing slot
 * of the node's alloc list). No PE_MAX_PREEMPT cap. PE_ESTATE: no such call
 * yet, or a pe_inplace_update since. */
int pe_inplace_update_preempted(const pe_stack* s, const uint32_t** updates, const uint32_t** off,
                                const uint32_t** allocs, uint32_t* n_entries);
/* pe_inplace_update_preempt for a caller that keeps AllocMetric: inplaceUpdate
 * ends every successful update with newAlloc.Metrics = ctx.Metrics()
 * (util.go:801), so a faithful caller runs with pe_set_metrics on, which the
 * two calls above refuse. This one does not, on a generic stack, a system
 * stack, or a system stack with preemption enabled. Arguments, result layout,
 * status codes, the node-list rule, PE_EINVAL cases and
 * pe_inplace_update_preempted are pe_inplace_update_preempt's; PE_EUNSUPPORTED
 * (checked before anything changes) is its list without the pe_set_metrics
 * entry. With metrics off the call is pe_inplace_update_preempt. With metrics
 * on, records, statuses and every later observable state (the class memo that
 * turns a later node of a failing class into "computed class ineligible"
 * included) are those of the per-call sequence run with metrics on, and
 * pe_inplace_metrics returns each update's maps. No further launch and no
 * further synchronisation than pe_inplace_update_preempt. pe_last_metrics*
 * answer PE_ESTATE afterwards: there is no "last Select". */
int pe_inplace_update_metrics(pe_stack* s, uint32_t tg_index, const uint32_t* allocs, uint32_t n,
                              pe_ranked_node* out, uint8_t* status, uint32_t* updated);
/* (pe_inplace_metric and pe_inplace_metrics: below, with the AllocMetric types.) */
/* pe_inplace_update_metrics that does not refuse spread stanzas, at job or
 * group level (a caller uses pe_inplace_update_csi below, which is this call
 * for every group without CSI requests). SpreadIterator never filters (spread.go:110-174), so the walk
 * decides the statuses without the spread sets; a second stage then adds the
 * allocation-spread part and the FinalScore built from it in list order, from
 * the property counts each update's Select sees in the per-call sequence
 * (the earlier updates' AppendAlloc and stops included). Arguments, result
 * layout, status codes, the node-list rule, PE_EINVAL cases,
 * pe_inplace_update_preempted and pe_inplace_metrics (whose ScoreMetaData
 * item carries allocation-spread) are pe_inplace_update_metrics'. Records,
 * statuses and every later observable state equal the per-call sequence's bit
 * for bit. PE_EUNSUPPORTED (checked before anything changes):
 * pe_inplace_update_metrics' list without "spreads"; distinct_property, alone
 * or beside a spread, stays on it. On a job without spreads, and on a system
 * stack (which drops them, stack.go:207-283), the call is
 * pe_inplace_update_metrics with no further launch; with spreads it adds a
 * memset and three short launches on the same stream (none when out == NULL
 * and metrics are off: the statuses are final) and no further copy back or
 * synchronisation. */
int pe_inplace_update_spread(pe_stack* s, uint32_t tg_index, const uint32_t* allocs, uint32_t n,
                             pe_ranked_node* out, uint8_t* status, uint32_t* updated);
/* pe_inplace_update_spread that does not refuse a task group with CSI volume
 * requests (pe_set_csi, pe_set_csi_requests below), which the four calls above
 * do: the call for every group. alloc_idx[i] is the name index of allocs[i]
 * (AllocSuffix, funcs.go:402), which per_alloc sources take as their suffix
 * for that update only; NULL: every update uses the index pe_csi_alloc_index
 * holds. Records, statuses and every later observable state are those of the
 * per-call sequence with pe_csi_alloc_index(alloc_idx[i]) before each
 * pe_select. CSIVolumeChecker runs behind the wrapper's job and group checks
 * and reads the state snapshot alone (feasible.go:261-337): an update whose
 * node passes those checks and is unavailable for its alloc index has status
 * 1 and a nil record (nodes_evaluated 1, nodes_filtered 1) before
 * distinct_hosts and BinPack are asked, so no fit and, on a preempting stack,
 * no eviction is tried for it; an update the wrapper filters keeps the
 * wrapper's reason, and the class memo advances as if the checker did not
 * exist (feasible.go:1141-1149). With pe_set_metrics on, pe_inplace_metrics
 * gives an unavailable update class_key as for any filtered node, reason_key
 * the engine key of pe_csi_reason_text for the failing request (the keys of
 * pe_place_csi_metrics) and score PE_NONE. The second stage of a job with
 * spreads counts such an update like any other status-1 update: not at all.
 * Afterwards the group's alloc index is alloc_idx[n - 1]. On a group without
 * CSI requests the call is pe_inplace_update_spread (alloc_idx is not read).
 * Otherwise it adds one store-only k_csi_avail launch per distinct set of
 * resolved request records among the listed indices (pe_csi_avail_launches)
 * and one upload of n bytes, and no synchronisation or copy back.
 * PE_EINVAL cases, pe_inplace_update_preempted, pe_inplace_metrics and
 * pe_inplace_spread_ms are pe_inplace_update_spread's. PE_EUNSUPPORTED
 * (checked before anything changes): pe_inplace_update_spread's list without
 * "CSI volumes"; a CSI group without a table or without requests, as pe_select
 * refuses it; computed classes whose nodes differ in the group's checks; more
 * than PE_MAX_CSI_SETS distinct record sets in the list. */
int pe_inplace_update_csi(pe_stack* s, uint32_t tg_index, const uint32_t* allocs, const uint32_t* alloc_idx,
                          uint32_t n, pe_ranked_node* out, uint8_t* status, uint32_t* updated);
/* HIP-event times of the last pe_inplace_update* call's launches in ms:
 * ms2[0] the walk(s), ms2[1] pe_inplace_update_spread's second stage (0 when
 * it did not run). pe_last_kernel_ms gives their sum. */
int pe_inplace_spread_ms(const pe_stack* s, double* ms2);
/* Fused count loop of GenericScheduler.computePlacements (generic_sched.go:493-649)
 * for `count` fresh placements of one task group (no preferred / penalty nodes):
 * Select -> AppendAlloc repeated on the device; stops at the first nil option
 * (failedTGAllocs short-circuit, generic_sched.go:519-523).
 * out[count] receives each placement; *placed the number placed. */
int pe_place(pe_stack* s, uint32_t tg_index, uint32_t count, pe_ranked_node* out,
             uint32_t* placed);
/* Concurrent evaluations (NumSchedulers workers, nomad/config.go:468; each
 * worker runs one eval against its snapshot, nomad/worker.go:244-274).
 * pe_stage_orders copies `n_evals` visit orders (each a shuffled SetNodes list
 * of length n, row ids) to HBM. pe_place_batch then runs, for every staged
 * order, an independent evaluation of `count` placements of task group
 * `tg_index` from the stack's current plan (offset 0), exactly as
 * SetNodes(order) + pe_place would, without modifying the stack's plan.
 * out[n_evals * count] (row-major by eval), placed[n_evals]; either may be NULL:
 * the results always land in a stack-owned page-locked buffer first, readable
 * in place through pe_batch_results until the next pe_place_batch. The host
 * preparation (fresh-memo feasibility tables, limit) is reused across calls
 * until a mutating call (set_state / set_job / stage_orders / select / ...). */
int pe_stage_orders(pe_stack* s, const uint32_t* orders, uint32_t n_evals, uint32_t n);
int pe_place_batch(pe_stack* s, uint32_t tg_index, uint32_t count, pe_placement* out,
                   uint32_t* placed);
/* Results of the last pe_place_batch: out[n_evals * count]; status[2 * e] =
 * placements of eval e, status[2 * e + 1] = its final StaticIterator offset. */
int pe_batch_results(const pe_stack* s, const pe_placement** out, const uint32_t** status,
                     uint32_t* n_evals, uint32_t* count);
/* Phases of the last pe_place_batch in ms: [0] host preparation, [1] kernel
 * (HIP events), [2] device-to-host result copy (HIP events), [3] call total. */
void pe_last_phase_ms(const pe_stack* s, double* out4);
/* SystemScheduler.computePlacements (scheduler_system.go:283-425) for one task
 * group over every row of the SetNodes list: one single-node Select per row.
 * out_row_score[n] = FinalScore or NaN when filtered/exhausted;
 * out_status[n] = 0 placed, 1 filtered, 2 exhausted. Commits placed allocs.
 * Both arrays NULL: the results stay in the engine's page-locked staging,
 * read through pe_system_results (no copy into caller memory). */
int pe_system_place(pe_stack* s, uint32_t tg_index, double* out_score,
                    uint8_t* out_status, uint32_t* placed);
/* The last pe_system_place's results in the engine's staging (score[n],
 * status[n], as above), valid until the next pe_system_place on the handle. */
int pe_system_results(const pe_stack* s, const double** score, const uint8_t** status, uint32_t* n);
/* SystemScheduler.computePlacements (scheduler_system.go:283-425) for a job
 * with several task groups, in one pass. The call covers every position pos of
 * the SetNodes list, in order, and within a position every listed group k, in
 * list order: each (position, group) pair is one single-node Select of
 * tg_indices[k] on list[pos], followed on an option by Plan.AppendAlloc.
 * Nodes do not interact under the refusals below, so every result and every
 * later observable state (node records, the job's and each group's collision
 * counts and device free counts, dynamic ports and bandwidth, the plan, the
 * EvalEligibility memo and its log) equals that of the sequence
 * pe_system_place(tg_indices[0]), ..., pe_system_place(tg_indices[n_tg-1]) on
 * the same handle. The reference visits the groups of one node in Go map order
 * (diffSystemAllocsForNode ranges over a map), so any fixed group order is one
 * of the reference's answers.
 *
 * Results, entry e = pos * n_tg + k:
 *   out_status2: 2 bits per entry, four entries per byte: entry e in byte
 *     e >> 2 at bits 2 * (e & 3); pe_system_place's codes (0 placed,
 *     1 filtered, 2 exhausted); unused bits of the last byte are 0.
 *     (n * n_tg + 3) / 4 bytes.
 *   out_score: dense, the FinalScore of the placed entries only, in increasing
 *     e; sized n * n_tg by the caller, the first *placed values are written.
 *   counts[3 * k + code]: entries of group k per outcome (queuedAllocs and
 *     CoalescedFailures of computePlacements).
 * out_score, out_status2 and counts are all NULL or all set; NULL: the results
 * stay in the engine's page-locked staging, read through
 * pe_system_groups_results, valid until the next pe_system_place* call on the
 * handle. An empty list returns PE_OK with *placed == 0.
 *
 * PE_EINVAL (nothing changed): n_tg == 0, an index out of range, a group
 * listed twice, a mixed NULL / non-NULL set of output arrays. PE_ESTATE: not a
 * system stack. PE_EUNSUPPORTED (checked before anything changes; the
 * per-group or per-Select calls answer): duplicate rows in the list,
 * preemption enabled on the stack, distinct_property at job or group level, a
 * reserved-cores ask, static ports in a listed group, a task network on a
 * snapshot with multi-NIC nodes, device asks in more than one listed group,
 * pe_set_metrics on, a handle over several devices, a listed group whose own
 * unsupported reason is set. */
int pe_system_place_groups(pe_stack* s, const uint32_t* tg_indices, uint32_t n_tg,
                           double* out_score, uint8_t* out_status2,
                           uint32_t* counts, uint32_t* placed);
/* The last pe_system_place_groups' results in the engine's staging (layout as
 * above; score holds *placed values). */
int pe_system_groups_results(const pe_stack* s, const double** score, const uint8_t** status2,
                             const uint32_t** counts, uint32_t* n, uint32_t* n_tg, uint32_t* placed);
/* pe_system_place_groups on a stack with preemption enabled
 * (PreemptionConfig.SystemSchedulerEnabled, the reference's default): the same
 * walk, every position of the SetNodes list in order and every listed group
 * in list order within it, each pair one single-node Select on the system
 * stack. A plain BinPack that fails its fit goes into BinPack with evict
 * (stack.go:267-278, rank.go:193-527, preemption.go); an option is followed
 * by Plan.AppendAlloc and by Plan.AppendPreemptedAlloc of each preempted
 * alloc. out_status2, out_score, counts and *placed have
 * pe_system_place_groups' layout and carry the final outcome: a pair placed by
 * eviction counts as placed and its score is the eviction Select's FinalScore.
 * NULL arrays leave the results in staging (pe_system_groups_results serves
 * both calls). Every result and every later observable state (node records,
 * collision counts, device free counts, ports and bandwidth, the plan and its
 * preemptions, the EvalEligibility memo and its log) equals that of the
 * node-major per-Select loop and that of pe_system_place(tg_indices[0]), ...,
 * pe_system_place(tg_indices[n_tg-1]) on the same handle. With preemption off
 * on the stack the call is pe_system_place_groups and preempts nothing.
 *
 * PE_EINVAL / PE_ESTATE as pe_system_place_groups. PE_EUNSUPPORTED (checked
 * before anything changes): everything pe_system_place_groups refuses except
 * preemption itself, and: a non-terminal alloc in the snapshot with
 * max_parallel > 0 whose job priority is at least 10 below the placing job's
 * (its penalty reads the plan's preemption counts, which other nodes grow); a
 * snapshot outside the on-device eviction limits; a device ask in a listed
 * group while a non-terminal alloc holds two device entries of one device
 * group; several task networks in a listed group; a listed node whose alloc
 * count, or that count plus the plan's placements on it plus n_tg, is beyond
 * the widest eviction width (1024 allocs, 2048 proposed allocs). */
int pe_system_place_groups_preempt(pe_stack* s, const uint32_t* tg_indices, uint32_t n_tg,
                                   double* out_score, uint8_t* out_status2,
                                   uint32_t* counts, uint32_t* placed);
/* The preempted allocs of the last pe_system_place_groups_preempt, a CSR in the
 * engine's page-locked staging, valid until the next pe_system_place* call on
 * the handle: entries[n_entries] holds the entry indices e = pos * n_tg + k
 * that preempted something, increasing; allocs[off[i] .. off[i + 1]) their
 * alloc-table rows in the order pe_select's record lists them (increasing slot
 * of the node's alloc list). No PE_MAX_PREEMPT cap. PE_ESTATE: no such call
 * yet, or a pe_system_place* call since. */
int pe_system_groups_preempted(const pe_stack* s, const uint32_t** entries, const uint32_t** off,
                               const uint32_t** allocs, uint32_t* n_entries);
/* pe_system_place_groups_preempt for a caller that keeps AllocMetric
 * (pe_set_metrics on), as SystemScheduler.computePlacements does
 * (scheduler_system.go:283-425: every placed alloc carries ctx.Metrics(), the
 * first failed placement of a task group is kept whole in failedTGAllocs, later
 * ones only count). The walk, the result layout, the staging rules, the
 * argument errors and the refusals are pe_system_place_groups_preempt's, minus
 * the refusal of pe_set_metrics; it runs on a preempting and on a
 * non-preempting system stack; pe_system_groups_results and
 * pe_system_groups_preempted serve it too. With metrics off it is
 * pe_system_place_groups_preempt. With metrics on every result and every later
 * observable state equals that of the node-major per-Select loop with metrics
 * on, the reference memo behind the "computed class ineligible" reasons of
 * later Selects included; the filtered reasons of this call's own Selects are
 * not returned (computePlacements drops a filtered nil Select, :311-324), and
 * there is no "last Select": pe_last_metrics answers PE_ESTATE after it.
 *
 * What the caller needs of each Select's maps comes from pe_system_groups_metrics:
 *   failures[k], k < n_tg: the first exhausted Select of listed group k in walk
 *     order (the smallest list position whose entry of group k is exhausted in
 *     the final outcome). That Select's maps are NodesEvaluated 1,
 *     NodesExhausted 1, ClassExhausted{node_class: 1} and
 *     DimensionExhausted{dimension: 1}: the dimension that Select saw, after
 *     the earlier groups' placements and evictions on the node. dimension is a
 *     key as pe_metric_count.key (pe_metric_string gives its text); it and
 *     node_class are PE_NONE where that Select recorded none (an empty
 *     NodeClass; an eviction Select that gave the node up without
 *     ExhaustedNode, rank.go:283-300). Later exhausted entries are
 *     counts[3 * k + 2] - 1 coalesced failures.
 *   *dev_group: the listed index of the group whose ask scores devices (a
 *     device request with affinities), or -1. When >= 0, dev_binpack[pos] and
 *     dev_devices[pos] (*n values each, by list position) are that group's
 *     "binpack" and "devices" ScoreNode values where its entry is placed,
 *     plainly or by eviction, NaN elsewhere; its NormScore is the entry's
 *     FinalScore. When -1 both pointers are NULL: every placed entry's
 *     ScoreMetaData is one item, its node with "binpack" = NormScore =
 *     FinalScore (the SystemStack ranks with BinPack alone, stack.go:277-281).
 * The arrays are page-locked staging, valid until the next pe_system_place*
 * call on the handle. PE_ESTATE: no pe_system_place_groups_metrics call with
 * metrics on yet, or a pe_system_place* call since. */
typedef struct pe_sysg_failure {
    uint32_t pos;          /* list position; PE_NONE: group k has no exhausted entry (dimension and node_class PE_NONE too) */
    uint32_t dimension;    /* DimensionExhausted key, or PE_NONE */
    uint32_t node_class;   /* ClassExhausted key (the node's NodeClass string id), or PE_NONE */
    uint32_t reserved;     /* 0 */
} pe_sysg_failure;
int pe_system_place_groups_metrics(pe_stack* s, const uint32_t* tg_indices, uint32_t n_tg,
                                   double* out_score, uint8_t* out_status2,
                                   uint32_t* counts, uint32_t* placed);
int pe_system_groups_metrics(const pe_stack* s, const pe_sysg_failure** failures,
                             int32_t* dev_group, const double** dev_binpack, const double** dev_devices,
                             uint32_t* n);
/* Full-scan Select sharded over GPUs (one process per GPU, each holding the
 * same snapshot, job, SetNodes list and plan). Each rank sweeps
 * the snapshot rows [row_begin, row_end) it owns into a pe_shard_rec: the
 * LimitIterator/MaxScoreIterator state of its rows (max score and its earliest
 * visit ranks, the first three non-positive options, option / filter / exhaust
 * counts), which merges associatively. After one all-gather of the records,
 * every rank calls pe_select_merge with all of them and gets the same Select
 * result (stack.go:117-179 with limit MaxInt32; a full pass leaves the cursor
 * unchanged), then commits it with pe_commit. Needs a full pass (affinities or
 * spreads), a visit list without repeated rows and no distinct_property. */
typedef struct pe_shard_rec { uint8_t bytes[80]; } pe_shard_rec;
int pe_select_shard(pe_stack* s, uint32_t tg_index, uint32_t row_begin, uint32_t row_end, pe_shard_rec* out);
int pe_select_merge(pe_stack* s, uint32_t tg_index, const pe_shard_rec* recs, uint32_t n_recs,
                    pe_ranked_node* out);
/* Milliseconds spent in device kernels by the last pe_place / pe_system_place
 * (HIP events on the engine's stream). */
double pe_last_kernel_ms(const pe_stack* s);
/* Algorithmic HBM bytes per node of the last full-scan sweep Select (73 with
 * the verdict byte, 76 with the folded per-node score word), 0 if none ran. */
uint32_t pe_last_sweep_bytes(const pe_stack* s);
/* Per-kernel device time of the windowed count loop (measurement aid; off by
 * default, or PE_KERNEL_SPLIT=1 in the environment at pe_stack_create): with it
 * on, the chain path records HIP events between its kernels and
 * pe_last_kernel_split writes the last launch's ms4 = {k_base, k_chain, k_emit,
 * k_emit_writeback}; PE_ESTATE when the last pe_place / Select ran no chain.
 * pe_system_place_groups_preempt and pe_system_place_groups_metrics on a
 * preempting stack record them too:
 * ms4 = {stopping pass, eviction walk at the first width, compaction, the
 * time on the stream from there to the end of the last relaunch at a wider
 * width (host waits between the rounds included); exactly 0 when no node
 * needed a wider width}. pe_last_kernel_ms covers the first round only. */
int pe_set_kernel_split(pe_stack* s, int on);
int pe_last_kernel_split(const pe_stack* s, double* ms4);
/* AllocMetric maps (structs.go:9826-10026) of Selects: ClassFiltered,
 * ConstraintFiltered, ClassExhausted, DimensionExhausted — what
 * `ctx.Metrics()` holds after GenericStack.Select (FilterNode / ExhaustedNode,
 * structs.go:9907-9937). Off by default; switch on before the first Select of
 * an evaluation (the maps depend on the EvalEligibility memo history).
 * Available for every Select: plain, with preferred nodes, and with Preempt
 * (BinPack with evict per visited row, k_evict_trace). */
int pe_set_metrics(pe_stack* s, int on);
/* The last Select's maps as text lines "KIND\tKEY\tCOUNT\n", KIND one of
 * CF / KF / CE / DE, keys sorted. Writes at most cap bytes (NUL-terminated) and
 * returns the bytes needed, or PE_ESTATE when the last Select has none. */
int64_t pe_last_metrics(const pe_stack* s, char* buf, size_t cap);
/* The same maps in binary form (what the Go shim turns into AllocMetric
 * without parsing text): count entries {kind, key, count} and the
 * ScoreMetaData items in GetItemsReverse order (NormScore descending, Go's
 * heap order for equal scores). A key without PE_METRIC_ENGINE_KEY is a
 * string id of the caller's table (the node classes of ClassFiltered /
 * ClassExhausted); a key with it names an engine string (checker reasons,
 * dimensions: pe_metric_string), stable for the handle's life. The arrays
 * stay valid until the next Select or state call. PE_ESTATE when the last
 * Select has no maps. */
#define PE_METRIC_ENGINE_KEY 0x80000000u
#define PE_METRIC_CLASS_FILTERED 1u       /* AllocMetric.ClassFiltered[key]       */
#define PE_METRIC_CONSTRAINT_FILTERED 2u  /* AllocMetric.ConstraintFiltered[key]  */
#define PE_METRIC_CLASS_EXHAUSTED 3u      /* AllocMetric.ClassExhausted[key]      */
#define PE_METRIC_DIMENSION_EXHAUSTED 4u  /* AllocMetric.DimensionExhausted[key]  */
typedef struct pe_metric_count {
    uint32_t kind;    /* PE_METRIC_* */
    uint32_t key;     /* string id (see above) */
    uint32_t count;
} pe_metric_count;
/* NodeScoreMeta.Scores names (the ScoreNode scorers, in the order they ran) */
#define PE_SCORER_BINPACK 0u
#define PE_SCORER_DEVICES 1u
#define PE_SCORER_JOB_ANTI_AFFINITY 2u
#define PE_SCORER_RESCHEDULE_PENALTY 3u   /* "node-reschedule-penalty" */
#define PE_SCORER_NODE_AFFINITY 4u
#define PE_SCORER_ALLOCATION_SPREAD 5u
#define PE_SCORER_PREEMPTION 6u
typedef struct pe_metric_score {
    int32_t row;                      /* NodeID: the node table row */
    uint32_t n_scores;
    double norm;                      /* NormScore */
    uint8_t scorer[PE_MAX_SCORES];    /* PE_SCORER_* */
    double score[PE_MAX_SCORES];
} pe_metric_score;
int pe_last_metrics_bin(const pe_stack* s, const pe_metric_count** counts, uint32_t* n_counts,
                        const pe_metric_score** scores, uint32_t* n_scores);
/* The text of metric key `key` (an engine string or a caller string id):
 * writes at most cap bytes (NUL-terminated), returns the bytes needed or
 * PE_EINVAL for an unknown key. Scorer names: pe_scorer_name.
 * The engine's key table only grows. Most reasons are a fixed few texts; the
 * CSI plugin reasons of pe_place_csi_metrics (PE_CSI_NO_PLUGIN, _UNHEALTHY,
 * _MAX_VOLUMES) name the plugin and the node, so they add at most one string
 * per (plugin, node) pair to a handle. */
int64_t pe_metric_string(const pe_stack* s, uint32_t key, char* buf, size_t cap);
const char* pe_scorer_name(uint32_t scorer);
/* What update i's Select left in its AllocMetric maps (pe_last_metrics_bin
 * after that Select in the per-call sequence). A Select over one node records
 * at most one key per map, each with count 1, or one ScoreMetaData item. Keys
 * are pe_metric_count's (pe_metric_string resolves them). */
typedef struct pe_inplace_metric {
    uint32_t class_key;   /* ClassFiltered (status 1) / ClassExhausted (status 2) key, or PE_NONE: a node
                           * without a NodeClass, or no key recorded (below) */
    uint32_t reason_key;  /* ConstraintFiltered (status 1) / DimensionExhausted (status 2) key, or PE_NONE:
                           * on a preempting stack, a BinPack with evict that gave the node up without
                           * ExhaustedNode (a network or device preemption that found nothing) */
    uint32_t score;       /* status 0: index into scores[]; otherwise PE_NONE */
} pe_inplace_metric;
/* The maps of the last pe_inplace_update_metrics that ran with metrics on:
 * m[n] by list position, scores[n_scores] one item per status-0 update in list
 * order (the scorers in the order pe_last_metrics_bin lists them; an evicting
 * update carries the eviction Select's named scores). Page-locked staging,
 * valid until the next pe_inplace_update* call on the handle. PE_ESTATE: no
 * such call yet, it ran with metrics off, or a pe_inplace_update* call since. */
int pe_inplace_metrics(const pe_stack* s, const pe_inplace_metric** m, uint32_t* n,
                       const pe_metric_score** scores, uint32_t* n_scores);
/* EvalEligibility (scheduler/context.go:190-356) as the reference chain would
 * hold it after this evaluation's Selects: the job-level and per task group
 * ComputedClassFeasibility entries FeasibilityWrapper.Next writes for every
 * node the chain pulls (feasible.go:1061-1153). createBlockedEval /
 * ReblockEval read GetClasses() and HasEscaped() from it
 * (generic_sched.go:177-181, 193-203); the shim mirrors the entries into
 * ctx.Eligibility() after each Select (changed_only = 1 returns the entries
 * set or changed since the last call that fit in `cap`). *n receives the
 * number of entries; *flags bit PE_ELIG_ESCAPED = HasEscaped(). */
#define PE_CLASS_INELIGIBLE 1   /* EvalComputedClassIneligible */
#define PE_CLASS_ELIGIBLE 2     /* EvalComputedClassEligible */
#define PE_ELIG_ESCAPED 1u
typedef struct pe_class_feas {
    uint32_t task_group;      /* PE_NONE: EvalEligibility.job; else the task group name (str id) */
    uint32_t computed_class;  /* Node.ComputedClass (str id, as in pe_node_table.computed_class) */
    uint32_t status;          /* PE_CLASS_INELIGIBLE / PE_CLASS_ELIGIBLE */
} pe_class_feas;
int pe_get_eligibility(pe_stack* s, uint32_t changed_only, pe_class_feas* out, uint32_t cap, uint32_t* n,
                       uint32_t* flags);
/* After the Go chain answered a Select (PE_EUNSUPPORTED): its ctx.Eligibility()
 * entries become the engine's memo, so later Selects filter and decide classes
 * exactly as the chain would (EvalEligibility is shared by the two stacks). */
int pe_put_eligibility(pe_stack* s, const pe_class_feas* in, uint32_t n);
/* The GenericStack iterator state that persists between Selects:
 * StaticIterator.offset (feasible.go:75-117) and the LimitIterator limit
 * (stack.go:81-90; latched to MaxInt32 by task groups with affinities or
 * spreads, stack.go:165-167). Before the shim's fallback GenericStack answers
 * a PE_EUNSUPPORTED Select it takes both from pe_get_cursor; afterwards
 * pe_set_cursor hands the chain's offset and limit back, with the task group
 * it selected for (its SpreadIterator.SetTaskGroup adds the group's spread
 * weights to sumSpreadWeights, spread.go:232-257), or PE_NONE. */
int pe_get_cursor(const pe_stack* s, uint32_t* offset, uint32_t* limit);
/* ---- zero-crossing served Selects --------------------------------------------
 * GenericScheduler.computePlacements (generic_sched.go:552-627) calls Select
 * once per placement, retries a nil one with Preempt=true when preemption is
 * enabled (selectNextOption, :773-792), and the shim commits each option
 * (Plan.AppendAlloc + AppendPreemptedAlloc, :627, :794-816): two or three cgo
 * crossings per placement. After the first plain Select of a task group the
 * engine already holds the records of the group's count loop (DESIGN.md §12,
 * §25): with preemption enabled, a placement that evicts is two records, the
 * plain Select's nil and the Preempt retry's option (flag PE_SPEC_PREEMPT,
 * its PreemptedAllocs in pre_allocs). This view lets the caller answer those
 * Selects and Commits from host memory and cross into C only when it
 * deviates. One view per handle, used from the handle's thread.
 *
 *   Select(tg, opts) with no preferred / penalty nodes, when v->n_rec > 0,
 *     tg == v->tg_index, v->served == v->confirmed, v->served < v->n_rec and
 *     (v->recs[v->served].flags & PE_SPEC_PREEMPT) is set exactly when
 *     opts.Preempt is:
 *       the result is v->recs[v->served], with PreemptedAllocs
 *       v->pre_allocs[v->pre_off[k] .. v->pre_off[k + 1]) for k = v->served
 *       (none when v->pre_off is NULL); then v->served++, and for a nil
 *       result (row < 0, which no Commit follows) also v->confirmed++;
 *   Commit(tg, row) / CommitPreempt(tg, row, list), when v->served ==
 *     v->confirmed + 1, tg == v->tg_index, row == v->recs[v->served - 1].row
 *     and the list is that record's PreemptedAllocs in its order (empty for
 *     Commit): v->confirmed++;
 *   anything else goes through the entry points below, which first take the
 *     counters over, so the engine state is exactly what the sequential calls
 *     would have produced; they may replace or withdraw the records (v->epoch
 *     changes; v->n_rec 0: nothing to serve).
 * A record the engine returned through pe_select may be confirmed through the
 * view as well. With pe_set_metrics on, the runs still publish records, each
 * with its AllocMetric maps. A served record is the leading part of pe_ranked_node (row ..
 * new_offset) plus the device offers; served Selects never reserve cores.
 * Replaces: the Select / Commit crossings of computePlacements' loop. */
#define PE_SPEC_PREEMPT 1u   /* pe_spec_rec.flags: answers the Select with Preempt=true */
typedef struct pe_spec_rec {
    int32_t row;
    uint32_t n_scores;
    double final_score;
    double scores[PE_MAX_SCORES];
    uint32_t nodes_evaluated, nodes_filtered, nodes_exhausted, new_offset;
    uint32_t n_device_offers;
    uint16_t device_offer_group[PE_MAX_DEVICE_REQ];
    uint32_t flags;               /* PE_SPEC_* */
} pe_spec_rec;
typedef struct pe_spec_view {
    uint32_t epoch;               /* engine: changes whenever recs / n_rec / tg_index change */
    uint32_t tg_index;            /* the task group the records answer */
    uint32_t n_rec;               /* records [0, n_rec) are valid */
    uint32_t pad0;
    const pe_spec_rec* recs;      /* the run's records in Select order */
    uint32_t served;              /* caller and engine: Selects answered from recs */
    uint32_t confirmed;           /* caller and engine: records settled (Commits, nils) */
    const uint32_t* pre_off;      /* [n_rec + 1] or NULL: record k's PreemptedAllocs ... */
    const uint32_t* pre_allocs;   /* ... are pre_allocs[pre_off[k] .. pre_off[k + 1]) (alloc-table rows) */
    /* With pe_set_metrics on: record k's AllocMetric maps, what
     * pe_last_metrics_bin returns after that Select, are
     * mcounts[mcounts_off[k] .. mcounts_off[k + 1]) and
     * mscores[mscores_off[k] .. mscores_off[k + 1]); NULL when the records
     * carry none. */
    const pe_metric_count* mcounts;
    const uint32_t* mcounts_off;
    const pe_metric_score* mscores;
    const uint32_t* mscores_off;
} pe_spec_view;
pe_spec_view* pe_spec_view_get(pe_stack* s);
/* SystemScheduler.computePlacements (scheduler_system.go:283-425) runs, for
 * every node, SetNodes([node]) + Select + (on an option) Plan.AppendAlloc:
 * three crossings per node (scheduler_system.go:289-302). From a task group's
 * third single-node Select the engine answers from a per-row cache filled by
 * one k_system pass; this view exposes that cache so the
 * caller answers the triples from host memory and logs them, and crosses into
 * C only when it deviates. One view per handle, used from its thread.
 *
 *   SetNodes([row]) + Select(tg) with no options, when v->n_rows > 0,
 *     tg == v->tg_index, row < v->n_rows, v->n_log < v->log_cap and
 *     outcome[row] is servable: a finite double is an option on `row` with
 *     that FinalScore (one score, nodes_evaluated 1); a NaN whose low two bits
 *     are 1 (filtered) or 2 (exhausted) is nil with nodes_filtered /
 *     nodes_exhausted 1 -- unless v->preempt and it is exhausted (BinPack with
 *     eviction answers: go to C); low bits 3 (PE_SYS_STALE) mean the row
 *     changed since the pass: go to C. Then v->log[v->n_log++] = row, with
 *     PE_SYS_NIL set for a nil answer;
 *   the Commit of that option: v->log[v->n_log - 1] |= PE_SYS_COMMITTED and
 *     outcome[row] = PE_SYS_STALE (a committed row is not served again);
 *   anything else goes through the entry points, which first take the log
 *     over (the engine state is then exactly what the sequential calls would
 *     have produced); they may withdraw the view (v->epoch changes; v->n_rows 0).
 * Replaces: the SetNodes / Select / Commit crossings of the per-node loop. */
#define PE_SYS_NIL (1u << 31)
#define PE_SYS_COMMITTED (1u << 30)
#define PE_SYS_ROW_MASK 0x3FFFFFFFu
#define PE_SYS_STALE 0x7FF8000000000003ull
typedef struct pe_system_view {
    uint32_t epoch;               /* engine: changes whenever outcome / n_rows / tg_index change */
    uint32_t tg_index;            /* the task group the outcomes answer */
    uint32_t n_rows;              /* 0: nothing to serve */
    uint32_t log_cap;             /* entries log[] can hold */
    uint64_t* outcome;            /* [n_rows] per row (bits of a double) */
    uint32_t* log;                /* [log_cap] served Selects in order, written by the caller */
    uint32_t n_log;               /* caller and engine: entries written / taken over */
    uint32_t preempt;             /* nonzero: exhausted rows go to the engine */
    /* With pe_set_metrics on (NULL otherwise): a served Select's AllocMetric
     * maps (scheduler_system.go:334-337), which the caller assembles from
     * per-row entries as FeasibilityWrapper and BinPack would have filled
     * them (feasible.go:1061-1153):
     *   option: ScoreMetaData = [{NodeID of row, NormScore = the outcome's
     *     FinalScore, Scores = {"binpack": mscore[row]}}];
     *   filtered: ConstraintFiltered[key]++ with key = mkey[row], except when
     *     c = mclass[row] != PE_NONE and mfailed[c] is set: key =
     *     mkey_ineligible ("computed class ineligible"); then mfailed[c] = 1
     *     when c != PE_NONE (the EvalEligibility memo of the row's class);
     *   exhausted: DimensionExhausted[mkey[row]]++;
     *   filtered / exhausted: ClassFiltered / ClassExhausted[mnode_class[row]]++
     *     unless it is PE_NONE (a node without NodeClass).
     * Keys as pe_metric_count.key (pe_metric_string). */
    const uint32_t* mkey;
    const uint32_t* mclass;
    uint8_t* mfailed;             /* caller and engine: per memo class */
    const double* mscore;
    const uint32_t* mnode_class;
    uint32_t mkey_ineligible;
    uint32_t pad1;
} pe_system_view;
pe_system_view* pe_system_view_get(pe_stack* s);
int pe_set_cursor(pe_stack* s, uint32_t tg_index, uint32_t offset, uint32_t limit);
/* ---- CSI volumes (CSIVolumeChecker, feasible.go:209-337) ----------------------
 * The CSI state of the snapshot, flattened by the caller. Every string field
 * is an id of the snapshot's table (`strs` extends it, as in pe_set_job).
 *   per node (CSR, off[n_nodes + 1]): Node.CSINodePlugins: the plugin id (the
 *     map key), Healthy, NodeInfo.MaxVolumes;
 *   per volume: ID, Namespace, PluginID, ReadSchedulable(), WriteSchedulable(),
 *     WriteFreeClaims(), and (CSR, claim_off[n_volumes + 1]) the allocs of
 *     WriteAllocs as (Namespace, JobID) of state.AllocByID, both PE_NONE for an
 *     alloc the state no longer has;
 *   per node (CSR): the indices into the volume table of the volumes
 *     state.CSIVolumesByNodeID yields (state_store.go:2240-2280).
 * n_nodes must equal the snapshot's node count. The table belongs to the
 * snapshot: pe_set_state, pe_update_nodes and pe_update_allocs drop it;
 * pe_reset_plan keeps it. table == NULL drops it. */
typedef struct pe_csi_table {
    uint32_t n_nodes;
    uint32_t n_volumes;
    const uint32_t* plug_off; const uint32_t* plug_id; const uint8_t* plug_healthy;
    const int64_t* plug_max_volumes;
    const uint32_t* vol_id; const uint32_t* vol_ns; const uint32_t* vol_plugin;
    const uint8_t* vol_read_ok; const uint8_t* vol_write_ok; const uint8_t* vol_write_free;
    const uint32_t* claim_off; const uint32_t* claim_ns; const uint32_t* claim_job;
    const uint32_t* node_vol_off; const uint32_t* node_vol_index;
} pe_csi_table;
int pe_set_csi(pe_stack* s, const pe_strtab* strs, const pe_csi_table* table);
/* The CSI volume requests of task group tg_index (TaskGroup.Volumes of type
 * csi), after pe_set_job. The reference ranges over a Go map; the list order
 * given here replaces it: the first failing request, in this order, names the
 * reason. At most PE_MAX_CSI_REQ. A group with has_csi_volumes set and no
 * table or no requests is refused (PE_EUNSUPPORTED "CSI volumes"). With both,
 * pe_select (plain: no preferred nodes, no Preempt, pe_set_metrics off) and
 * pe_system_place place it, and so does pe_place_csi (below), the count loop
 * for such a group; every other placing call refuses it before
 * anything changes. On a generic stack pe_select may itself return
 * PE_EUNSUPPORTED with the cursor, the memo and the plan untouched: the
 * reference would resume its walk past an unavailable node of a class already
 * memoised eligible (select.go:59-67), or a full pass (a group with affinities
 * or spreads) ends at such a node; the engine leaves both to the chain
 * (pe_place_csi answers the first of the two). */
#define PE_MAX_CSI_REQ 16
typedef struct pe_csi_request {
    uint32_t source;      /* VolumeRequest.Source (str id) */
    uint32_t read_only;   /* VolumeRequest.ReadOnly */
    uint32_t per_alloc;   /* VolumeRequest.PerAlloc: the source takes the "[idx]" suffix */
} pe_csi_request;
int pe_set_csi_requests(pe_stack* s, uint32_t tg_index, const pe_csi_request* reqs, uint32_t n);
/* AllocSuffix of the alloc name the next Selects of the group place
 * (funcs.go:402): per_alloc sources become source + "[idx]". 0 after
 * pe_set_csi_requests. */
int pe_csi_alloc_index(pe_stack* s, uint32_t tg_index, uint32_t idx);
/* The engine's availability column of the group, one code per snapshot row:
 * 0 available, else request_index << 3 | reason with the reason numbered as
 * isFeasible's checks run (feasible.go:293-333): 1 volume not found, 2 the
 * node lacks the volume's plugin, 3 plugin unhealthy, 4 MaxVolumes reached,
 * 5 no read claims, 6 no write claims, 7 volume in use by another job. */
#define PE_CSI_NOT_FOUND 1u
#define PE_CSI_NO_PLUGIN 2u
#define PE_CSI_UNHEALTHY 3u
#define PE_CSI_MAX_VOLUMES 4u
#define PE_CSI_NO_READ 5u
#define PE_CSI_NO_WRITE 6u
#define PE_CSI_IN_USE 7u
int pe_csi_check(pe_stack* s, uint32_t tg_index, uint16_t* codes);
/* Measurement aid: device time of the last k_csi_avail launch in ms, by HIP
 * events that are recorded only with PE_CSI_TIME=1 in the environment at
 * pe_stack_create; 0 otherwise. */
double pe_csi_last_ms(pe_stack* s);
/* computePlacements' loop for `count` fresh placements of a task group with CSI
 * requests: for i in [0, count): SetVolumes(alloc name with index alloc_idx[i]),
 * Select, AppendAlloc; ends at the first nil option, as pe_place does.
 * alloc_idx == NULL: every placement takes the index that pe_csi_alloc_index holds.
 * Afterwards the cursor, the memo (pe_get_eligibility), the plan and the records
 * out[0..*placed] (the failed Select's too, if any) are what the per-placement
 * sequence pe_csi_alloc_index / pe_select / pe_commit would leave if the
 * reference chain answered the Selects that pe_select hands back: a stop while
 * LimitIterator holds skipped options resumes past the node here
 * (select.go:35-67). One launch of the loop kernel and one synchronisation per
 * call; one k_csi_avail launch per distinct set of resolved request records
 * among the call's alloc indices, at most PE_MAX_CSI_SETS.
 * On a group without CSI requests the call is pe_place. PE_EUNSUPPORTED, with
 * the cursor, the limit, the memo and the plan untouched: pe_set_metrics on, a
 * handle over several devices, a system stack, a preempting stack, computed
 * classes whose nodes differ in the group's checks, a group that runs full
 * passes (affinities, spreads, distinct_property, a latched limit;
 * pe_place_csi_full places all of these but distinct_property), whatever
 * pe_place refuses, more than PE_MAX_CSI_SETS distinct record sets, and a
 * count beyond the overlay of one launch. */
#define PE_MAX_CSI_SETS 8
int pe_place_csi(pe_stack* s, uint32_t tg_index, uint32_t count, const uint32_t* alloc_idx, pe_ranked_node* out,
                 uint32_t* placed);
/* pe_place_csi for a group that runs full passes: node affinities or spreads at
 * job or group level, or a limit an earlier Select of a sibling group latched
 * to MaxInt32 (stack.go:165-167). Arguments, records and contract are
 * pe_place_csi's: alloc_idx NULL means the held index, the failed Select's
 * record is written, the group's alloc index afterwards is the last attempted
 * placement's. Each Select may consume the whole list from the cursor, wrapping
 * (StaticIterator.seen is reset per Select); it ends at a stop with no skipped
 * option pending, or at the end of the list, and the next one starts after that
 * position; a Select that starts on a stop is nil and ends the loop. Afterwards
 * the cursor, the limit (latched as Select latches it), the memo, the plan,
 * the property-set counts behind later spread scores and every record are what
 * the reference chain leaves after computePlacements' loop. One launch of
 * k_csi_full and one synchronisation per call, the k_csi_avail and k_csi_first
 * launches as pe_place_csi.
 * On every other group the call is pe_place_csi (and so pe_place without CSI
 * requests). PE_EUNSUPPORTED, with cursor, limit, memo, plan and alloc index
 * untouched: pe_place_csi's list without its full-pass row, distinct_property
 * at job or group level (it filters above the wrapper), and spread values
 * cleared by plan stops (the counts are rebuilt on the host per commit).
 * pe_csi_place_ms then reports k_csi_full in ms2[1]. */
int pe_place_csi_full(pe_stack* s, uint32_t tg_index, uint32_t count, const uint32_t* alloc_idx, pe_ranked_node* out,
                      uint32_t* placed);
/* Lanes of k_csi_full's one workgroup: a placement's passes take the visit list
 * in chunks of this many positions (tests choose list lengths around it).
 * Stateless, needs no device. */
uint32_t pe_csi_full_block(void);
/* pe_place_csi with AllocMetric kept: what GenericScheduler.computePlacements
 * stores per placed alloc and, for the nil Select that ends the loop, in
 * failedTGAllocs (generic_sched.go:552-627).
 * With pe_set_metrics off the call is pe_place_csi: same records, same
 * refusals, no further launch, and pe_place_csi_maps answers PE_ESTATE.
 * With it on, the records out[0..*placed] (the failed Select's too), the
 * cursor, the plan, the memo (pe_get_eligibility), the group's alloc index and
 * every later observable state are exactly what pe_place_csi leaves with
 * metrics off. pe_place_csi_maps then gives record k's AllocMetric maps as
 * counts[counts_off[k] .. counts_off[k + 1]) and scores[scores_off[k] ..
 * scores_off[k + 1]) for k < n_rec = the records written (the layout of
 * pe_spec_view.mcounts / mscores; keys as pe_metric_count.key). They include
 * what only CSIVolumeChecker.Feasible records (feasible.go:251-259): for every
 * node the checker fails, ClassFiltered[NodeClass] and
 * ConstraintFiltered[reason], the reason being pe_csi_reason_text's for the
 * failing request, its volume and (plugin reasons) the node. The maps stay
 * valid until the next placing or state call on the handle. pe_last_metrics*
 * answers PE_ESTATE afterwards, as after the other batched metrics calls, and
 * the metrics shadow of the memo advances as the per-Select sequence would
 * advance it. The loop kernel additionally logs one byte per consumed visit
 * position into mapped page-locked memory; the maps then cost one host walk
 * over the consumed windows and one batched trace (everything it returns in
 * one copy): two stream synchronisations per call, the loop's and the trace's,
 * and no k_csi_avail launch beyond pe_place_csi's. A call that needs a larger
 * log or trace buffer than the handle has allocated so far also pays that
 * allocation, which waits for the device like any other.
 * pe_set_metrics must be on from the job's first Select, as for the other
 * metrics calls: the maps follow the metrics shadow of the memo, which only
 * Selects made with metrics on advance. A caller that places the group with
 * metrics off and then turns them on may get PE_EINTERNAL from this call after
 * the loop has committed (the kernel's stops follow the real memo).
 * PE_EUNSUPPORTED, all before anything changes (cursor, limit, memo, its
 * metrics shadow and plan untouched): pe_place_csi's list without its
 * pe_set_metrics row; with metrics on, a group without CSI requests (its maps
 * come from pe_select or the served view), static port asks, group networks on
 * multi-device nodes, reserved cores, two task groups of one name, and
 * count * (visit list length) above 2^24 (the trace log of one call; a caller
 * splits the loop). */
int pe_place_csi_metrics(pe_stack* s, uint32_t tg_index, uint32_t count, const uint32_t* alloc_idx,
                         pe_ranked_node* out, uint32_t* placed);
int pe_place_csi_maps(const pe_stack* s, const pe_metric_count** counts, const uint32_t** counts_off,
                      const pe_metric_score** scores, const uint32_t** scores_off, uint32_t* n_rec);
/* Measurement aid, recorded only with PE_CSI_TIME=1 in the environment at
 * pe_stack_create (no clock is read otherwise): the last pe_place_csi_metrics
 * call that ran with metrics on, by the host clock in microseconds: us4[0] the loop (launches to the end of
 * its synchronisation), [1] the host walk, [2] the trace (upload, launches,
 * download), [3] the maps; and the trace log bytes the call wrote (its
 * consumed positions). PE_ESTATE without PE_CSI_TIME=1 or when
 * pe_place_csi_maps would answer so. */
int pe_place_csi_metrics_stats(const pe_stack* s, double* us4, uint64_t* log_bytes);
/* pe_place_csi_full with AllocMetric kept: arguments, records and contract are
 * pe_place_csi_full's, the maps come back through pe_place_csi_maps (same
 * store, layout and generation rule as after pe_place_csi_metrics) and the
 * split through pe_place_csi_metrics_stats. A caller that keeps AllocMetric
 * calls this one entry for every CSI group:
 *  - pe_set_metrics off: the call is pe_place_csi_full, no further launch, and
 *    pe_place_csi_maps answers PE_ESTATE;
 *  - on, a group that runs no full passes under an unlatched limit: the call is
 *    pe_place_csi_metrics (a group without CSI requests is refused there);
 *  - on, a group with node affinities or spreads, or a latched limit: the
 *    records, cursor, limit, plan, memo, alloc index, property-set counts and
 *    every later observable state are pe_place_csi_full's with metrics off, bit
 *    for bit: the same kernel places (k_csi_full's metrics form), and beside it
 *    stores one trace log byte per classified position at (positions consumed
 *    so far) + (relative position), into mapped page-locked memory. A Select
 *    here may consume the whole list, so the log of one call holds up to
 *    count * (visit list length) bytes. The maps cost one host walk over the
 *    consumed windows (any length, wrapping) and one batched trace with every
 *    record's own spread tables: two stream synchronisations per call, as
 *    pe_place_csi_metrics. pe_last_metrics* answers PE_ESTATE afterwards.
 * pe_set_metrics must be on from the job's first Select (see above).
 * PE_EUNSUPPORTED, all before anything changes (cursor, limit, memo, its
 * metrics shadow, plan and alloc index untouched): pe_place_csi_full's list
 * without its pe_set_metrics row (distinct_property, spread values cleared by
 * plan stops, several devices, a system or preempting stack, non-uniform
 * classes, group networks on multi-device nodes, more than PE_MAX_CSI_SETS
 * record sets, a count beyond the overlay) and pe_place_csi_metrics' metrics-on
 * rows (static port asks, reserved cores, two task groups of one name,
 * count * (visit list length) above 2^24). */
int pe_place_csi_full_metrics(pe_stack* s, uint32_t tg_index, uint32_t count, const uint32_t* alloc_idx,
                              pe_ranked_node* out, uint32_t* placed);
/* pe_place_destructive with AllocMetric kept: what
 * GenericScheduler.computePlacements stores on each new alloc of its
 * destructive loop and, for the nil Select that ends it, in failedTGAllocs
 * (generic_sched.go:552-645). Arguments, records, contract and later state are
 * pe_place_destructive's.
 * With pe_set_metrics off the call is pe_place_destructive, and
 * pe_place_destructive_maps answers PE_ESTATE. (pe_place_destructive itself
 * keeps refusing a handle with metrics on.)
 * With it on, records, maps and every later observable state equal those of
 * the per-call sequence with metrics on: pe_plan_stop(&allocs[i], 1),
 * pe_select(tg, NULL), the maps read, then pe_commit, or
 * pe_plan_pop_update(allocs[i]) and a break. Later state includes the metrics
 * shadow of the memo, which the call advances as that sequence's Selects
 * would, the eligibility log, the cursor and the plan.
 * pe_place_destructive_maps gives record k's maps in pe_place_csi_maps'
 * layout: counts[counts_off[k] .. counts_off[k + 1]) and scores[scores_off[k]
 * .. scores_off[k + 1]) for k < n_rec = the records written. There is one map
 * set per returned record; the nil Select's are what the scheduler keeps in
 * failedTGAllocs, and that Select saw its own stop. The maps stay valid until
 * the handle's next mutating call. pe_last_metrics* answers PE_ESTATE after
 * the call, as after pe_place_csi_metrics.
 * The dynamic node columns are copied on the device before the loop, and the
 * maps then cost one host walk over the consumed windows and one batched trace
 * against that copy, which is told every stop record k's Select saw: two
 * stream synchronisations per call, whatever `n`.
 * PE_EINVAL, PE_ESTATE and n == 0 as pe_place_destructive. PE_EUNSUPPORTED,
 * checked before anything changes: pe_place_destructive's list without its
 * pe_set_metrics row. PE_EINTERNAL: a bounds guard of the loop kernel tripped;
 * pe_place_destructive_maps then answers PE_ESTATE. */
int pe_place_destructive_metrics(pe_stack* s, uint32_t tg_index, const uint32_t* allocs, uint32_t n,
                                 pe_ranked_node* out, uint32_t* placed);
int pe_place_destructive_maps(const pe_stack* s, const pe_metric_count** counts, const uint32_t** counts_off,
                              const pe_metric_score** scores, const uint32_t** scores_off, uint32_t* n_rec);
/* pe_place_destructive for a group that runs full passes: node affinities or
 * spreads (target or even, at job or group level, attributes that some nodes
 * lack included), or a plain group under a limit that a sibling group's Select
 * latched to MaxInt32. Arguments and records are pe_place_destructive's. On a
 * group that runs no full passes under an unlatched limit the call is
 * pe_place_destructive, so a caller that keeps no AllocMetric uses this one
 * entry for every run of destructive updates.
 *
 * One staged upload (the stop list with each stop's list position, and per
 * value of every spread set what build_psets and cleared_counts read at the
 * call's start), one launch of k_destructive_full and one synchronisation
 * whatever `n`. Records and every later observable state equal those of the
 * per-call sequence pe_plan_stop(&allocs[i], 1), pe_select(tg, NULL), then
 * pe_commit, or pe_plan_pop_update(allocs[i]) and a break. Every Select is a
 * full pass: nodes_evaluated is the list length, nodes_filtered and
 * nodes_exhausted are those of the state that Select saw (its own stop
 * included), new_offset is the cursor unchanged, and pe_get_cursor afterwards
 * reads limit MaxInt32. The spread counts each Select sees are those
 * propertySet.GetCombinedUseMap gives with the stops so far cleared
 * (propertyset.go:159-209), kept on the device in closed form.
 *
 * PE_EINVAL, PE_ESTATE, n == 0 and PE_EINTERNAL as pe_place_destructive.
 * PE_EUNSUPPORTED, checked before anything changes (cursor, limit, memo, plan
 * and NodeUpdate untouched; the per-call sequence answers instead), each with
 * this entry's name in the message: every row of pe_place_destructive's list
 * except the full-pass one (n: more than 4096 updates); distinct_property at
 * job or group level; spread sets or affinity scores beyond the folded
 * per-node word (more than 2 sets, a set of more than 255 values, more than
 * 256 distinct affinity scores); a node list that names a row twice; more
 * options and listed stop positions than one workgroup's LDS holds (8192; the
 * kernel finds this while it builds its entries, before the first stop).
 * pe_place_destructive_stats covers this call too. */
int pe_place_destructive_full(pe_stack* s, uint32_t tg_index, const uint32_t* allocs, uint32_t n, pe_ranked_node* out,
                              uint32_t* placed);
/* pe_place_destructive_full with AllocMetric kept: the one entry of a caller
 * that keeps it (GenericScheduler always does, generic_sched.go:552-645) for
 * every run of destructive updates. Arguments and records are
 * pe_place_destructive_full's; the maps come back through
 * pe_place_destructive_maps (the same store, layout and lifetime as after
 * pe_place_destructive_metrics), one map set per returned record, the nil
 * Select's included, and that Select saw its own stop; the counters through
 * pe_place_destructive_stats.
 * With pe_set_metrics off the call is pe_place_destructive_full (no further
 * launch; the maps accessor answers PE_ESTATE). With it on and a group that
 * runs no full passes under an unlatched limit the call is
 * pe_place_destructive_metrics. With it on and a full-pass group, records,
 * maps and every later observable state equal those of the per-call sequence
 * with metrics on: pe_plan_stop(&allocs[i], 1), pe_select(tg, NULL), the maps
 * read, then pe_commit, or pe_plan_pop_update(allocs[i]) and a break. Later
 * state includes the metrics shadow of the memo. The records also equal
 * pe_place_destructive_full's on a handle with metrics off. pe_last_metrics*
 * answers PE_ESTATE after the call.
 * The dynamic node columns are copied on the device before the loop, the loop
 * kernel logs the spread use counts every Select saw, the host walks the list
 * until a walk changes no memo entry (later records reuse that walk), and one
 * batched trace builds the maps: the number of launches, uploads and
 * synchronisations does not depend on `n`.
 * PE_EINVAL, PE_ESTATE and n == 0 as pe_place_destructive_full. PE_EUNSUPPORTED,
 * checked before anything changes (the memo's metrics shadow included), with
 * this entry's name in the message: pe_place_destructive_full's list without
 * its pe_set_metrics row, and n * (node list length) above 2^24 (the caller
 * splits the run). PE_EINTERNAL: a bounds guard of the loop kernel tripped;
 * no maps are built and pe_place_destructive_maps answers PE_ESTATE. */
int pe_place_destructive_full_metrics(pe_stack* s, uint32_t tg_index, const uint32_t* allocs, uint32_t n,
                                      pe_ranked_node* out, uint32_t* placed);
/* The reason text CSIVolumeChecker.Feasible records (feasible.go:19-26) for
 * `reason` (PE_CSI_*): stateless, needs no device. `volume` is the request's
 * source after the per_alloc suffix (reasons 1, 5, 6, 7), `plugin` the volume's
 * plugin id and `node_id` Node.ID (reasons 2 to 4); NULL reads as "". Writes at
 * most cap bytes (NUL-terminated) and returns the bytes needed, or PE_EINVAL
 * for reason 0 or above 7. */
int64_t pe_csi_reason_text(uint32_t reason, const char* plugin, const char* volume, const char* node_id, char* buf,
                           size_t cap);
/* k_csi_avail launches of the handle so far (pe_select's and pe_place_csi's). */
uint64_t pe_csi_avail_launches(const pe_stack* s);
/* Measurement aid: device time in ms of the last pe_place_csi's k_csi_first
 * (ms2[0]) and k_csi_loop (ms2[1]), recorded only with PE_CSI_TIME=1;
 * PE_ESTATE otherwise. */
int pe_csi_place_ms(pe_stack* s, double* ms2);
/* LimitIterator + MaxScoreIterator (select.go:35-116) over a source with
 * transient nils, the fold pe_place_csi's kernel steps, exposed for tests;
 * needs no device. Item i of the stream is an option scoring scores[i]
 * (kind[i] == 0) or a nil after which the source goes on (kind[i] == 1); past
 * item n - 1 the source returns nil for ever. Outputs: the winner's item index
 * (-1 none), LimitIterator.seen, the items pulled, and whether the Select ended
 * at a nil Next rather than at seen == limit. */
int pe_csi_limit_fold(const double* scores, const uint8_t* kind, uint32_t n, uint32_t limit, int32_t* winner,
                      uint32_t* seen, uint32_t* consumed, uint32_t* ended_nil);
/* The same fold at limit MaxInt32 as pe_place_csi_full's kernel runs it: the
 * stream is compressed to its first 7 nils, its first 6 non-positive options
 * and the collapsed runs of options between them (csi_limit.h), and those are
 * stepped. Outputs as pe_csi_limit_fold(..., limit = 0x7FFFFFFF), which it
 * equals on every stream; PE_EINTERNAL if a bound of the compression does not
 * hold. Needs no device. */
int pe_csi_full_fold(const double* scores, const uint8_t* kind, uint32_t n, int32_t* winner, uint32_t* seen,
                     uint32_t* consumed, uint32_t* ended_nil);
/* The fp64 scoring math the kernels run (Go 1.16 math.Pow / Exp / Log restated,
 * ScoreFit, basicResourceDistance, preemptionScore, the score's ordered-integer
 * key), exposed for tests: item i of `op` evaluated by the function the kernels
 * call, on the host (device == 0; needs no device) or by a one-lane-per-item
 * kernel (device != 0; PE_EHIP without a device). out[i] holds the result's
 * IEEE-754 bits (PE_PROBE_ORDER_KEY: the key). Inputs:
 *   POW10_UNIT, POW10 (finite y, |y| < 2^63), EXP, LOG (x > 0), POW2, ORDER_KEY:
 *     xd[n];
 *   FIT_SCORE: xi[5 n] = (cap_cpu, cap_mem, util_cpu, util_mem, spread), the
 *     score over binPackingMaxFitScore as the ranking uses it;
 *   BASIC_DISTANCE: xi[6 n] = (ask cpu, mem, disk, alloc cpu, mem, disk);
 *   PREEMPTION_SCORE: xi = n + 1 offsets (xi[0] == 0, non-decreasing, at most
 *     256 apart), then the priorities of the preempted allocs they slice. */
#define PE_PROBE_POW10_UNIT 0u
#define PE_PROBE_POW10 1u
#define PE_PROBE_EXP 2u
#define PE_PROBE_LOG 3u
#define PE_PROBE_FIT_SCORE 4u
#define PE_PROBE_POW2 5u
#define PE_PROBE_BASIC_DISTANCE 6u
#define PE_PROBE_ORDER_KEY 7u
#define PE_PROBE_PREEMPTION_SCORE 8u
int pe_probe_math(uint32_t op, const double* xd, const int64_t* xi, uint32_t n, uint64_t* out, int device);
/* Go 1.16 sort.Slice as the Preemptor's kernels run it (less = key[x] < key[y]
 * over an index list), exposed for tests: array a is keys[off[a] .. off[a + 1])
 * (off[0] == 0), its identity permutation is sorted and written to perm_out at
 * the same offsets. idx_width picks the index type of the two the kernels
 * instantiate: 1 (uint8_t, arrays of at most 255) or 2 (uint16_t, at most
 * 65535). device == 0 sorts on the host and needs no device; otherwise one lane
 * per array (PE_EHIP without a device). */
int pe_probe_go_sort(const double* keys, const uint32_t* off, uint32_t n_arrays, uint32_t idx_width,
                     uint32_t* perm_out, int device);
/* Host-side constraint semantics used for pre-resolution (checkConstraint,
 * feasible.go:785-820), exposed for known-answer tests; needs no device.
 * l_state / r_state: 0 nil (unknown ${...} target), 1 found, 2 missing ("", false). */
int pe_check_constraint(const char* op, const char* l, int l_state, const char* r, int r_state);
/* The typed-attribute comparator of device constraints and affinities
 * (checkAttributeConstraint, feasible.go:1334-1447, over Attribute.Compare,
 * plugins/shared/structs/attribute.go:314-426), exposed for known-answer tests;
 * needs no device. The left side is a typed attribute as a device fingerprint
 * carries it: l_kind picks the value (PE_ATTR_INT: l_int, PE_ATTR_FLOAT:
 * l_float, PE_ATTR_STRING: l_str, PE_ATTR_BOOL: l_int != 0), l_unit is its unit
 * ("" or NULL: none), l_found whether the target resolved. The right side is
 * the constraint's literal text, parsed as RTarget is (ParseAttribute); r_found
 * == 0 or r_text == NULL stands for a target that did not resolve. */
#define PE_ATTR_NONE 0
#define PE_ATTR_INT 1
#define PE_ATTR_FLOAT 2
#define PE_ATTR_STRING 3
#define PE_ATTR_BOOL 4
int pe_check_attr(const char* op, int l_kind, int64_t l_int, double l_float, const char* l_str,
                  const char* l_unit, int l_found, const char* r_text, int r_found);

/* ======================================================================== *
 * Plan applier fit check (leader side).
 *
 * Replaces evaluatePlanPlacements' per-node worker calls
 * (nomad/plan_apply.go:439-582) to evaluateNodePlan (plan_apply.go:611-674) →
 * structs.AllocsFit(node, proposed, nil, checkDevices=true)
 * (nomad/structs/funcs.go:148-211), with NetworkIndex.SetNode/AddAllocs
 * (nomad/structs/network.go:92-193, 196-296) and DeviceAccounter
 * (nomad/structs/devices.go:22-101). The planner handle keeps the state
 * snapshot (nodes and their non-terminal allocations) resident in HBM; one
 * kernel evaluates every node of a plan (one wavefront per plan node) and
 * pe_planner_commit folds an applied plan back into the resident snapshot
 * (the optimistic snapshot.UpsertPlanResults of planApply, plan_apply.go:207).
 * Strings: every call carries its own pe_strtab; the planner interns by
 * content, so ids need not be stable across calls.
 * ======================================================================== */

/* evaluateNodePlan outcome per plan node; the reason strings are the
 * reference's (plan_apply.go:627-633, funcs.go:184-208, structs.go:3891-3905). */
#define PE_PLAN_FIT 0
#define PE_PLAN_NODE_MISSING 1      /* "node does not exist" */
#define PE_PLAN_NODE_NOT_READY 2    /* "node is not ready for placements" */
#define PE_PLAN_NODE_INELIGIBLE 3   /* "node is not eligible" */
#define PE_PLAN_CORES 4             /* "cores" (overlap between allocs, or not a subset of the node's) */
#define PE_PLAN_CPU 5               /* "cpu" */
#define PE_PLAN_MEMORY 6            /* "memory" */
#define PE_PLAN_DISK 7              /* "disk" */
#define PE_PLAN_PORTS 8             /* "reserved port collision" */
#define PE_PLAN_BANDWIDTH 9         /* "bandwidth exceeded": never (Overcommitted is disabled, network.go:79-90) */
#define PE_PLAN_DEVICES 10          /* "device oversubscribed" */

/* Nodes of the snapshot, the fields evaluateNodePlan / AllocsFit read. */
typedef struct pe_plan_node_table {
    uint32_t n;
    const uint8_t* ready;            /* Node.Status == "ready" */
    const uint8_t* eligible;         /* Node.SchedulingEligibility != "ineligible" */
    const int64_t* cpu_shares;       /* NodeResources.Cpu.CpuShares */
    const int64_t* memory_mb;
    const int64_t* disk_mb;
    const int64_t* reserved_cpu;     /* ReservedResources (0 when nil) */
    const int64_t* reserved_memory_mb;
    const int64_t* reserved_disk_mb;
    /* NodeResources.Cpu.ReservableCpuCores minus ReservedResources.Cpu.ReservedCpuCores */
    const uint32_t* core_off; const uint32_t* core_id;
    /* NodeResources.Networks entries with Device != "": their IP (str id) */
    const uint32_t* net_off; const uint32_t* net_ip;
    /* NodeResources.NodeNetworks[*].Addresses[*]: Address and ReservedPorts spec (str ids) */
    const uint32_t* addr_off; const uint32_t* addr_ip; const uint32_t* addr_reserved_ports;
    /* ReservedResources.Networks.ReservedHostPorts spec (str id; "" when unset) */
    const uint32_t* reserved_host_ports;
    /* NodeResources.Devices: groups (vendor, type, name) and their instances */
    const uint32_t* dev_off; const uint32_t* dev_vendor; const uint32_t* dev_type; const uint32_t* dev_name;
    const uint32_t* inst_off;        /* CSR over device groups */
    const uint32_t* inst_id; const uint8_t* inst_healthy;
} pe_plan_node_table;

/* Allocations: the snapshot's (node_row set) or a plan's (node_row ignored).
 * Resources are Allocation.ComparableResources() (structs.go:9656-9688). */
typedef struct pe_plan_alloc_table {
    uint32_t count;
    const uint32_t* node_row;
    const uint8_t* terminal;         /* Allocation.TerminalStatus() */
    const int64_t* cpu_shares;
    const int64_t* memory_mb;
    const int64_t* disk_mb;
    /* Flattened.Cpu.ReservedCores (a set per alloc) */
    const uint32_t* core_off; const uint32_t* core_id;
    /* the ports NetworkIndex.AddAllocs marks (network.go:144-193): the
       AllocatedResources.Shared.Ports (HostIP, Value) when non-empty, else the
       Reserved+Dynamic ports of Shared.Networks and of each task's first network (IP) */
    const uint32_t* port_off; const uint32_t* port_ip; const int64_t* port_value;
    /* one entry per AllocatedDeviceResource.DeviceIDs element of every task */
    const uint32_t* dev_off;
    const uint32_t* dev_vendor; const uint32_t* dev_type; const uint32_t* dev_name; const uint32_t* dev_instance;
} pe_plan_alloc_table;

/* One plan (structs.Plan) as evaluatePlanPlacements sees it, node by node. */
typedef struct pe_plan {
    uint32_t n_nodes;                /* nodeIDList: NodeUpdate keys then NodeAllocation keys */
    const uint32_t* node_row;        /* snapshot row, or PE_NONE when the node does not exist */
    /* snapshot allocs RemoveAllocs drops on that node: NodeUpdate ∪ NodePreemptions ∪
       NodeAllocation IDs (plan_apply.go:650-665), as indices into the snapshot alloc table */
    const uint32_t* remove_off; const uint32_t* remove_alloc;
    /* NodeAllocation[node]: CSR into `allocs` */
    const uint32_t* place_off;
    pe_plan_alloc_table allocs;
} pe_plan;

typedef struct pe_planner pe_planner;
pe_planner* pe_planner_create(int device);
void pe_planner_destroy(pe_planner* p);
const char* pe_planner_last_error(const pe_planner* p);
/* Upload the state snapshot: nodes and allocations (terminal ones are kept
 * as rows but never counted). Replaces any earlier snapshot. */
int pe_planner_set_state(pe_planner* p, const pe_strtab* strs, const pe_plan_node_table* nodes,
                         const pe_plan_alloc_table* allocs);
/* evaluateNodePlan for every plan node on the device: reason[i] = PE_PLAN_*.
 * *n_fit = nodes that fit. The AllAtOnce / partial-commit bookkeeping of
 * evaluatePlanPlacements stays with the caller (it needs only reason[]). */
int pe_planner_evaluate(pe_planner* p, const pe_strtab* strs, const pe_plan* plan, uint8_t* reason,
                        uint32_t* n_fit);
/* Apply the nodes whose reason is PE_PLAN_FIT to the resident snapshot:
 * removed allocs stop counting, placed allocs are appended (ApplyPlanResults).
 * `keep[i]` != 0 selects plan node i (the caller passes the result it applied). */
int pe_planner_commit(pe_planner* p, const pe_strtab* strs, const pe_plan* plan, const uint8_t* keep);
/* Device time of the last evaluate (HIP events around the kernel) and its
 * algorithmic bytes (records and keys read + reasons written), computed when
 * asked against the current snapshot: ask before pe_planner_commit. */
double pe_planner_kernel_ms(const pe_planner* p);
uint64_t pe_planner_last_bytes(const pe_planner* p);
uint32_t pe_planner_snapshot_allocs(const pe_planner* p);

#ifdef __cplusplus
}
#endif
#endif /* NOMAD_PE_H */
