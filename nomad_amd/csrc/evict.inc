// BinPack with eviction on the device (included by kernels.hip, namespace pe).
//
// A Select with Preempt=true (GenericScheduler.selectNextOption,
// generic_sched.go:773-792, after a nil Select) runs BinPackIterator with
// `evict` (rank.go:193-527): device asks that cannot be met go through
// Preemptor.PreemptForDevice, a failed AllocsFit through PreemptForTaskGroup
// (scheduler/preemption.go:194-601), and PreemptionScoringIterator appends the
// logistic net-priority score (rank.go:773-844). Every node's outcome depends
// only on the plan, so k_evict evaluates the whole visit list in parallel (one
// lane per node, the node's alloc list walked in registers) and
// k_evict_resolve reproduces LimitIterator + MaxScoreIterator over it.
//
// Order conventions (Go map order in the reference, SURVEY.md A5):
// ProposedAllocs = the node's non-terminal, non-preempted state allocs in
// table order followed by this eval's plan placements; device groups in node
// order. sort.Slice is Go 1.16's quickSort_func in full (go_sort below).
//
// Eviction width W (a launch parameter, PreemptArgs::mask_words): preempted
// sets are bit masks of W 32-bit words over the node's alloc indices, so a
// launch evaluates nodes with up to 32 W allocs and a ProposedAllocs list of
// up to 64 W entries (state allocs + plan placements). The host picks the
// narrowest width that covers the snapshot's largest node (W = 1 for <= 32
// allocs, the common case, with byte indices and one-word masks; W = 8 for
// <= 256); a node past the launch's width flags the launch (flags bit 1) and
// the host reruns it wider.

enum : int { kSkipped = 3 };
constexpr int kResolveBlock = 1024;

template <int W>
struct AMask {
    uint32_t w[W];
    __host__ __device__ __forceinline__ static AMask zero() {
        AMask m;
#pragma unroll
        for (int i = 0; i < W; i++) m.w[i] = 0u;
        return m;
    }
    __host__ __device__ __forceinline__ bool test(uint32_t i) const { return (w[i >> 5] >> (i & 31u)) & 1u; }
    __host__ __device__ __forceinline__ void set(uint32_t i) { w[i >> 5] |= 1u << (i & 31u); }
    __device__ __forceinline__ bool any() const {
        uint32_t x = 0;
#pragma unroll
        for (int i = 0; i < W; i++) x |= w[i];
        return x != 0u;
    }
    __device__ __forceinline__ AMask& operator|=(const AMask& o) {
#pragma unroll
        for (int i = 0; i < W; i++) w[i] |= o.w[i];
        return *this;
    }
    __device__ __forceinline__ void store(uint32_t* dst) const {
#pragma unroll
        for (int i = 0; i < W; i++) dst[i] = w[i];
    }
    __device__ __forceinline__ static AMask load(const uint32_t* src) {
        AMask m;
#pragma unroll
        for (int i = 0; i < W; i++) m.w[i] = src[i];
        return m;
    }
};

template <int W>
struct EvW {
    static constexpr uint32_t kAllocs = 32u * W;   // node allocs a launch evaluates
    static constexpr uint32_t kL = 64u * W;        // ProposedAllocs entries (state allocs + plan placements)
    using Idx = typename std::conditional<(W <= 4), uint8_t, uint16_t>::type;
    static constexpr Idx kPh = (Idx)~(Idx)0;       // a plan placement of the job in ProposedAllocs
    static_assert(kAllocs < (uint32_t)kPh, "alloc indices below the placeholder");
    using Mask = AMask<W>;
};

// math.Pow(x, 2) (Go 1.16 pow.go: yi = 2, yf = 0 -> Frexp mantissa squaring)
__host__ __device__ __forceinline__ double pow2_go(double x) {
    if (x == 1.0) return 1.0;
    if (x != x) return x;
    if (x == 0.0) return 0.0;
    if (__builtin_isinf(x)) return __builtin_inf();
    int xe;
    double x1 = gm::frexp_go(x, &xe);
    double a1 = 1.0;
    int ae = 0;
    for (int64_t i = 2; i != 0; i >>= 1) {
        if (xe < -(1 << 12) || (1 << 12) < xe) { ae += xe; break; }
        if (i & 1) { a1 *= x1; ae += xe; }
        x1 *= x1;
        xe <<= 1;
        if (x1 < 0.5) { x1 += x1; xe--; }
    }
    return gm::ldexp_go(a1, ae);
}

// basicResourceDistance (preemption.go:603-622)
__host__ __device__ __forceinline__ double basic_distance(int64_t ac, int64_t am, int64_t ad, const PreemptAlloc& u) {
    double mc = 0.0, cc = 0.0, dc = 0.0;
    if (am > 0) mc = ((double)am - (double)u.mem) / (double)am;
    if (ac > 0) cc = ((double)ac - (double)u.cpu) / (double)ac;
    if (ad > 0) dc = ((double)ad - (double)u.disk) / (double)ad;
    return __builtin_sqrt(pow2_go(mc) + pow2_go(cc) + pow2_go(dc));
}

// Go 1.16 sort.Slice: GoSortDev / go_sort in gosort.h (host and device).

// The Preemptor's sorts with the comparator's value precomputed per alloc
// index: key[x] < key[y]. A descending order stores negated keys (IEEE
// negation reverses every ordered comparison and leaves NaN unordered both
// ways, so the permutation is the reference's). One out-of-line sort per index
// type instead of one inlined copy per comparator: the distance comparators
// (three Pow calls each, at every call site of the sort) made
// PreemptForTaskGroup 67 KB of code, more than a CU pair's instruction cache,
// and a cold single-lane evaluation paid for the misses.
template <class Idx>
struct KeyLess {
    const double* key;
    __host__ __device__ __forceinline__ bool operator()(Idx x, Idx y) const { return key[x] < key[y]; }
};

template <class Idx>
__host__ __device__ __noinline__ void go_sort_keyed(Idx* v, int n, const double* key) {
    GoSortDev<Idx, KeyLess<Idx>> g{v, KeyLess<Idx>{key}};
    g.sort(n);
}

// Wave evaluations (k_ploop): all 64 lanes of a wave run one node's
// evaluation together, the scalar steps redundantly on identical values (the
// lists in LDS written with identical values by every lane), and split the
// per-alloc loops over the lanes. Every lane of the wave must be active.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The sequential `if (f(i) < best)` scan from best = DBL_MAX over i in [0, n):
// the first index of the smallest value below DBL_MAX, -1 for none. With
// kWave the lanes take i = lane, lane + 64, ... and a butterfly keeps the
// smaller value, the lower index on ties.
template <bool kWave, class F>
__device__ __forceinline__ int first_min(int n, F f) {
    const int lane = kWave ? (int)(threadIdx.x & 63u) : 0;
    double bd = 1.7976931348623157e308;
    int bi = 0x7FFFFFFF;
    for (int i = lane; i < n; i += kWave ? 64 : 1) {
        const double d = f(i);
        if (d < bd) { bd = d; bi = i; }
    }
    if (kWave)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double od = __shfl_xor(bd, off);
            const int oi = __shfl_xor(bi, off);
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
        }
    return bi == 0x7FFFFFFF ? -1 : bi;
}

__device__ __forceinline__ uint32_t byte_of(uint32_t w, int k) { return (w >> (8 * k)) & 255u; }

// AssignDevice of request q on packed free counts without consuming (device.go:32-131)
__device__ __forceinline__ int assign_one(const Ask& a, const DevClass& dc, int q, uint32_t free) {
    const uint32_t cnt = (uint32_t)a.dev_cnt[q];
    if (dc.n_groups == 0 || cnt == 0) return -1;
    int best = -1;
    double bs = 0.0;
    for (int g = 0; g < kMaxDevGroups; g++) {
        if (g >= (int)dc.n_groups) break;
        if (byte_of(free, g) < cnt || !((dc.match[q] >> g) & 1u)) continue;
        const double sc = dc.choice[q][g];
        if (best >= 0 && sc < bs) continue;
        best = g;
        bs = sc;
    }
    return best;
}

// Instances of group g held by an alloc.
__device__ __forceinline__ uint32_t held_in(const PreemptAlloc& x, int g) {
    uint32_t h = 0;
    for (int k = 0; k < 4; k++)
        if (k < (int)x.n_dev && (int)byte_of(x.dev_g, k) == g) h += byte_of(x.dev_c, k);
    return h;
}

// The index lists of one evaluation: ProposedAllocs and three scratch lists
// (the Preemptor's candidate / priority-group / chosen lists; its three
// passes run one after another). Per-lane evaluations (k_evict) keep it in
// private memory; k_ploop's single-lane evaluations get an LDS copy, so their
// many dependent list accesses are LDS reads instead of scratch round trips.
template <int W>
struct EvictCtx {
    using E = EvW<W>;
    using Idx = typename E::Idx;
    const PreemptArgs* A;
    const PreemptAlloc* na;   // the node's allocs (CSR slice)
    uint32_t m;               // node alloc count
    Idx* L;                   // ProposedAllocs: node alloc index or kPh
    Idx *t0, *t1, *t2;        // scratch lists (EvictWs)
    double* key;              // sort keys by node alloc index (EvictWs)
    int nL;
    bool unsupported;
};

template <int W>
struct EvictWs {
    using Idx = typename EvW<W>::Idx;
    Idx L[EvW<W>::kL];
    Idx t0[EvW<W>::kAllocs], t1[EvW<W>::kAllocs], t2[EvW<W>::kAllocs];
    double key[EvW<W>::kAllocs];
    // the evaluation's context beside its lists: in LDS for k_ploop's
    // single-lane evaluations (the out-of-line Preemptor passes read it
    // through memory; on the stack it cost the refreshes ~0.6 ms of C5's 34)
    EvictCtx<W> ctx;
};


template <int W>
__device__ __forceinline__ bool is_cand(const EvictCtx<W>& c, typename EvW<W>::Idx x) {
    return x != EvW<W>::kPh && c.na[x].job_key != c.A->job_key;   // SetCandidates (preemption.go:141-154)
}

// structs.RemoveAllocs (funcs.go:47-64): swap-with-last removal of `mask`
template <int W>
__device__ __forceinline__ void remove_allocs(EvictCtx<W>& c, const AMask<W>& mask) {
    int n = c.nL;
    for (int i = 0; i < n; i++) {
        const auto x = c.L[i];
        if (x != EvW<W>::kPh && mask.test(x)) {
            c.L[i] = c.L[n - 1];
            i--;
            n--;
        }
    }
    c.nL = n;
}

template <int W>
__device__ __forceinline__ bool preemptible(const EvictCtx<W>& c, uint32_t x) {
    return c.A->job_priority - c.na[x].priority >= 10;   // filterAndGroupPreemptibleAllocs
}

// Next priority group after `after` among the listed allocs: the smallest
// preemptible priority > after (INT32_MAX: none).
template <int W, class Idx>
__device__ __forceinline__ int32_t next_priority(const EvictCtx<W>& c, const Idx* v, int n, int32_t after) {
    int32_t p = 0x7FFFFFFF;
    for (int i = 0; i < n; i++) {
        const int32_t q = c.na[v[i]].priority;
        if (preemptible(c, v[i]) && q > after && q < p) p = q;
    }
    return p;
}

// PreemptForDevice + selectBestAllocs (preemption.go:472-601); returns the
// preempted allocs as a mask over node alloc indices (empty: no option).
template <int W>
__device__ __noinline__ AMask<W> preempt_for_device(EvictCtx<W>& c, const DevClass& dc, int q, uint32_t outer_free) {
    using Idx = typename EvW<W>::Idx;
    const uint32_t needed = (uint32_t)c.A->ask.dev_cnt[q];
    AMask<W> best_mask = AMask<W>::zero();
    int32_t best_prio = 0x7FFFFFFF;
    bool have = false;
    for (int g = 0; g < kMaxDevGroups && g < (int)dc.n_groups; g++) {
        if (!((dc.match[q] >> g) & 1u)) continue;
        // allocs using group g, once per matching device entry, in candidate order
        Idx* lst = c.t0;
        int nl = 0;
        for (int i = 0; i < c.nL; i++) {
            const Idx x = c.L[i];
            if (!is_cand(c, x)) continue;
            const PreemptAlloc& a = c.na[x];
            for (int k = 0; k < 4 && k < (int)a.n_dev; k++)
                if ((int)byte_of(a.dev_g, k) == g) {
                    // an alloc listed twice (two tasks on one group) would be
                    // counted twice by the reference's net priority
                    if (nl >= (int)EvW<W>::kAllocs || (nl > 0 && lst[nl - 1] == x)) {
                        c.unsupported = true;
                        return AMask<W>::zero();
                    }
                    lst[nl++] = x;
                }
        }
        if (nl == 0) continue;
        // priority groups ascending, accumulate until the free count suffices
        Idx* pre = c.t1;
        int np = 0;
        uint32_t cnt = 0;
        bool done = false;
        for (int32_t pr = next_priority(c, lst, nl, -0x7FFFFFFF - 1); pr != 0x7FFFFFFF && !done;
             pr = next_priority(c, lst, nl, pr)) {
            for (int i = 0; i < nl; i++) {
                if (c.na[lst[i]].priority != pr || !preemptible(c, lst[i])) continue;
                cnt += held_in(c.na[lst[i]], g);
                pre[np++] = lst[i];
                if (cnt + byte_of(outer_free, g) >= needed) { done = true; break; }
            }
        }
        if (!done) continue;
        // selectBestAllocs: sort by instances of g descending, keep until `needed`
        for (int i = 0; i < np; i++) c.key[pre[i]] = -(double)held_in(c.na[pre[i]], g);   // descending
        go_sort_keyed(pre, np, c.key);
        uint32_t got = 0;
        AMask<W> mask = AMask<W>::zero();
        int32_t net = 0;
        for (int i = 0; i < np; i++) {
            if (got >= needed) break;
            got += held_in(c.na[pre[i]], g);
            mask.set(pre[i]);
            const int32_t pr = c.na[pre[i]].priority;
            bool dup = false;   // net priority: each distinct priority once
            for (int k = 0; k < i && !dup; k++) dup = c.na[pre[k]].priority == pr;
            if (!dup) net += pr;
        }
        if (!have || net < best_prio) { best_prio = net; best_mask = mask; have = true; }
    }
    return best_mask;
}

// PreemptForTaskGroup + filterSuperset (preemption.go:194-264, 699-731).
// Ordered compaction: out[0..k) = get(i) for the i in [0, n) with pred(i), in
// order; returns k. kWave: the lanes test i = lane, lane + 64, ... and place
// their entries by ballot prefix counts.
template <bool kWave, class Idx, class P, class G>
__device__ __forceinline__ int compact(Idx* out, int n, P pred, G get) {
    int k = 0;
    if (kWave) {
        const uint32_t lane = threadIdx.x & 63u;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + (int)lane;
            const bool t = i < n && pred(i);
            const uint64_t bal = __ballot(t);
            if (t) out[k + __popcll(bal & ((1ull << lane) - 1ull))] = get(i);
            k += __popcll(bal);
        }
        wave_lds_sync();
    } else {
        for (int i = 0; i < n; i++)
            if (pred(i)) out[k++] = get(i);
    }
    return k;
}

// Sum of f(i) over i in [0, n) (exact integer arithmetic: any order).
template <bool kWave, class F>
__device__ __forceinline__ int64_t sum_i64(int n, F f) {
    int64_t x = 0;
    for (int i = kWave ? (int)(threadIdx.x & 63u) : 0; i < n; i += kWave ? 64 : 1) x += f(i);
    if (kWave)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// next_priority over the lanes: the smallest preemptible priority > after.
template <bool kWave, int W, class Idx>
__device__ __forceinline__ int32_t next_priority_w(const EvictCtx<W>& c, const Idx* v, int n, int32_t after) {
    if (!kWave) return next_priority(c, v, n, after);
    int32_t p = 0x7FFFFFFF;
    for (int i = (int)(threadIdx.x & 63u); i < n; i += 64) {
        const int32_t q = c.na[v[i]].priority;
        if (preemptible(c, v[i]) && q > after && q < p) p = q;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) p = min(p, __shfl_xor(p, off));
    return p;
}

template <int W, bool kWave = false>
__device__ AMask<W> preempt_for_tg(EvictCtx<W>& c, const NodeRec& r) {
    using Idx = typename EvW<W>::Idx;
    const Ask& a = c.A->ask;
    Idx* cand = c.t0;
    const int nc = compact<kWave>(cand, c.nL, [&](int i) { return is_cand(c, c.L[i]); }, [&](int i) { return c.L[i]; });
    const int64_t rem_c = r.cap_cpu - sum_i64<kWave>(nc, [&](int i) { return c.na[cand[i]].cpu; });
    const int64_t rem_m = r.cap_mem - sum_i64<kWave>(nc, [&](int i) { return c.na[cand[i]].mem; });
    const int64_t rem_d = r.cap_disk - sum_i64<kWave>(nc, [&](int i) { return c.na[cand[i]].disk; });
    int64_t need_c = a.cpu, need_m = a.mem, need_d = a.disk;
    int64_t av_c = rem_c, av_m = rem_m, av_d = rem_d;
    Idx* best = c.t1;
    int nb = 0;
    bool met = false;
    for (int32_t pr = next_priority_w<kWave>(c, cand, nc, -0x7FFFFFFF - 1); pr != 0x7FFFFFFF && !met;
         pr = next_priority_w<kWave>(c, cand, nc, pr)) {
        Idx* v = c.t2;
        int m = compact<kWave>(v, nc, [&](int i) { return c.na[cand[i]].priority == pr && preemptible(c, cand[i]); },
                               [&](int i) { return cand[i]; });
        while (m > 0 && !met) {
            int idx = first_min<kWave>(m, [&](int i) {
                const PreemptAlloc& x = c.na[v[i]];
                double pen = 0.0;
                const int32_t num = (int32_t)c.A->pcount[x.jtg_key];
                if (x.max_parallel > 0 && num >= x.max_parallel) pen = (double)((num + 1) - x.max_parallel) * 50.0;
                return basic_distance(need_c, need_m, need_d, x) + pen;
            });
            if (idx < 0) idx = 0;
            const PreemptAlloc& x = c.na[v[idx]];
            av_c += x.cpu; av_m += x.mem; av_d += x.disk;
            met = av_c >= a.cpu && av_m >= a.mem && av_d >= a.disk;
            best[nb++] = v[idx];
            v[idx] = v[m - 1];
            m--;
            need_c -= x.cpu; need_m -= x.mem; need_d -= x.disk;
            if (kWave) wave_lds_sync();
        }
    }
    if (!met) return AMask<W>::zero();
    for (int i = kWave ? (int)(threadIdx.x & 63u) : 0; i < nb; i += kWave ? 64 : 1)   // descending
        c.key[best[i]] = -basic_distance(a.cpu, a.mem, a.disk, c.na[best[i]]);
    if (kWave) wave_lds_sync();
    go_sort_keyed(best, nb, c.key);
    AMask<W> mask = AMask<W>::zero();
    int64_t f_c = rem_c, f_m = rem_m, f_d = rem_d;
    for (int i = 0; i < nb; i++) {
        const PreemptAlloc& x = c.na[best[i]];
        mask.set(best[i]);
        f_c += x.cpu; f_m += x.mem; f_d += x.disk;
        if (f_c >= a.cpu && f_m >= a.mem && f_d >= a.disk) break;
    }
    return mask;
}

// PreemptForNetwork (preemption.go:270-455) for an ask without static ports,
// on the node's single host network device: candidates with a network
// (Flattened.Networks non-empty) and a priority at least 10 below the job's;
// when the device's free bandwidth (total - used, possibly negative) is short,
// priority groups ascending, each sorted by distanceComparatorForNetwork
// (|needed - MBits| / needed plus the max_parallel penalty), are taken until
// it suffices; filterSuperset with the network resource factory then keeps
// the allocs, by distance descending, until MeetsRequirements (which is never
// true for an ask of 0 MBits, so all are kept). Returns the preempted mask,
// empty for nil (no candidate, nothing to preempt, or not enough).
// With static ports in the ask, the reserved-port step runs first
// (preemption.go:309-342) from the host-built per-node record: `plist` holds
// the port holders to preempt (CSR-relative indices, ask order), `pinfo` the
// kPort* flags; they leave the candidate list as RemoveAllocs does.
template <int W>
__device__ __noinline__ AMask<W> preempt_for_network(EvictCtx<W>& c, int32_t needed, int32_t total, int32_t used, bool* pdep,
                                        uint64_t plist = ~0ull, uint32_t pinfo = 0u) {
    using Idx = typename EvW<W>::Idx;
    Idx* lst = c.t0;
    int nl = 0;
    bool any = false;
    for (int i = 0; i < c.nL; i++) {
        const Idx x = c.L[i];
        if (!is_cand(c, x)) continue;
        any = true;
        if (!(c.na[x].state_index & kAllocHasNet) || !preemptible(c, x)) continue;
        lst[nl++] = x;
    }
    if (!any || nl == 0 || total < needed) return AMask<W>::zero();
    if (pinfo & kPortFail) return AMask<W>::zero();   // a needed port is held by an alloc too close in priority
    const int32_t free_bw = total - used;
    const double dn = (double)needed;
    auto dist = [&](Idx x) { return __builtin_fabs((double)((int64_t)needed - c.na[x].mbits) / dn); };
    auto score = [&](Idx x) {   // scoreForNetwork (preemption.go:653-660)
        const PreemptAlloc& u = c.na[x];
        double pen = 0.0;
        const int32_t num = (int32_t)c.A->pcount[u.jtg_key];
        if (u.max_parallel > 0 && num >= u.max_parallel) pen = (double)((num + 1) - u.max_parallel) * 50.0;
        return dist(x) + pen;
    };
    Idx* pre = c.t1;
    int np = 0;
    int32_t pbw = 0;
    if (pinfo & kPortCount) {
        AMask<W> rm = AMask<W>::zero();
        for (int k = 0; k < (int)(pinfo & kPortCount); k++) {
            const Idx x = (Idx)byte_of((uint32_t)(plist >> (32 * (k >> 2))), k & 3);
            pre[np++] = x;
            pbw += c.na[x].mbits;
            rm.set(x);
        }
        for (int i = 0; i < nl; i++)   // currentAllocs = RemoveAllocs(currentAllocs, allocsToPreempt)
            if (rm.test(lst[i])) { lst[i] = lst[nl - 1]; i--; nl--; }
    }
    bool met = pbw + free_bw >= needed;
    for (int32_t pr = next_priority(c, lst, nl, -0x7FFFFFFF - 1); !met && pr != 0x7FFFFFFF;
         pr = next_priority(c, lst, nl, pr)) {
        Idx* v = c.t2;
        int m = 0;
        for (int i = 0; i < nl; i++)
            if (c.na[lst[i]].priority == pr) v[m++] = lst[i];
        for (int i = 0; i < m && pdep && !*pdep; i++) *pdep = c.na[v[i]].max_parallel > 0;
        for (int i = 0; i < m; i++) c.key[v[i]] = score(v[i]);
        go_sort_keyed(v, m, c.key);
        for (int i = 0; i < m; i++) {
            pbw += c.na[v[i]].mbits;
            pre[np++] = v[i];
            if (pbw + free_bw >= needed) { met = true; break; }
        }
    }
    if (!met || np == 0) return AMask<W>::zero();
    for (int i = 0; i < np; i++) c.key[pre[i]] = -dist(pre[i]);   // descending
    go_sort_keyed(pre, np, c.key);
    int32_t avail = free_bw;
    AMask<W> mask = AMask<W>::zero();
    for (int i = 0; i < np; i++) {
        mask.set(pre[i]);
        avail += c.na[pre[i]].mbits;
        if (avail != 0 && needed != 0 && avail >= needed) break;
    }
    return mask;
}

// netPriority / preemptionScore (rank.go:808-844) over the preempted allocs
template <int W>
__host__ __device__ __forceinline__ double preemption_score(const EvictCtx<W>& c, const AMask<W>& mask) {
    int32_t sum = 0;
    double mx = 0.0;
    for (uint32_t i = 0; i < c.m; i++)
        if (mask.test(i)) {
            const double p = (double)c.na[i].priority;
            if (p > mx) mx = p;
            sum += c.na[i].priority;
        }
    const double net = mx + ((double)sum / mx);
    return 1.0 / (1.0 + gm::exp_go(0.0048 * (net - 2048.0)));
}

// BinPack with evict for one node + the rest of the ranking chain. Returns the
// status; out->score (and parts with kKeepParts), the preempted mask and the
// device offers (one byte per request).
// With `named` (AllocMetric, k_evict_trace): the ScoreNode values by scorer,
// [binpack, devices, job-anti-affinity, node-affinity, allocation-spread,
// preemption, normalized], `flags` bit 0 the rescheduling penalty, bit 1 a
// preemption; `dim_out` the AllocsFit dimension of an exhausted node.
// *unsupported gets kEvictUnsup (outside the modelled surface) or kEvictWider
// (the node's allocs or ProposedAllocs exceed width W: rerun wider).
// `ws`: the evaluation's index lists (private memory or LDS).
template <bool kKeepParts, bool kCores = false, int W = 1, bool kWave = false>
__device__ int evict_eval(const PreemptArgs& A, uint32_t row, NodeEval* out, AMask<W>* mask_out,
                          uint32_t* offers_out, uint32_t* unsupported, EvictWs<W>* ws, double* named = nullptr,
                          uint32_t* flags = nullptr, uint32_t* dim_out = nullptr, bool* pdep = nullptr,
                          const PreemptAlloc* na_stage = nullptr) {
    using Mask = AMask<W>;
    using Idx = typename EvW<W>::Idx;
    const NodeSoA& s = A.soa;
    const TgTables& t = A.tg;
    const Ask& a = A.ask;
    NodeIn in;
    load_node(s, t, row, in);
    const NodeRec& r = in.r;
    const uint32_t cls = r.cls;
    bool ok = t.node_feas ? in.feas != 0 : (t.class_ok[cls] != 0 && (!t.node_ok || t.node_ok[row] != 0));
    if (ok && (a.distinct_job | a.distinct_tg)) {
        if (a.distinct_job && s.coll_job[row] > 0) ok = false;
        if (a.distinct_tg && in.coll_tg > 0) ok = false;
    }
    if (ok && t.n_psets > t.n_spread) ok = distinct_ok(t, A.spread_tab, row, cls);
    if (!ok) return kFiltered;
    // BinPack network offers (rank.go:248-379). Static ports (group or task
    // network): the host-built gate says whether they are free now; after
    // PreemptForNetwork they are free when the host's record says the listed
    // holders were all that blocked them and no placement of the group since
    bool g_ok = true, t_ok = true, post_base = true;
    uint64_t plist = ~0ull;
    uint32_t pinfo = 0;
    uint64_t pblock = ~0ull;
    if (t.static_gate || t.task_gate) {
        const uint32_t gv = t.static_gate ? t.static_gate[row] : t.task_gate[row];
        const bool now = gv != 0u && in.coll_tg + 1u == gv;
        pinfo = t.port_info ? t.port_info[row] : (uint32_t)kPortUnsup;
        plist = t.port_list ? t.port_list[row] : ~0ull;
        pblock = t.port_block ? t.port_block[row] : ~0ull;
        // after PreemptForNetwork the ports are free when nothing permanent
        // blocks them, every blocking alloc was preempted, and no placement of
        // the group took them since the gate was built (the host's blocker
        // list names up to 8 allocs; a node with more marks kPortUnsup)
        post_base = !(pinfo & kPortBlocked) && (gv == 0u || in.coll_tg + 1u == gv);
        if (t.static_gate) g_ok = now;
        else t_ok = now;
    }
    auto ports_free_after = [&](const Mask& preempted) {
        if (!post_base) return false;
        for (int k = 0; k < 8; k++) {   // every listed blocker preempted
            const uint32_t x = (uint32_t)(pblock >> (8 * k)) & 0xFFu;
            if (x == 0xFFu) break;
            if (!preempted.test(x)) return false;
        }
        return true;
    };
    EvictCtx<W>& c = ws->ctx;
    c.A = &A;
    c.L = ws->L;
    c.t0 = ws->t0;
    c.t1 = ws->t1;
    c.t2 = ws->t2;
    c.key = ws->key;
    const uint32_t b = A.node_alloc_off[row];
    c.m = A.node_alloc_off[row + 1] - b;
    c.na = na_stage ? na_stage : A.allocs + b;   // an LDS copy of the node's list (k_ploop), or HBM
    c.unsupported = false;
    if (!kCores && a.cores > 0) { *unsupported |= kEvictUnsup; return kFiltered; }   // compiled without reserved cores
    const uint32_t placeholders = s.coll_job[row] - A.own_existing[row];
    const bool ctx_ok = c.m <= EvW<W>::kAllocs && c.m + placeholders <= EvW<W>::kL;
    c.nL = 0;
    if (ctx_ok) {
        if (kWave) {   // the preempted flags read by the lanes at once, compacted in order by ballot
            const uint32_t lane = threadIdx.x & 63u;
            int nl = 0;
            for (uint32_t i0 = 0; i0 < c.m; i0 += 64u) {
                const uint32_t i = i0 + lane;
                const bool keep = i < c.m && !A.preempted[b + i];
                const uint64_t bal = __ballot(keep);
                if (keep) c.L[nl + __popcll(bal & ((1ull << lane) - 1ull))] = (Idx)i;
                nl += __popcll(bal);
            }
            wave_lds_sync();
            c.nL = nl;
        } else {
            for (uint32_t i = 0; i < c.m; i++)
                if (!A.preempted[b + i]) c.L[c.nL++] = (Idx)i;
        }
        for (uint32_t i = 0; i < placeholders; i++) c.L[c.nL++] = EvW<W>::kPh;
    }
    Mask pre = Mask::zero(), net_pre = Mask::zero();
    // a multi-device node (TgTables::md): the task network's outcome is the host's
    const MdNet* md = (a.has_task_net && t.md && t.md[row].lim != ~0u) ? &t.md[row] : nullptr;
    if (a.tg_dyn > 0 || a.has_task_net || t.static_gate) {
        // the NetworkIndex over the proposed allocs (SetNode + AddAllocs)
        int32_t bw = r.used_mbits, dyn = r.used_dyn;
        const int32_t total = r.avail_mbits > 0 ? r.avail_mbits : 0;   // AvailBandwidth of the device
        auto drop = [&](const Mask& np) {   // proposed = RemoveAllocs(proposed, np); index rebuilt
            pre |= np;
            net_pre |= np;
            remove_allocs(c, np);
            for (uint32_t i = 0; i < c.m; i++)
                if (np.test(i)) { bw -= c.na[i].mbits; dyn -= c.na[i].dyn; }
        };
        int32_t idx_dyn = dyn;
        bool md_group = false;   // a multi-device node whose group offer failed: the host's verdict covers it
        if (a.tg_dyn > 0 || t.static_gate) {
            const bool alias = !(t.alias_ok && !t.alias_ok[row]);
            auto dyn_ok = [&]() { return a.tg_dyn == 0 || (alias && kDynPortCapacity - dyn - a.static_dyn >= 1); };
            if (md && (!g_ok || !dyn_ok())) {
                // candidates grouped per device: the host ran the group's
                // PreemptForNetwork and retry before the task network's (MdNet::gpre)
                md_group = true;
            } else if (!g_ok || !dyn_ok()) {
                // AssignPorts failed (rank.go:265-300): PreemptForNetwork on the
                // group's ask (no MBits; its static ports' holders first)
                if (!ctx_ok) { *unsupported |= kEvictWider; return kFiltered; }
                if (t.static_gate && (pinfo & kPortUnsup)) { *unsupported |= kEvictUnsup; return kFiltered; }
                const Mask np = t.static_gate ? preempt_for_network(c, 0, total, bw, pdep, plist, pinfo)
                                              : preempt_for_network(c, 0, total, bw, pdep);
                if (c.unsupported) { *unsupported |= kEvictUnsup; return kFiltered; }
                if (!np.any()) return kSkipped;
                drop(np);
                if ((t.static_gate && !ports_free_after(pre)) || !dyn_ok()) return kSkipped;
            }
            idx_dyn = dyn + a.tg_dyn + a.static_dyn;   // AddReservedPorts(offer)
        }
        if (md) {
            // the host built the verdict for this state (the Preempt Select
            // rebuilds the tables): the offer fits, or PreemptForNetwork's
            // listed allocs leave and the retried offer fits, or the node is
            // skipped (nil from PreemptForNetwork or from the retry)
            const MdNet m = *md;
            if (m.ev == kMdUnsup || in.coll_tg != m.coll || (m.gpre != 0) != md_group) {
                *unsupported |= kEvictUnsup;
                return kFiltered;
            }
            if (m.ev == kMdSkip) return kSkipped;
            if (m.ev == kMdPre) {
                if (!ctx_ok) { *unsupported |= kEvictWider; return kFiltered; }
                Mask np = Mask::zero();
                for (uint32_t k = 0; k < m.n_pre && k < 8; k++) {
                    const uint32_t x = (uint32_t)(m.pre >> (8 * k)) & 0xFFu;
                    if (x >= c.m) { *unsupported |= kEvictUnsup; return kFiltered; }
                    np.set(x);
                }
                drop(np);
            }
        } else if (a.has_task_net && (r.avail_mbits < 0 || bw + a.task_mbits > r.avail_mbits || !t_ok ||
                               kDynPortCapacity - idx_dyn < a.task_dyn)) {
            // AssignNetwork failed (rank.go:343-379): PreemptForNetwork on the
            // task's ask; one task network only (each task's ask is its own).
            // The host's port record assumes the snapshot's candidates: not
            // after the group's own network preemption
            if (!ctx_ok) { *unsupported |= kEvictWider; return kFiltered; }
            if (a.has_task_net > 1 || (t.task_gate && ((pinfo & kPortUnsup) || net_pre.any()))) {
                *unsupported |= kEvictUnsup;
                return kFiltered;
            }
            const Mask np = t.task_gate ? preempt_for_network(c, a.task_mbits, total, bw, pdep, plist, pinfo)
                                        : preempt_for_network(c, a.task_mbits, total, bw, pdep);
            if (c.unsupported) { *unsupported |= kEvictUnsup; return kFiltered; }
            if (!np.any()) return kSkipped;
            drop(np);
            // the rebuilt index holds the remaining proposed allocs only: the
            // group's port offer is not added back (rank.go:362-371)
            if (r.avail_mbits < 0 || bw + a.task_mbits > r.avail_mbits || (t.task_gate && !ports_free_after(pre)) ||
                kDynPortCapacity - dyn < a.task_dyn)
                return kSkipped;
        }
    }
    if (!ctx_ok) { *unsupported |= kEvictWider; return kFiltered; }
    Mask dev_pre = Mask::zero();
    uint32_t offers = 0;
    double dev_match = 0.0;
    if (a.n_dev > 0) {   // rank.go:366-414
        const DevClass& dc = t.dev_cls[cls];
        const uint32_t fr0 = in.dev_free;
        uint32_t fr = fr0;
        for (int q = 0; q < kMaxDevReq && q < a.n_dev; q++) {
            int g = assign_one(a, dc, q, fr);
            if (g < 0) {
                const Mask d = preempt_for_device(c, dc, q, fr);
                if (c.unsupported) { *unsupported |= kEvictUnsup; return kFiltered; }
                if (!d.any()) return kSkipped;
                pre |= d;
                dev_pre |= d;
                remove_allocs(c, pre);
                // a fresh allocator over the remaining proposed allocs (rank.go:400-402)
                uint32_t inner = fr0;
                for (uint32_t i = 0; i < c.m; i++)
                    if (pre.test(i))
                        for (int k = 0; k < 4 && k < (int)c.na[i].n_dev; k++)
                            inner += byte_of(c.na[i].dev_c, k) << (8 * byte_of(c.na[i].dev_g, k));
                g = assign_one(a, dc, q, inner);
                if (g < 0) return kSkipped;
            }
            const uint32_t cnt = (uint32_t)a.dev_cnt[q];
            const uint32_t f = byte_of(fr, g);
            fr -= (cnt < f ? cnt : f) << (8 * g);   // AddReserved on the outer allocator
            if ((a.dev_aff >> q) & 1u) dev_match += dc.matched[q][g];
            offers |= (uint32_t)g << (8 * q);
        }
    }
    // reserved cores (rank.go:437-466): evaluated here only where no eviction
    // is involved (a plain fit, or the reference's "TODO preemption" exhaustion)
    int64_t acpu = a.cpu;
    bool core_out = false;
    if (kCores && a.cores > 0) {
        if (dev_pre.any()) { *unsupported |= kEvictUnsup; return kFiltered; }
        const CoreFit f = core_fit(s.core_rsvable, s.core_used, s.core_avail, s.core_spc, (uint32_t)a.cores, row, 0);
        if (f.status == 1) {
            if (dim_out) *dim_out = kTrCores;
            return kExhausted;
        }
        acpu += f.cpu;
        core_out = f.status == 2;
    }
    // AllocsFit over the remaining proposed allocs plus the ask
    int64_t ucpu = r.used_cpu + acpu, umem = r.used_mem + a.mem, udisk = r.used_disk + a.disk;
    for (uint32_t i = 0; i < c.m; i++)   // network and device preemptions already left `proposed`
        if (dev_pre.test(i) || net_pre.test(i)) { ucpu -= c.na[i].cpu; umem -= c.na[i].mem; udisk -= c.na[i].disk; }
    if (r.cap_cpu < ucpu || core_out || r.cap_mem < umem || r.cap_disk < udisk) {
        if (a.cores > 0) { *unsupported |= kEvictUnsup; return kFiltered; }   // eviction with reserved cores: host path
        if (pdep)   // the max_parallel penalty reads the plan's preemption counts (preemption.go:220-240)
            for (uint32_t i = 0; i < c.m && !*pdep; i++) *pdep = c.na[i].max_parallel > 0;
        const Mask tp = preempt_for_tg<W, kWave>(c, r);
        if (c.unsupported) { *unsupported |= kEvictUnsup; return kFiltered; }
        if (!tp.any()) {
            if (dim_out) *dim_out = r.cap_cpu < ucpu ? kTrCpu : (r.cap_mem < umem ? kTrMemory : kTrDisk);
            return kExhausted;
        }
        pre |= tp;
    }
    ScoreIn si;
    si.ccpu = r.cap_cpu;
    si.cmem = r.cap_mem;
    si.ucpu = ucpu;
    si.umem = umem;
    si.coll = in.coll_tg;
    si.dev_aff = a.dev_tw != 0.0 ? dev_match / a.dev_tw : 0.0;
    lookup_scores(t, A.penalty_bits, A.spread_tab, row, cls, &si);
    NodeEval ev;
    score_option<true>(a, A.log10, si, &ev);
    double ps = 0.0;
    const bool any_pre = pre.any();
    if (any_pre && A.score_preemption) {   // PreemptionScoringIterator: appended last, then the average again
        ps = preemption_score(c, pre);
        double sum = 0.0;
        for (uint32_t k = 0; k < ev.nscores; k++) sum += ev.parts[k];
        sum += ps;
        ev.parts[ev.nscores] = ps;
        ev.nscores++;
        ev.score = sum / (double)ev.nscores;
    }
    if (named) {   // the parts in append order, by scorer (as k_trace)
        uint32_t k = 1;
        named[0] = ev.parts[0];
        named[1] = a.dev_tw != 0.0 ? ev.parts[k++] : 0.0;
        named[2] = (a.anti_aff && si.coll > 0) ? ev.parts[k++] : 0.0;
        if (si.penalty) k++;
        named[3] = si.aff != 0.0 ? ev.parts[k++] : 0.0;
        named[4] = si.spread != 0.0 ? ev.parts[k++] : 0.0;
        named[5] = ps;
        named[6] = ev.score;
        *flags = (si.penalty ? 1u : 0u) | ((any_pre && A.score_preemption) ? 2u : 0u);
    }
    out->status = kOption;
    out->score = ev.score;
    out->nscores = ev.nscores;
    if (kKeepParts)
        for (int k = 0; k < PE_MAX_SCORES; k++) out->parts[k] = k < (int)ev.nscores ? ev.parts[k] : 0.0;
    *mask_out = pre;
    *offers_out = offers;
    return kOption;
}

// The Preempt outcome of one visit position into the per-position arrays
// (with kParts also the score parts of an option).
// mask_out holds W words per position.
template <bool kParts, int W, bool kWave = false>
__device__ __forceinline__ int evict_store(const PreemptArgs& A, uint32_t j, uint32_t* unsup, bool* dep,
                                           EvictWs<W>* ws, const PreemptAlloc* na_stage = nullptr) {
    NodeEval ev;
    AMask<W> mask = AMask<W>::zero();
    uint32_t offers = 0;
    const int st = evict_eval<kParts, false, W, kWave>(A, A.visit[j], &ev, &mask, &offers, unsup, ws, nullptr, nullptr,
                                                nullptr, dep, na_stage);
    A.score[j] = st == kOption ? ev.score : 0.0;
    if (A.mask_out) mask.store(A.mask_out + (size_t)j * W);
    if (A.offers_out) A.offers_out[j] = offers;
    if (kParts && st == kOption) {
        A.nparts_out[j] = (uint8_t)ev.nscores;
        for (int k = 0; k < PE_MAX_SCORES; k++) A.parts_out[(size_t)j * PE_MAX_SCORES + k] = ev.parts[k];
    }
    return st;
}

template <bool kParts, int W>
__global__ void __launch_bounds__(256) k_evict(PreemptArgs A) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < A.n_visit; j += stride) {
        uint32_t unsup = 0;
        bool dep = false;
        EvictWs<W> ws;
        const int st = evict_store<kParts, W>(A, j, &unsup, A.dep_out ? &dep : nullptr, &ws);
        if (unsup) atomicOr(A.flags, unsup);
        if (A.dep_out) A.dep_out[j] = dep ? 1 : 0;
        A.status[j] = (uint8_t)st;
    }
}

// AllocMetric of a Select with Preempt (compute_metrics): per row the BinPack
// with evict outcome, code = status | dim << 8 | flags << 16, and the ScoreNode
// values of an option (7 per row, evict_eval's `named`). Bits 24-25: the
// kEvictUnsup / kEvictWider flags of the row.
template <int W>
__global__ void __launch_bounds__(64) k_evict_trace(PreemptArgs A, const uint32_t* rows, uint32_t n, uint32_t* code,
                                                    double* named) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    NodeEval ev;
    AMask<W> m = AMask<W>::zero();
    uint32_t offers = 0, flags = 0, dim = 0, unsup = 0;
    EvictWs<W> ws;
    const int st = evict_eval<true, false, W>(A, rows[i], &ev, &m, &offers, &unsup, &ws, named + (size_t)i * 7,
                                              &flags, &dim);
    code[i] = (uint32_t)st | (dim << 8) | (flags << 16) | (unsup << 24);
}

// The chosen node's full record (scores in append order, preempted allocs as
// W mask words, offers); mask[W] gets the kEvict* flags.
template <int W>
__global__ void __launch_bounds__(64) k_evict_record(PreemptArgs A, uint32_t row, pe_ranked_node* out, uint32_t* mask) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    NodeEval ev;
    AMask<W> m = AMask<W>::zero();
    uint32_t offers = 0, unsup = 0;
    EvictWs<W> ws;
    const int st = evict_eval<true, true, W>(A, row, &ev, &m, &offers, &unsup, &ws);
    out->final_score = st == kOption ? ev.score : 0.0;
    out->n_scores = st == kOption ? ev.nscores : 0u;
    for (int k = 0; k < PE_MAX_SCORES; k++) out->scores[k] = (st == kOption && k < (int)ev.nscores) ? ev.parts[k] : 0.0;
    out->n_device_offers = (st == kOption && A.ask.n_dev > 0) ? (uint32_t)A.ask.n_dev : 0u;
    for (int q = 0; q < PE_MAX_DEVICE_REQ; q++) out->device_offer_group[q] = byte_of(offers, q);
    m.store(mask);
    mask[W] = unsup;
}

// LimitIterator + MaxScoreIterator over the per-position results (one workgroup).
// Chunks without an option (a saturated cluster) only count filtered /
// exhausted positions per lane; the prefix walk runs on chunks with options.
__global__ void __launch_bounds__(kResolveBlock) k_evict_resolve(EvictResolveArgs R) {
    constexpr int BLOCK = kResolveBlock;
    __shared__ LoopShared<BLOCK> sh;
    const int tid = threadIdx.x;
    const uint32_t n = R.n;
    uint32_t r = 0, a = 0, n_filtered = 0, n_exhausted = 0, consumed = n;
    uint32_t lane_f = 0, lane_e = 0;   // counts of the option-free chunks
    double best_score = -__builtin_inf();
    int best_pos = -1;
    bool stopped = false;
    // Super-chunks of kSuper chunks: their status / score loads are issued
    // together, one chunk-set ahead (software pipelining), and a super-chunk
    // without any option is only counted (one block vote instead of kSuper).
    constexpr int kSuper = 4;
    auto load = [&](uint32_t sbase, int* st, double* sc) {
        for (int q = 0; q < kSuper; q++) {
            const uint32_t j = sbase + (uint32_t)q * BLOCK + tid;
            st[q] = kFiltered;
            sc[q] = 0.0;
            if (j < n) {
                uint32_t pos = R.offset + j;
                if (pos >= n) pos -= n;
                st[q] = R.status[pos];
                sc[q] = R.score[pos];
            }
        }
    };
    int st_next[kSuper];
    double sc_next[kSuper];
    load(0, st_next, sc_next);
    for (uint32_t sbase = 0; sbase < n && !stopped; sbase += kSuper * BLOCK) {
        int st_cur[kSuper];
        double sc_cur[kSuper];
        bool any = false;
        for (int q = 0; q < kSuper; q++) {
            st_cur[q] = st_next[q];
            sc_cur[q] = sc_next[q];
            any = any || (sbase + (uint32_t)q * BLOCK + tid < n && st_cur[q] == kOption);
        }
        if (sbase + kSuper * BLOCK < n) load(sbase + kSuper * BLOCK, st_next, sc_next);
        if (!__syncthreads_or(any)) {
            for (int q = 0; q < kSuper; q++) {
                const bool valid = sbase + (uint32_t)q * BLOCK + tid < n;
                lane_f += (valid && st_cur[q] == kFiltered) ? 1u : 0u;
                lane_e += (valid && st_cur[q] == kExhausted) ? 1u : 0u;
            }
            continue;
        }
      for (int q = 0; q < kSuper; q++) {
        const uint32_t base = sbase + (uint32_t)q * BLOCK;
        if (base >= n) break;
        const uint32_t j = base + tid;
        const bool valid = j < n;
        const int st = st_cur[q];
        const double sc = sc_cur[q];
        const bool is_opt = valid && st == kOption;
        if (!__syncthreads_or(is_opt)) {
            lane_f += (valid && st == kFiltered) ? 1u : 0u;
            lane_e += (valid && st == kExhausted) ? 1u : 0u;
            continue;
        }
        const bool is_np = is_opt && sc <= 0.0;
        uint32_t np_tot;
        const uint32_t np_before = a + block_prefix<BLOCK>(is_np, sh.wave_a, &np_tot);
        const bool aside = is_np && np_before < (uint32_t)kMaxSkip;
        const bool ret = is_opt && !aside;
        uint32_t ret_tot;
        const uint32_t ret_before = r + block_prefix<BLOCK>(ret, sh.wave_b, &ret_tot);
        const bool is_stop = ret && ret_before == R.limit - 1u;
        if (tid == 0) sh.stop_j = -1;
        __syncthreads();
        if (is_stop) sh.stop_j = tid;
        __syncthreads();
        const int stop_j = sh.stop_j;
        const bool pulled = valid && (stop_j < 0 || tid <= stop_j);
        if (aside && pulled) {
            sh.aside_score[np_before] = sc;
            sh.aside_pos[np_before] = (int)j;
        }
        const bool cand = ret && ret_before < R.limit;
        double cs;
        int cp;
        block_argmax<BLOCK>(cand, sc, (int)j, sh.red_score, sh.red_pos, &cs, &cp);
        if (cp != 0x7FFFFFFF && cs > best_score) { best_score = cs; best_pos = cp; }
        uint32_t f_tot, e_tot, a_tot;
        block_prefix<BLOCK>(pulled && st == kFiltered, sh.wave_a, &f_tot);
        block_prefix<BLOCK>(pulled && st == kExhausted, sh.wave_b, &e_tot);
        block_prefix<BLOCK>(aside && pulled, sh.wave_a, &a_tot);
        n_filtered += f_tot;
        n_exhausted += e_tot;
        a += a_tot;
        if (stop_j >= 0) {
            consumed = base + (uint32_t)stop_j + 1u;
            r = R.limit;
            stopped = true;
            break;
        }
        r += ret_tot;
      }
    }
    __syncthreads();
    if (!stopped) {
        const uint32_t take = min(a, R.limit - r);
        for (uint32_t i = 0; i < take; i++)
            if (sh.aside_score[i] > best_score) { best_score = sh.aside_score[i]; best_pos = sh.aside_pos[i]; }
    }
    uint32_t f_tot, e_tot;
    for (int off = 32; off > 0; off >>= 1) {
        lane_f += __shfl_xor(lane_f, off);
        lane_e += __shfl_xor(lane_e, off);
    }
    if ((tid & 63) == 0) { sh.wave_a[tid >> 6] = lane_f; sh.wave_b[tid >> 6] = lane_e; }
    __syncthreads();
    f_tot = e_tot = 0;
    for (int w = 0; w < BLOCK / 64; w++) { f_tot += sh.wave_a[w]; e_tot += sh.wave_b[w]; }
    n_filtered += f_tot;
    n_exhausted += e_tot;
    if (tid == 0) {
        R.out[0] = best_pos;
        R.out[1] = (int32_t)consumed;
        R.out[2] = (int32_t)n_filtered;
        R.out[3] = (int32_t)n_exhausted;
    }
}

// Plan.AppendPreemptedAlloc of the masked allocs of `row` (generic_sched.go:794-816):
// their resources leave the node's proposed state and the (job, tg) counters grow.
template <int W>
__device__ void apply_preempt(const PreemptArgs& A, uint32_t row, const AMask<W>& mask, uint8_t* preempted,
                              uint32_t* pcount, uint32_t* dev_free) {
    const uint32_t b = A.node_alloc_off[row];
    const uint32_t m = A.node_alloc_off[row + 1] - b;
    NodeRec& r = A.soa.rec[row];
    uint32_t fr = dev_free ? dev_free[row] : 0u;
    for (uint32_t i = 0; i < m; i++) {
        if (i >= 32u * W || !mask.test(i) || preempted[b + i]) continue;
        const PreemptAlloc& x = A.allocs[b + i];
        r.used_cpu -= x.cpu;
        r.used_mem -= x.mem;
        r.used_disk -= x.disk;
        r.used_mbits -= x.mbits;
        r.used_dyn -= x.dyn;
        for (int k = 0; k < 4 && k < (int)x.n_dev; k++) fr += byte_of(x.dev_c, k) << (8 * byte_of(x.dev_g, k));
        if (A.palloc_cores && A.soa.core_used)   // its reserved cores are free again
            for (int w = 0; w < 4; w++) A.soa.core_used[4 * row + w] &= ~A.palloc_cores[4 * (size_t)(b + i) + w];
        preempted[b + i] = 1;
        atomicAdd(&pcount[x.jtg_key], 1u);
    }
    if (dev_free) dev_free[row] = fr;
}

// Plan.AppendStoppedAlloc (sign +1) / PopUpdate (sign -1) of snapshot allocs
// (slots of the per-node CSR): the alloc leaves (returns to) the proposed
// state of its node, EvalContext.ProposedAllocs (context.go:120-157). The flag
// value 2 marks a stop (1 is a plan preemption); neither is a Preemptor
// candidate. Several allocs may share a node: integer atomics.
__global__ void __launch_bounds__(64) k_plan_stop(NodeRec* rec, uint32_t* dev_free, const PreemptAlloc* allocs,
                                                  uint8_t* preempted, const uint32_t* slots, const uint32_t* rows,
                                                  uint32_t n, int sign, uint64_t* core_used,
                                                  const uint64_t* palloc_cores) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = slots[i], row = rows[i];
    const PreemptAlloc& x = allocs[slot];
    if (core_used && palloc_cores)   // reserved cores leave (return to) the node's used set
        for (int w = 0; w < 4; w++) {
            const unsigned long long m = palloc_cores[4 * (size_t)slot + w];
            if (!m) continue;
            if (sign > 0) atomicAnd(reinterpret_cast<unsigned long long*>(&core_used[4 * row + w]), ~m);
            else atomicOr(reinterpret_cast<unsigned long long*>(&core_used[4 * row + w]), m);
        }
    NodeRec& r = rec[row];
    const unsigned long long s64 = (unsigned long long)(long long)(-sign);
    const unsigned int s32 = (unsigned int)(-sign);
    atomicAdd(reinterpret_cast<unsigned long long*>(&r.used_cpu), (unsigned long long)x.cpu * s64);
    atomicAdd(reinterpret_cast<unsigned long long*>(&r.used_mem), (unsigned long long)x.mem * s64);
    atomicAdd(reinterpret_cast<unsigned long long*>(&r.used_disk), (unsigned long long)x.disk * s64);
    atomicAdd(reinterpret_cast<unsigned int*>(&r.used_mbits), (unsigned int)x.mbits * s32);
    atomicAdd(reinterpret_cast<unsigned int*>(&r.used_dyn), (unsigned int)x.dyn * s32);
    if (dev_free) {
        uint32_t d = 0;
        for (int k = 0; k < 4 && k < (int)x.n_dev; k++) d += byte_of(x.dev_c, k) << (8 * byte_of(x.dev_g, k));
        if (sign > 0) atomicAdd(&dev_free[row], d);
        else atomicSub(&dev_free[row], d);
    }
    preempted[slot] = sign > 0 ? 2 : 0;
}

// `mask`: W words in device memory
template <int W>
__global__ void k_commit_preempt(PreemptArgs A, uint32_t row, const uint32_t* mask, uint8_t* preempted,
                                 uint32_t* pcount, uint32_t* dev_free) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    apply_preempt(A, row, AMask<W>::load(mask), preempted, pcount, dev_free);
}

// One evicting placement on `row`: Plan.AppendPreemptedAlloc of the masked
// allocs, then Plan.AppendAlloc of the ask with its device offers (*offers:
// one byte per request, read only for a device ask).
template <int W>
__device__ __forceinline__ void commit_evicted_row(const PreemptArgs& A, uint32_t row, const AMask<W>& mask,
                                                   const uint32_t* offers, uint8_t* preempted, uint32_t* pcount,
                                                   uint32_t* dev_free) {
    apply_preempt(A, row, mask, preempted, pcount, dev_free);
    NodeRec& r = A.soa.rec[row];
    r.used_cpu += ask_cpu(A.soa, A.ask, row);
    core_take(A.soa, A.ask, row, 1);
    r.used_mem += A.ask.mem;
    r.used_disk += A.ask.disk;
    r.used_mbits += A.ask.commit_mbits;
    r.used_dyn += A.ask.commit_dyn;
    A.soa.coll_job[row] += 1;
    A.tg.coll_tg[row] += 1;
    if (A.ask.n_dev > 0) {
        uint32_t fr = A.tg.dev_free[row];
        for (int q = 0; q < kMaxDevReq && q < A.ask.n_dev; q++) {
            const uint32_t g = byte_of(*offers, q), f = byte_of(fr, (int)g);
            const uint32_t cnt = (uint32_t)A.ask.dev_cnt[q];
            fr -= (cnt < f ? cnt : f) << (8 * g);
        }
        A.tg.dev_free[row] = fr;
    }
}

// SystemScheduler placements that evict (scheduler_system.go:283-425): every
// listed node is distinct, so the preemptions and Plan.AppendAlloc of all
// chosen nodes apply in parallel (one lane per node).
template <int W>
__global__ void __launch_bounds__(256) k_commit_evicted(PreemptArgs A, uint8_t* preempted, uint32_t* pcount,
                                                        uint32_t* dev_free, uint32_t* placed) {
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t local = 0;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < A.n_visit; j += stride) {
        if (A.status[j] != kOption) continue;
        commit_evicted_row(A, A.visit[j], AMask<W>::load(A.mask_out + (size_t)j * W), A.offers_out + j, preempted,
                           pcount, dev_free);
        local++;
    }
    for (int off = 32; off > 0; off >>= 1) local += __shfl_xor(local, off);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(placed, local);
}

// ---- device-resident count loop over sparse options (k_ploop) --------------
//
// GenericScheduler.computePlacements on a saturated cluster (generic_sched.go:
// 552-627, 773-792): every placement is a plain Select whose options are rare,
// retried with Preempt=true when it comes back nil. Both Selects read the
// per-position outcomes of the whole visit list; a commit changes the outcome
// of the committed row only (its proposed allocs, collisions and device free
// counts; no spread or distinct_property sets, no max_parallel penalty on the
// path), so the loop keeps the outcomes of both passes as 2-bit codes in LDS
// (kOption / kFiltered / kExhausted / kSkipped, 16 positions per word), its
// scores by position in HBM, and re-evaluates only committed rows: the plain
// outcome right after the commit, the evict outcome lazily before the next
// Preempt Select. LimitIterator + MaxScoreIterator (select.go:5-116) resolve
// over the codes with the same prefix rules as k_evict_resolve, 16 consecutive
// positions per lane, chunks without an option counted with popcounts.

// Threads of the k_ploop workgroup. The single-lane evaluations keep stack
// objects and spills in scratch, and their first touches cost far more than
// the work itself (a plain winner's evaluation takes ~13-20 us cold, ~5 us when
// re-run at once; inlining them, which spills more, made it ~490 us; having
// the wave pre-load the node's tables first only added its own round trip). 512 (8 waves, 256 VGPRs per lane)
// spilled half as much as 1024: C5 k_ploop 56.8 -> 41.5 ms per 1000
// placements. 256 (one wave per SIMD) lets the compiler spill into the 256
// AGPRs instead of scratch: 43.0 -> 34.8 ms on one A/B box (the plain resolve
// gets slower with half the lanes, the evaluations and the Preempt resolve
// faster). A/B builds set it.
#ifndef PE_PLOOP_BLOCK
#define PE_PLOOP_BLOCK 256
#endif
constexpr int kPLoopBlock = PE_PLOOP_BLOCK;
constexpr int kPLoopPer = 16;
constexpr uint32_t kPLoopDirtyCap = 2048;
constexpr uint32_t kCodeEven = 0x55555555u;
constexpr int kPLoopStage = 4;   // LDS alloc-list slots: waves refreshing one dirty row each / the winner
// Plain-outcome summary: options, filtered and exhausted positions per
// aligned block of kPLoopSpan positions (one resolve step), so a plain
// resolve steps over the blocks without an option (the plain options of a
// busy cluster are sparse and its windows long)
constexpr uint32_t kPLoopSpan = 2048;
constexpr uint32_t kPLoopMaxBlk = (229376u + kPLoopSpan - 1u) / kPLoopSpan;
struct PLoopSummary {
    uint32_t opt[kPLoopMaxBlk], fil[kPLoopMaxBlk], exh[kPLoopMaxBlk];
};

// A placement's pe_ranked_node fields, staged in LDS by thread 0 and written
// to L.out by wave 1: on gfx9 one counter (vmcnt) tracks a wave's loads and
// stores in issue order, so stores left on wave 0 would hold up its next
// loads (the committed row's re-evaluation, the next resolve's scores).
struct PLoopRec {
    double score, parts[PE_MAX_SCORES];
    uint32_t row, nscores, evaluated, filtered, exhausted, new_offset, n_dev, offers;
    uint32_t mask[8];
};

struct PLoopShared {
    uint32_t wave_f[kPLoopBlock / 64];   // ploop_count_codes' per-wave sums
    uint32_t wave_e[kPLoopBlock / 64];
    double aside_score[kMaxSkip];
    int aside_pos[kMaxSkip];
    int32_t res[4];
    uint32_t n_dirty, dirty_all, pcount_changed, flags;
    uint32_t n_live;                  // dirty entries not yet refreshed (refreshed ones hold PE_NONE)
    uint32_t n_hit;                   // dirty positions inside a lazy resolve's window
    uint32_t hit[kPLoopStage];
    uint32_t last_plain;   // the committed row's plain outcome on the new state
    PLoopRec rec;          // the placement's record, written out by wave 1
    PLoopSummary sum_plain;
    uint32_t dirty[kPLoopDirtyCap];
    PreemptAlloc stage[kPLoopStage][kMaxNodeAllocs];
};

__device__ __forceinline__ uint32_t ploop_pos(uint32_t n, uint32_t offset, uint32_t j) {
    const uint32_t p = offset + j;
    return p >= n ? p - n : p;
}

// Codes of relative positions j0 .. j0+15 (2 bits each, position j0+i at bit
// 2i); positions past the list read as kSkipped (counted nowhere).
// LDS-qualified pointers: the callees get pointers into LDS as generic ones,
// whose loads would be flat (a vector-memory round trip each); these keep them
// ds_read.
#define PE_LDS __attribute__((address_space(3)))

__device__ __forceinline__ uint32_t ploop_codes16(const PE_LDS uint32_t* codes, uint32_t n, uint32_t offset,
                                                  uint32_t j0) {
    if (j0 >= n) return 0xFFFFFFFFu;
    const uint32_t p0 = ploop_pos(n, offset, j0);
    if (j0 + kPLoopPer <= n && p0 + kPLoopPer <= n) {
        const uint32_t w = p0 >> 4, sh = p0 & 15u;
        const uint64_t lo = codes[w];
        const uint64_t hi = sh ? (uint64_t)codes[w + 1] : 0ull;
        return (uint32_t)(((hi << 32) | lo) >> (2u * sh));
    }
    uint32_t x = 0;
    for (uint32_t i = 0; i < (uint32_t)kPLoopPer; i++) {
        const uint32_t j = j0 + i;
        uint32_t c = 3u;
        if (j < n) {
            const uint32_t p = ploop_pos(n, offset, j);
            c = (codes[p >> 4] >> (2u * (p & 15u))) & 3u;
        }
        x |= c << (2u * i);
    }
    return x;
}

__device__ __forceinline__ void ploop_set_code(uint32_t* codes, uint32_t pos, uint32_t c) {
    const uint32_t sh = 2u * (pos & 15u);
    atomicAnd(&codes[pos >> 4], ~(3u << sh));
    atomicOr(&codes[pos >> 4], (c & 3u) << sh);
}

// Wave-wide exclusive prefix sum of v < 64; *total = the wave's sum. Bit
// slices through ballots: no LDS round trip (v counts a lane's 32 positions).
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t* total) {
    const uint64_t lt = (1ull << (threadIdx.x & 63u)) - 1ull;
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int b = 0; b < 6; b++) {
        const uint64_t m = __ballot((v >> b) & 1u);
        before += (uint32_t)__popcll(m & lt) << b;
        tot += (uint32_t)__popcll(m) << b;
    }
    *total = tot;
    return before;
}

// Wave-wide sum of v < 2^13 through bit-slice ballots (scalar popcounts).
__device__ __forceinline__ uint32_t wave_sum13(uint32_t v) {
    uint32_t tot = 0;
#pragma unroll
    for (int b = 0; b < 13; b++) tot += (uint32_t)__popcll(__ballot((v >> b) & 1u)) << b;
    return tot;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// LimitIterator + MaxScoreIterator over the coded outcomes from `offset`.
// One wave resolves (32 positions a lane, 2048 a step: the window is
// usually one step, and wave scans and reductions need no workgroup
// barrier); every lane of the block calls it and finds sh.res after the
// closing barrier: [0] winner (relative position) or -1, [1] consumed,
// [2] filtered, [3] exhausted.
// With `summary` the steps are aligned blocks (the first and last partial)
// and a whole block without an option adds its counts without a step.
__device__ void ploop_resolve(PLoopShared& sh, const uint32_t* codes, const double* score, uint32_t n,
                              uint32_t offset, uint32_t limit, unsigned long long* tp = nullptr,
                              const PLoopSummary* summary = nullptr) {
    if (threadIdx.x < 64) {
        const PE_LDS uint32_t* lc = (const PE_LDS uint32_t*)codes;
        PE_LDS PLoopShared* ls = (PE_LDS PLoopShared*)&sh;
        const PE_LDS PLoopSummary* su = (const PE_LDS PLoopSummary*)summary;
        uint32_t steps = 0;
        constexpr uint32_t kPer = 2u * kPLoopPer;
        constexpr uint64_t kEven = 0x5555555555555555ull;
        const uint32_t lane = threadIdx.x & 63u;
        uint32_t r = 0, a = 0, lane_f = 0, lane_e = 0, consumed = n, blk_f = 0, blk_e = 0;
        double best = -__builtin_inf();
        int best_pos = -1;
        bool stopped = false;
        uint32_t step;
        for (uint32_t base = 0; base < n; base += step) {
            step = min(kPLoopSpan, n - base);
            if (summary) {
                const uint32_t ab = ploop_pos(n, offset, base), blk = ab / kPLoopSpan;
                step = min(min(kPLoopSpan * (blk + 1u), n) - ab, n - base);
                if (ab == kPLoopSpan * blk && step == min(kPLoopSpan, n - ab) && su->opt[blk] == 0u) {
                    blk_f += su->fil[blk];   // wave-uniform
                    blk_e += su->exh[blk];
                    continue;
                }
            }
            const uint32_t j0 = base + lane * kPer;
            uint64_t x = (uint64_t)ploop_codes16(lc, n, offset, j0) |
                         ((uint64_t)ploop_codes16(lc, n, offset, j0 + kPLoopPer) << 32);
            if (step < kPLoopSpan) {   // positions past the step read as kSkipped
                const uint32_t v = j0 >= base + step ? 0u : min(base + step - j0, kPer);
                if (v < kPer) x |= ~((1ull << (2u * v)) - 1ull);
            }
            const uint64_t opt = ~(x | (x >> 1)) & kEven;
            const uint64_t fil = x & ~(x >> 1) & kEven;
            const uint64_t exh = (x >> 1) & ~x & kEven;
            const bool none = __ballot(opt != 0ull) == 0ull;
            steps++;
            if (none) {
                lane_f += (uint32_t)__popcll(fil);
                lane_e += (uint32_t)__popcll(exh);
                continue;
            }
            // non-positive options (the LimitIterator's skip candidates), and
            // the lane's best positive option on the way (one score load each,
            // four of a lane's loads in flight at a time: A/B on C5 against all
            // 32 at once 25.2 -> 23.3 ms, against one at a time 24.2 ms)
            uint64_t np = 0;
            double pb = -__builtin_inf();
            int pp = 0x7FFFFFFF;
            // only the options the stop can be among get a score: limit - r
            // returned ones and the skips still left to set aside (a dense
            // Preempt window loads ~limit scores, not the step's 2048)
            uint64_t ldm = opt;
            {
                const uint32_t oc = (uint32_t)__popcll(opt);
                uint32_t o_tot;
                const uint32_t o_before = wave_excl_scan(oc, &o_tot);
                const uint32_t quota0 = a < (uint32_t)kMaxSkip ? (uint32_t)kMaxSkip - a : 0u;
                const uint64_t need = (uint64_t)(limit - r) + quota0;
                if ((uint64_t)o_before >= need) {
                    ldm = 0;
                } else if ((uint64_t)o_before + oc > need) {
                    uint64_t m = opt;
                    for (uint32_t c = (uint32_t)(need - o_before); c > 0u; c--) m &= m - 1ull;
                    ldm = opt & ~m;
                }
            }
            for (uint64_t m = ldm; m;) {   // KB options at a time: their loads in one round
                constexpr int KB = 4;
                uint32_t ix[KB];
#pragma unroll
                for (int t = 0; t < KB; t++) {
                    ix[t] = m ? (uint32_t)__builtin_ctzll(m) >> 1 : 0xFFu;
                    m &= m - 1ull;
                }
                double v[KB];
#pragma unroll
                for (int t = 0; t < KB; t++) v[t] = ix[t] != 0xFFu ? score[ploop_pos(n, offset, j0 + ix[t])] : 0.0;
#pragma unroll
                for (int t = 0; t < KB; t++) {
                    if (ix[t] == 0xFFu) break;
                    const double sc = v[t];
                    if (sc <= 0.0) np |= 1ull << (2u * ix[t]);
                    else if (pp == 0x7FFFFFFF || sc > pb) { pb = sc; pp = (int)(j0 + ix[t]); }
                }
            }
            const bool any_np = __ballot(np != 0ull) != 0ull;
            uint32_t np_before = a;
            uint64_t aside = 0;
            if (any_np) {
                uint32_t np_tot;
                np_before = a + wave_excl_scan((uint32_t)__popcll(np), &np_tot);
                uint32_t k = np_before;
                for (uint64_t m = np; m && k < (uint32_t)kMaxSkip; m &= m - 1ull, k++) aside |= m & (~m + 1ull);
            }
            const uint64_t ret = opt & ~aside;
            const uint32_t ret_cnt = (uint32_t)__popcll(ret);
            uint32_t ret_tot;
            const uint32_t ret_before = r + wave_excl_scan(ret_cnt, &ret_tot);
            // the lane holding the limit-th returned option (at most one)
            const bool holds = ret_before < limit && (uint64_t)ret_before + ret_cnt >= (uint64_t)limit;
            const uint64_t hb = __ballot(holds);
            int stop_j = -1;
            if (hb) {
                const int sl = (int)__builtin_ctzll(hb);
                int mine = 0;
                if (holds) {
                    uint64_t m = ret;
                    for (uint32_t k = limit - ret_before; k > 1u; k--) m &= m - 1ull;
                    mine = (int)(j0 + ((uint32_t)__builtin_ctzll(m) >> 1));
                }
                stop_j = __builtin_amdgcn_readlane(mine, sl);
            }
            uint64_t pulled = ~0ull;
            if (stop_j >= 0) {
                const int64_t lim = (int64_t)stop_j - (int64_t)j0 + 1;   // positions of this lane up to the stop
                pulled = lim <= 0 ? 0ull : (lim >= (int64_t)kPer ? ~0ull : ((1ull << (2u * (uint32_t)lim)) - 1ull));
            }
            // MaxScoreIterator over the returned options pulled (earliest on
            // ties): the lane's best positive option, unless the stop cuts the
            // lane or a non-positive option is returned (then from the scores)
            double lb = -__builtin_inf();
            int lp = 0x7FFFFFFF;
            if (pulled == ~0ull && (np & ~aside) == 0ull) {
                lb = pb;
                lp = pp;
            } else if (pulled != 0ull) {
                for (uint64_t m = ret & pulled; m; m &= m - 1ull) {
                    const uint32_t i = (uint32_t)__builtin_ctzll(m) >> 1;
                    const double sc = score[ploop_pos(n, offset, j0 + i)];
                    if (lp == 0x7FFFFFFF || sc > lb) { lb = sc; lp = (int)(j0 + i); }
                }
            }
            uint64_t cm = __ballot(lp != 0x7FFFFFFF);
            if (__popcll(cm) <= 8) {
                // few candidate lanes: read them in lane (= position) order
                double bs = -__builtin_inf();
                int bp = 0x7FFFFFFF;
                for (; cm; cm &= cm - 1ull) {
                    const int l = (int)__builtin_ctzll(cm);
                    const long long bits = __double_as_longlong(lb);
                    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bits, l);
                    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(bits >> 32), l);
                    const double os = __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
                    const int op = __builtin_amdgcn_readlane(lp, l);
                    if (bp == 0x7FFFFFFF || os > bs) { bs = os; bp = op; }
                }
                lb = bs;
                lp = bp;
            } else {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const double os = __shfl_xor(lb, off);
                    const int op = __shfl_xor(lp, off);
                    if (os > lb || (os == lb && op < lp)) { lb = os; lp = op; }
                }
            }
            if (lp != 0x7FFFFFFF && lb > best) { best = lb; best_pos = lp; }
            if (any_np) {
                uint32_t k = np_before;
                for (uint64_t m = aside & pulled; m; m &= m - 1ull, k++) {
                    const uint32_t i = (uint32_t)__builtin_ctzll(m) >> 1;
                    ls->aside_score[k] = score[ploop_pos(n, offset, j0 + i)];
                    ls->aside_pos[k] = (int)(j0 + i);
                }
                a += wave_sum((uint32_t)__popcll(aside & pulled));
            }
            lane_f += (uint32_t)__popcll(fil & pulled);
            lane_e += (uint32_t)__popcll(exh & pulled);
            if (stop_j >= 0) {
                consumed = (uint32_t)stop_j + 1u;
                r = limit;
                stopped = true;
                break;
            }
            r += ret_tot;
        }
        wave_lds_sync();   // the aside entries
        if (!stopped) {
            const uint32_t take = min(a, limit - r);
            for (uint32_t i = 0; i < take; i++)
                if (ls->aside_score[i] > best) { best = ls->aside_score[i]; best_pos = ls->aside_pos[i]; }
        }
        // a lane's own counts stay below n / 64 + 64 < 2^13
        const uint32_t f_tot = wave_sum13(lane_f) + blk_f, e_tot = wave_sum13(lane_e) + blk_e;
        if (lane == 0) {
            ls->res[0] = best_pos;
            ls->res[1] = (int32_t)consumed;
            ls->res[2] = (int32_t)f_tot;
            ls->res[3] = (int32_t)e_tot;
            if (tp) {   // profile: steps and calls
                tp[0] += steps;
                tp[1] += 1;
            }
        }
    }
    __syncthreads();
}

// Filtered and exhausted positions over the whole plain code list (a plain
// Select the loop skipped as provably failing consumed all of it).
__device__ void ploop_count_codes(PLoopShared& sh, const uint32_t* codes, uint32_t n, uint32_t* fil_tot,
                                  uint32_t* exh_tot) {
    uint32_t f = 0, e = 0;
    for (uint32_t w = (uint32_t)threadIdx.x; w < ((n + 15u) >> 4); w += kPLoopBlock) {
        const uint32_t x = codes[w];   // positions past n hold kSkipped (3): counted nowhere
        f += (uint32_t)__popc(x & ~(x >> 1) & kCodeEven);
        e += (uint32_t)__popc((x >> 1) & ~x & kCodeEven);
    }
    f = wave_sum(f);
    e = wave_sum(e);
    if ((threadIdx.x & 63u) == 0u) {
        sh.wave_f[threadIdx.x >> 6] = f;
        sh.wave_e[threadIdx.x >> 6] = e;
    }
    __syncthreads();
    uint32_t ft = 0, et = 0;
#pragma unroll
    for (int w = 0; w < kPLoopBlock / 64; w++) {
        ft += sh.wave_f[w];
        et += sh.wave_e[w];
    }
    __syncthreads();
    *fil_tot = ft;
    *exh_tot = et;
}

template <int W>
__device__ __forceinline__ void ploop_nil(const PLoopArgs& L, uint32_t p, const int32_t* res, uint32_t new_offset) {
    pe_ranked_node& o = L.out[p];
    o.row = -1;
    o.n_scores = 0;
    o.final_score = 0.0;
    for (int k = 0; k < PE_MAX_SCORES; k++) o.scores[k] = 0.0;
    o.nodes_evaluated = (uint32_t)res[1];
    o.nodes_filtered = (uint32_t)res[2];
    o.nodes_exhausted = (uint32_t)res[3];
    o.new_offset = new_offset;
    o.n_preempted = 0;
    o.n_device_offers = 0;
    for (int q = 0; q < PE_MAX_DEVICE_REQ; q++) o.device_offer_group[q] = 0;
    AMask<W>::zero().store(L.out_mask + (size_t)p * W);
}

// The heavy per-row evaluations of the loop stay out of line: the resolve's
// registers are not spilled around them (inlined, C5 took 20x as long).
// The winner's evaluation is a wave evaluation (every lane of wave 0).
template <bool kKeepParts, int W>
__device__ __noinline__ int ploop_evict_eval(const PreemptArgs& A, uint32_t row, NodeEval* out, AMask<W>* mask,
                                             uint32_t* offers, uint32_t* unsup, bool* dep, EvictWs<W>* ws,
                                             const PreemptAlloc* na_stage = nullptr) {
    return evict_eval<kKeepParts, false, W, true>(A, row, out, mask, offers, unsup, ws, nullptr, nullptr, nullptr,
                                                  dep, na_stage);
}

// The loop's single-row evaluations walk the node's alloc list many times
// (candidate filters, priority groups, distance sorts): one wave copies the
// list (<= 32 x 64 B) into an LDS slot with coalesced 16-byte loads first, so
// the evaluating lane's dependent reads hit LDS instead of L2. Null when the
// node has more allocs than the device path evicts over (evict_eval then
// reads HBM and flags the node itself). Every lane of the wave calls it.
__device__ __forceinline__ const PreemptAlloc* ploop_stage(const PreemptArgs& A, uint32_t row, PreemptAlloc* slot) {
    const uint32_t b = A.node_alloc_off[row], m = A.node_alloc_off[row + 1] - b;
    if (m > (uint32_t)kMaxNodeAllocs) return nullptr;
    const uint4* src = reinterpret_cast<const uint4*>(A.allocs + b);
    uint4* dst = reinterpret_cast<uint4*>(slot);
    constexpr uint32_t kWords = sizeof(PreemptAlloc) / sizeof(uint4);
    for (uint32_t i = threadIdx.x & 63u; i < m * kWords; i += 64u) dst[i] = src[i];
    return slot;
}

// Preempt outcome of one position on the current state: score, code, and
// whether it read the plan's preemption counts.
template <bool kParts, int W, bool kWave>
__device__ __noinline__ int ploop_evict_store(const PreemptArgs& A, uint32_t pos, uint32_t* unsup, bool* dep,
                                              EvictWs<W>* ws, const PreemptAlloc* na_stage) {
    return evict_store<kParts, W, kWave>(A, pos, unsup, dep, ws, na_stage);
}

// k_ploop's refresh flags: 1 a node outside the modelled surface, 4 a node
// wider than the launch (2 is the winner check's)
__device__ __forceinline__ uint32_t ploop_flag_of(uint32_t unsup) {
    return ((unsup & kEvictUnsup) ? 1u : 0u) | ((unsup & kEvictWider) ? 4u : 0u);
}

// kWave: a wave evaluation (every lane of the wave, lane 0 publishes).
template <int W, bool kWave = false>
__device__ __forceinline__ void ploop_refresh(const PLoopArgs& L, uint32_t* ce, uint32_t* dep, uint32_t pos,
                                              uint32_t* flags, EvictWs<W>* ws, const PreemptAlloc* na_stage = nullptr,
                                              const PreemptArgs* EP = nullptr) {
    uint32_t unsup = 0;
    bool d = false;
    int st;
    if (kWave) {
        // the winner's evaluation function itself: one copy of the evaluation
        // code in the instruction cache (a cold evaluation costs ~13 us against
        // ~4.5 us with its code cached, whatever its data)
        NodeEval ev;
        AMask<W> mask = AMask<W>::zero();
        uint32_t offers = 0;
        st = ploop_evict_eval<true, W>(EP ? *EP : L.P, L.P.visit[pos], &ev, &mask, &offers, &unsup, &d, ws, na_stage);
        if ((threadIdx.x & 63u) != 0u) return;
        const PreemptArgs& A = L.P;   // evict_store's stores
        A.score[pos] = st == kOption ? ev.score : 0.0;
        if (A.mask_out) mask.store(A.mask_out + (size_t)pos * W);
        if (A.offers_out) A.offers_out[pos] = offers;
        if (A.parts_out && st == kOption) {
            A.nparts_out[pos] = (uint8_t)ev.nscores;
            for (int k = 0; k < PE_MAX_SCORES; k++) A.parts_out[(size_t)pos * PE_MAX_SCORES + k] = ev.parts[k];
        }
    } else {
        st = L.P.parts_out ? ploop_evict_store<true, W, false>(L.P, pos, &unsup, &d, ws, na_stage)
                           : ploop_evict_store<false, W, false>(L.P, pos, &unsup, &d, ws, na_stage);
    }
    if (unsup) atomicOr(flags, ploop_flag_of(unsup));
    ploop_set_code(ce, pos, (uint32_t)st);
    if (d) atomicOr(&dep[pos >> 5], 1u << (pos & 31u));
    else atomicAnd(&dep[pos >> 5], ~(1u << (pos & 31u)));
}

__device__ __forceinline__ void ploop_plain_eval(const PreemptArgs& A, uint32_t row, NodeEval* out) {
    Overlay none;
    none.keys = nullptr;
    eval_node<true, false>(A.soa, A.tg, A.tg.class_ok, A.ask, none, A.penalty_bits, A.log10, nullptr, row, out);
}

// A plain winner's record: its plain outcome's score parts (k_census, or the
// re-evaluation after its row's last commit: a placement changes no other
// row's plain outcome), the device offers on the current state (AllocsFit
// holds, so no request needs a preemption: rank.go:366-414 without its
// fallback) and evict_eval's width check (the node's allocs and
// ProposedAllocs fit the launch's width). The record evict_eval would give a
// node that fits, without an evaluation.
template <int W>
__device__ __forceinline__ int ploop_plain_winner(const PLoopArgs& L, const PreemptArgs& A, uint32_t pos, uint32_t row,
                                               NodeEval* out, uint32_t* offers, uint32_t* unsup) {
    const uint32_t m = A.node_alloc_off[row + 1] - A.node_alloc_off[row];
    const uint32_t placeholders = A.soa.coll_job[row] - A.own_existing[row];
    out->status = kOption;
    out->score = L.sc_plain[pos];
    out->nscores = L.nparts_plain[pos];
    for (int k = 0; k < PE_MAX_SCORES; k++) out->parts[k] = L.parts_plain[(size_t)pos * PE_MAX_SCORES + k];
    if (m > EvW<W>::kAllocs || m + placeholders > EvW<W>::kL) {
        *unsup |= kEvictWider;
        return kFiltered;
    }
    uint32_t o = 0;
    const Ask& a = A.ask;
    if (a.n_dev > 0) {
        const DevClass& dc = A.tg.dev_cls[A.soa.rec[row].cls];
        uint32_t fr = A.tg.dev_free ? A.tg.dev_free[row] : 0u;
        for (int q = 0; q < kMaxDevReq && q < a.n_dev; q++) {
            const int g = assign_one(a, dc, q, fr);
            if (g < 0) return kSkipped;   // not a plain fit after all: the caller's winner check fails
            const uint32_t cnt = (uint32_t)a.dev_cnt[q];
            const uint32_t f = byte_of(fr, g);
            fr -= (cnt < f ? cnt : f) << (8 * g);
            o |= (uint32_t)g << (8 * q);
        }
    }
    *offers = o;
    return kOption;
}

__device__ __forceinline__ int64_t readlane64(int64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Plan.AppendPreemptedAlloc of the masked allocs (apply_preempt) and
// Plan.AppendAlloc of the placement (commit_row<false>) in one pass of wave 0:
// every load (the row's counters on lane 0, the masked allocs one per lane)
// issues before the first store, so the commit costs two round trips (the
// row's alloc offsets, then its allocs) however many allocs it evicts.
// `mask` and `offers` are uniform; evicted sums move to lane 0 by readlane.
template <int W>
__device__ __forceinline__ void ploop_commit(const PLoopArgs& L, uint32_t row, const AMask<W>& mask, bool evict,
                                             uint32_t offers) {
    const int lane = (int)(threadIdx.x & 63u);
    const NodeSoA& s = L.P.soa;
    const TgTables& t = L.P.tg;
    const Ask& a = L.P.ask;
    // apply_preempt's dev_free and commit_row's tg.dev_free are one buffer (d_dev_free)
    uint32_t* const df = L.dev_free ? L.dev_free : (a.n_dev > 0 ? t.dev_free : nullptr);
    const bool cores = evict && L.P.palloc_cores && s.core_used;
    NodeRec& r = s.rec[row];
    int64_t cpu = 0, mem = 0, disk = 0;
    int32_t mbits = 0, dyn = 0;
    uint32_t cls = 0, cj = 0, ct = 0, fr = 0;
    uint64_t cu[4] = {0, 0, 0, 0};
    if (lane == 0) {
        cpu = r.used_cpu;
        mem = r.used_mem;
        disk = r.used_disk;
        mbits = r.used_mbits;
        dyn = r.used_dyn;
        cls = r.cls;
        cj = s.coll_job[row];
        ct = t.coll_tg[row];
        if (df) fr = df[row];
        if (cores)
            for (int w = 0; w < 4; w++) cu[w] = s.core_used[4 * row + w];
    }
    int64_t ecpu = 0, emem = 0, edisk = 0;
    int32_t embits = 0, edyn = 0;
    uint32_t efr = 0;
    uint64_t ecores[4] = {0, 0, 0, 0};
    if (evict) {
        const uint32_t b = L.P.node_alloc_off[row];
        const uint32_t m = min(L.P.node_alloc_off[row + 1] - b, 32u * W);
#pragma unroll
        for (int k = 0; k < (32 * W + 63) / 64; k++) {
            const uint32_t i = 64u * k + (uint32_t)lane;
            const uint32_t word = (lane < 32 || 2 * k + 1 >= W) ? mask.w[2 * k] : mask.w[2 * k + 1];
            const bool want = i < m && ((word >> (i & 31u)) & 1u);
            uint32_t pz = 1;
            PreemptAlloc x;
            if (want) {
                pz = L.preempted[b + i];
                x = L.P.allocs[b + i];
            }
            const bool ev = want && pz == 0u;
            uint32_t dfr = 0;
            if (ev)
                for (int q = 0; q < 4 && q < (int)x.n_dev; q++) dfr += byte_of(x.dev_c, q) << (8 * byte_of(x.dev_g, q));
            for (uint64_t bal = __ballot(ev); bal; bal &= bal - 1) {
                const int l = __builtin_ctzll(bal);
                ecpu += readlane64(x.cpu, l);
                emem += readlane64(x.mem, l);
                edisk += readlane64(x.disk, l);
                embits += __builtin_amdgcn_readlane(x.mbits, l);
                edyn += __builtin_amdgcn_readlane(x.dyn, l);
                efr += (uint32_t)__builtin_amdgcn_readlane((int)dfr, l);
            }
            if (cores && __ballot(ev)) {
                for (int w = 0; w < 4; w++) {
                    uint64_t c = ev ? L.P.palloc_cores[4 * (size_t)(b + i) + w] : 0ull;
                    for (int off = 32; off > 0; off >>= 1) c |= (uint64_t)__shfl_xor((unsigned long long)c, off);
                    ecores[w] |= c;
                }
            }
            if (ev) {
                L.preempted[b + i] = 1;
                atomicAdd(&L.pcount[x.jtg_key], 1u);
            }
        }
    }
    if (lane != 0) return;
    fr += efr;
    if (a.n_dev > 0) {
        if (offers == 0xFFFFFFFFu) {
            fr = dev_after(a, t.dev_cls[cls], fr, 1);
        } else {
            for (int q = 0; q < kMaxDevReq && q < a.n_dev; q++) {
                const uint32_t g = (offers >> (8 * q)) & 255u, f = (fr >> (8 * g)) & 255u;
                const uint32_t cnt = (uint32_t)a.dev_cnt[q];
                fr -= (cnt < f ? cnt : f) << (8 * g);
            }
        }
    }
    r.used_cpu = cpu - ecpu + a.cpu;
    r.used_mem = mem - emem + a.mem;
    r.used_disk = disk - edisk + a.disk;
    r.used_mbits = mbits - embits + a.commit_mbits;
    r.used_dyn = dyn - edyn + a.commit_dyn;
    s.coll_job[row] = cj + 1u;
    t.coll_tg[row] = ct + 1u;
    if (df && (evict || a.n_dev > 0)) df[row] = fr;
    if (cores)
        for (int w = 0; w < 4; w++) s.core_used[4 * row + w] = cu[w] & ~ecores[w];
    for (int p = 0; p < t.n_psets; p++) {
        const uint32_t v = pset_value(t, p, row, cls);
        if (v != kMissing) t.pset_counts[p][v] += 1;
    }
}

template <int W>
__global__ void __launch_bounds__(kPLoopBlock) k_ploop(PLoopArgs L) {
    extern __shared__ uint32_t ploop_dyn[];
    __shared__ PLoopShared sh;
    // index lists of the single-lane evaluations: one per refreshing wave, one for the winner
    __shared__ EvictWs<W> ews[kPLoopStage + 1];
    // the evaluations' arguments in LDS: their many field reads do not go
    // through the vector L1 the resolves stream through
    __shared__ PreemptArgs pa;
    static_assert(sizeof(PreemptArgs) % 4 == 0, "word copy");
    for (uint32_t i = (uint32_t)threadIdx.x; i < sizeof(PreemptArgs) / 4; i += kPLoopBlock)
        reinterpret_cast<uint32_t*>(&pa)[i] = reinterpret_cast<const uint32_t*>(&L.P)[i];
    const int tid = threadIdx.x;
    const uint32_t n = L.P.n_visit, nw = (n + 15u) >> 4;
    const uint32_t nd32 = (n + 31u) >> 5;
    uint32_t* cp = ploop_dyn;            // plain outcomes
    uint32_t* ce = ploop_dyn + nw;       // Preempt outcomes
    uint32_t* dep = ploop_dyn + 2 * nw;  // Preempt outcomes that read the plan's preemption counts
    for (uint32_t w = (uint32_t)tid; w < nd32; w += kPLoopBlock) {
        uint32_t x = 0;
        if (L.dep_init)
            for (uint32_t i = 0; i < 32u; i++) {
                const uint32_t p = w * 32u + i;
                if (p < n && L.dep_init[p]) x |= 1u << i;
            }
        dep[w] = x;
    }
    for (uint32_t w = (uint32_t)tid; w < nw; w += kPLoopBlock) {
        uint32_t xp = 0, xe = 0;
        for (uint32_t i = 0; i < 16u; i++) {
            const uint32_t p = w * 16u + i;
            const uint32_t a = p < n ? (uint32_t)L.st_plain[p] : 3u;
            const uint32_t b = p < n ? (uint32_t)L.P.status[p] : 3u;
            xp |= (a & 3u) << (2u * i);
            xe |= (b & 3u) << (2u * i);
        }
        cp[w] = xp;
        ce[w] = xe;
    }
    if (tid == 0) { sh.n_dirty = 0; sh.dirty_all = 0; sh.pcount_changed = 0; sh.flags = 0; sh.n_live = 0; }
    __syncthreads();
    // the plain summary: one wave per block
    for (uint32_t blk = (uint32_t)tid >> 6; blk * kPLoopSpan < n; blk += kPLoopBlock / 64) {
        uint32_t o = 0, f = 0, e = 0;
        for (uint32_t w = blk * (kPLoopSpan / 16u) + ((uint32_t)tid & 63u); w < min((blk + 1u) * (kPLoopSpan / 16u), nw);
             w += 64u) {
            const uint32_t x = cp[w];   // positions past n hold kSkipped (3): counted nowhere
            o += (uint32_t)__popc(~(x | (x >> 1)) & kCodeEven);
            f += (uint32_t)__popc(x & ~(x >> 1) & kCodeEven);
            e += (uint32_t)__popc((x >> 1) & ~x & kCodeEven);
        }
        o = wave_sum(o);
        f = wave_sum(f);
        e = wave_sum(e);
        if ((tid & 63) == 0) {
            sh.sum_plain.opt[blk] = o;
            sh.sum_plain.fil[blk] = f;
            sh.sum_plain.exh[blk] = e;
        }
    }
    __syncthreads();
    uint32_t offset = L.offset, p = 0, records = 0, err = 0;
    // profile (thread 0, wall clock ticks): plain resolve, refresh, Preempt resolve, winner; refreshed rows
    unsigned long long prof[7] = {0, 0, 0, 0, 0, 0, 0};   // [5] winner evict_eval, [6] its commit
    unsigned long long t0 = 0;
    // A plain Select fails only when no position holds a plain option (it then
    // consumed the whole list: the cursor stays), and a placement changes the
    // plain outcome of its own row only. So after a failed plain Select whose
    // placement left its row without a plain option, the next plain Select
    // fails too and is skipped.
    bool plain_dead = false;
    while (p < L.count) {
        if (L.prof) t0 = wall_clock64();
        int32_t win = -1;
        uint32_t no = offset;
        if (!plain_dead) {
            ploop_resolve(sh, cp, L.sc_plain, n, offset, L.limit, L.prof ? L.prof + 12 : nullptr, &sh.sum_plain);
            win = sh.res[0];
            no = (uint32_t)(((uint64_t)offset + (uint32_t)sh.res[1]) % n);
        } else if (L.check_dead) {
            // verification mode: the skipped resolve must fail
            ploop_resolve(sh, cp, L.sc_plain, n, offset, L.limit, L.prof ? L.prof + 12 : nullptr, &sh.sum_plain);
            if (sh.res[0] >= 0) { err = 3; records = p; break; }
        }
        if (L.prof) { const unsigned long long t = wall_clock64(); prof[0] += t - t0; t0 = t; }
        int mode = 0;
        if (win < 0) {
            if (!L.retry) {
                if (tid == 0) ploop_nil<W>(L, p, sh.res, no);
                records = p + 1;
                break;
            }
            if (L.nil_out) {   // the plain nil the Preempt retry follows (its record for served Selects)
                uint32_t ne = n, nf, nx;
                if (plain_dead) {
                    ploop_count_codes(sh, cp, n, &nf, &nx);
                } else {
                    ne = (uint32_t)sh.res[1];
                    nf = (uint32_t)sh.res[2];
                    nx = (uint32_t)sh.res[3];
                }
                if (tid == 0) {
                    uint32_t* o = L.nil_out + 4u * (size_t)p;
                    o[0] = ne;
                    o[1] = nf;
                    o[2] = nx;
                    o[3] = no;
                }
            }
            offset = no;
            // Preempt outcomes of the rows committed since their last refresh,
            // and after an eviction of every position that read the preemption
            // counts. Lazily (§25): the resolve depends only on the positions it
            // consumes, so it runs on the codes as they are; only dirty rows
            // inside its window are refreshed (then it runs again), the others
            // keep their stale code until a later window reaches them.
            const uint32_t nd = sh.n_dirty, all = sh.dirty_all, pc = sh.pcount_changed;
            bool any_dep = false;
            if (pc && !all) {
                bool mine = false;
                for (uint32_t w = (uint32_t)tid; w < nd32 && !mine; w += kPLoopBlock) mine = dep[w] != 0u;
                any_dep = __syncthreads_or(mine) != 0;
            }
            const bool lazy = !all && !any_dep && sh.n_live > 0;
            if (lazy) {
                // A refreshed row can move the window's end past another stale
                // row, so resolve → refresh the rows inside → resolve again
                // until the window holds none; every round retires ≥1 entry.
                for (;;) {
                    ploop_resolve(sh, ce, L.P.score, n, offset, L.limit, L.prof ? L.prof + 12 : nullptr);
                    const uint32_t consumed = (uint32_t)sh.res[1];
                    if (tid == 0) sh.n_hit = 0;
                    __syncthreads();
                    for (uint32_t d = (uint32_t)tid; d < nd; d += kPLoopBlock) {
                        const uint32_t q = sh.dirty[d];
                        if (q == PE_NONE || (q >= offset ? q - offset : q + n - offset) >= consumed) continue;
                        const uint32_t k = atomicAdd(&sh.n_hit, 1u);
                        if (k < (uint32_t)kPLoopStage) {   // refreshed below by its own wave
                            sh.hit[k] = q;
                            sh.dirty[d] = PE_NONE;
                            atomicSub(&sh.n_live, 1u);
                        }
                    }
                    __syncthreads();
                    const uint32_t nh = sh.n_hit;
                    if (nh == 0) break;
                    const uint32_t wv = (uint32_t)tid >> 6;
                    if (wv < min(nh, (uint32_t)kPLoopStage)) {
                        const uint32_t pos = sh.hit[wv];
                        const PreemptAlloc* na = ploop_stage(L.P, L.P.visit[pos], sh.stage[wv]);
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        ploop_refresh<W, true>(L, ce, dep, pos, &sh.flags, &ews[wv], na, &pa);
                    }
                    if (nh > (uint32_t)kPLoopStage) {
                        // more stale rows in the window than waves: the rest
                        // many lanes at once
                        __syncthreads();
                        EvictWs<W> pws;
                        for (uint32_t d = (uint32_t)tid; d < nd; d += kPLoopBlock) {
                            const uint32_t q = sh.dirty[d];
                            if (q == PE_NONE || (q >= offset ? q - offset : q + n - offset) >= consumed) continue;
                            ploop_refresh<W>(L, ce, dep, q, &sh.flags, &pws);
                            sh.dirty[d] = PE_NONE;
                            atomicSub(&sh.n_live, 1u);
                        }
                    }
                    if (L.prof && tid == 0) prof[4] += nh;
                    __syncthreads();
                    if (sh.flags) break;
                }
            } else {
                const uint32_t lim = all ? n : nd;
                if (!all && lim <= (uint32_t)kPLoopStage) {
                    // one wave per row, its alloc list staged in LDS, lane 0 evaluates
                    const uint32_t wv = (uint32_t)tid >> 6;
                    const uint32_t pos = wv < lim ? sh.dirty[wv] : PE_NONE;
                    if (pos != PE_NONE) {
                        const PreemptAlloc* na = ploop_stage(L.P, L.P.visit[pos], sh.stage[wv]);
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        ploop_refresh<W, true>(L, ce, dep, pos, &sh.flags, &ews[wv], na, &pa);
                    }
                } else {
                    EvictWs<W> pws;   // many lanes at once: private lists
                    for (uint32_t d = (uint32_t)tid; d < lim; d += kPLoopBlock) {
                        const uint32_t q = all ? d : sh.dirty[d];
                        if (q != PE_NONE) ploop_refresh<W>(L, ce, dep, q, &sh.flags, &pws);
                    }
                }
                if (L.prof && tid == 0) prof[4] += lim;
                if (pc && !all) {
                    __syncthreads();   // the dirty rows' dependency bits first
                    EvictWs<W> pws;
                    for (uint32_t w = (uint32_t)tid; w < nd32; w += kPLoopBlock)
                        for (uint32_t b = dep[w]; b; b &= b - 1u) {
                            ploop_refresh<W>(L, ce, dep, w * 32u + (uint32_t)__builtin_ctz(b), &sh.flags, &pws);
                            if (L.prof) atomicAdd(&L.prof[5], 1ull);
                        }
                }
            }
            __syncthreads();
            const uint32_t fl = sh.flags;
            __syncthreads();
            if (tid == 0) {
                if (!lazy) { sh.n_dirty = 0; sh.dirty_all = 0; sh.n_live = 0; }
                else if (sh.n_live == 0) sh.n_dirty = 0;
                sh.pcount_changed = 0;
            }
            if (fl) { err = (fl & 1u) ? 1u : 4u; records = p; break; }   // 4: rerun wider from here
            if (L.prof) { const unsigned long long t = wall_clock64(); prof[1] += t - t0; t0 = t; }
            if (!lazy) ploop_resolve(sh, ce, L.P.score, n, offset, L.limit, L.prof ? L.prof + 12 : nullptr);
            if (L.prof) { const unsigned long long t = wall_clock64(); prof[2] += t - t0; t0 = t; }
            win = sh.res[0];
            no = (uint32_t)(((uint64_t)offset + (uint32_t)sh.res[1]) % n);
            if (win < 0) {
                if (tid == 0) ploop_nil<W>(L, p, sh.res, no);
                records = p + 1;
                break;
            }
            mode = 1;
        }
        const PreemptAlloc* win_na = nullptr;   // the profile's evaluations only
        if (L.prof && tid < 64) win_na = ploop_stage(L.P, L.P.visit[ploop_pos(n, offset, (uint32_t)win)], sh.stage[0]);
        __syncthreads();
        const uint32_t pos = ploop_pos(n, offset, (uint32_t)win);
        const uint32_t row = L.P.visit[pos];
        NodeEval ev;
        AMask<W> mask = AMask<W>::zero();
        uint32_t offers = 0, unsup = 0;
        int st = kOption;
        if (tid < 64) {   // wave 0: the winner's record
            if (mode && L.P.parts_out) {
                // the Preempt outcome of this position is current (k_evict, or
                // refreshed since its row last changed): read its record
                ev.score = L.P.score[pos];
                ev.nscores = L.P.nparts_out[pos];
                for (int k = 0; k < PE_MAX_SCORES; k++) ev.parts[k] = L.P.parts_out[(size_t)pos * PE_MAX_SCORES + k];
                mask = AMask<W>::load(L.P.mask_out + (size_t)pos * W);
                offers = L.P.offers_out[pos];
            } else {
                if (tid == 0) st = ploop_plain_winner<W>(L, pa, pos, row, &ev, &offers, &unsup);
                if (L.prof) {   // the Preempt evaluation with its data cache-warm (profiling only)
                    bool d = false;
                    NodeEval ev2;
                    AMask<W> m2 = AMask<W>::zero();
                    uint32_t o2 = 0, u2 = 0;
                    bool d2 = false;
                    const unsigned long long c0 = wall_clock64();
                    (void)ploop_evict_eval<true, W>(pa, row, &ev2, &m2, &o2, &u2, &d, &ews[kPLoopStage], win_na);
                    const unsigned long long a0 = wall_clock64();
                    (void)ploop_evict_eval<true, W>(pa, row, &ev2, &m2, &o2, &u2, &d2, &ews[kPLoopStage], win_na);
                    if (tid == 0) {
                        L.prof[8] += wall_clock64() - a0;
                        L.prof[9] += 1;
                    }
                    // the next position's row right after: the code warm, its data cold
                    const uint32_t row2 = L.P.visit[pos + 1u < n ? pos + 1u : 0u];
                    const PreemptAlloc* na2 = ploop_stage(L.P, row2, sh.stage[1]);
                    wave_lds_sync();
                    const unsigned long long a1 = wall_clock64();
                    (void)ploop_evict_eval<true, W>(pa, row2, &ev2, &m2, &o2, &u2, &d2, &ews[kPLoopStage], na2);
                    if (tid == 0) {
                        L.prof[10] += wall_clock64() - a1;
                        L.prof[11] += 1;
                    }
                    t0 += wall_clock64() - c0;   // not charged to the winner's figures
                }
            }
        }
        const unsigned long long prof5_0 = prof[5], prof6_0 = prof[6];
        const unsigned long long tw = L.prof ? wall_clock64() : 0ull;
        // the plain winner's width check, offers and status are lane 0's
        const bool wider = (__builtin_amdgcn_readfirstlane(unsup) & kEvictWider) != 0u;
        if (!mode) mask = AMask<W>::zero();
#pragma unroll
        for (int i = 0; i < W; i++) mask.w[i] = (uint32_t)__builtin_amdgcn_readfirstlane(mask.w[i]);
        offers = (uint32_t)__builtin_amdgcn_readfirstlane(offers);
        const bool evict = mode && mask.any();
        if (tid < 64 && !wider)
            ploop_commit<W>(L, row, mask, evict, L.P.ask.n_dev > 0 ? offers : 0xFFFFFFFFu);
        if (tid == 0) {
            if (L.prof) {
                const unsigned long long t = wall_clock64();
                prof[5] += tw - t0;
                prof[6] += t - tw;
                if (!mode) { L.prof[20] += tw - t0; L.prof[21]++; }
            }
            if (wider) sh.flags |= 4u;   // the plain winner's ProposedAllocs outgrew the width
            else if (evict) sh.pcount_changed = 1;
        }
        if (tid == 0) {
          if (!(sh.flags & 4u)) {
            PLoopRec& o = sh.rec;
            o.row = row;
            o.score = st == kOption ? ev.score : 0.0;
            o.nscores = st == kOption ? ev.nscores : 0u;
            for (int k = 0; k < PE_MAX_SCORES; k++)
                o.parts[k] = (st == kOption && k < (int)ev.nscores) ? ev.parts[k] : 0.0;
            o.evaluated = (uint32_t)sh.res[1];
            o.filtered = (uint32_t)sh.res[2];
            o.exhausted = (uint32_t)sh.res[3];
            o.new_offset = no;
            o.n_dev = (st == kOption && L.P.ask.n_dev > 0) ? (uint32_t)L.P.ask.n_dev : 0u;
            o.offers = offers;
            for (int i = 0; i < W; i++) o.mask[i] = mask.w[i];
            // the committed row's plain outcome on the new state
            NodeEval pe;
            const unsigned long long pe0 = L.prof ? wall_clock64() : 0ull;
            if (L.prof) L.prof[17] += pe0 - t0 - prof[5] - prof[6] + prof5_0 + prof6_0;
            ploop_plain_eval(pa, row, &pe);
            if (L.prof) {
                L.prof[14] += wall_clock64() - pe0;
                L.prof[15] += 1;
            }
            L.sc_plain[pos] = pe.status == kOption ? pe.score : 0.0;
            if (pe.status == kOption) {
                L.nparts_plain[pos] = (uint8_t)pe.nscores;
                for (int k = 0; k < PE_MAX_SCORES; k++) L.parts_plain[(size_t)pos * PE_MAX_SCORES + k] = pe.parts[k];
            }
            {
                const uint32_t was = (cp[pos >> 4] >> (2u * (pos & 15u))) & 3u, now = (uint32_t)pe.status & 3u;
                const uint32_t blk = pos / kPLoopSpan;
                auto bump = [&](uint32_t c, uint32_t d) {
                    if (c == 0u) sh.sum_plain.opt[blk] += d;
                    else if (c == 1u) sh.sum_plain.fil[blk] += d;
                    else if (c == 2u) sh.sum_plain.exh[blk] += d;
                };
                bump(was, ~0u);
                bump(now, 1u);
            }
            ploop_set_code(cp, pos, (uint32_t)pe.status);
            sh.last_plain = (uint32_t)pe.status;
            if (sh.n_dirty == kPLoopDirtyCap && sh.n_live < kPLoopDirtyCap) {   // drop the refreshed entries
                uint32_t k = 0;
                for (uint32_t d = 0; d < kPLoopDirtyCap; d++)
                    if (sh.dirty[d] != PE_NONE) sh.dirty[k++] = sh.dirty[d];
                sh.n_dirty = k;
            }
            if (sh.n_dirty < kPLoopDirtyCap) {
                sh.dirty[sh.n_dirty++] = pos;
                sh.n_live++;
            } else {
                sh.dirty_all = 1;
            }
            if (st != kOption) sh.flags |= 2u;   // the resolve's winner must be an option
            if (L.prof) L.prof[18] += wall_clock64() - pe0 - 0;
          }
        }
        const unsigned long long tsy = L.prof ? wall_clock64() : 0ull;
        __syncthreads();
        if (L.prof && tid == 0) L.prof[19] += wall_clock64() - tsy;
        if (tid == 64 && !(sh.flags & 4u)) {   // wave 1: the record, while wave 0 goes on
            const PLoopRec& r = sh.rec;
            pe_ranked_node& o = L.out[p];
            o.row = (int32_t)r.row;
            o.final_score = r.score;
            o.n_scores = r.nscores;
            for (int k = 0; k < PE_MAX_SCORES; k++) o.scores[k] = r.parts[k];
            o.nodes_evaluated = r.evaluated;
            o.nodes_filtered = r.filtered;
            o.nodes_exhausted = r.exhausted;
            o.new_offset = r.new_offset;
            o.n_preempted = 0;
            o.n_device_offers = r.n_dev;
            for (int q = 0; q < PE_MAX_DEVICE_REQ; q++) o.device_offer_group[q] = byte_of(r.offers, q);
            for (int i = 0; i < W; i++) L.out_mask[(size_t)p * W + i] = r.mask[i];
        }
        if (sh.flags & 4u) { err = 4; records = p; break; }   // nothing applied: this placement reruns wider
        if (L.prof) prof[3] += wall_clock64() - t0;
        if (sh.flags & 2u) { err = 2; records = p + 1; p++; break; }
        plain_dead = mode == 1 && sh.last_plain != (uint32_t)kOption;
        offset = no;
        p++;
        records = p;
    }
    if (tid == 0) {
        L.state[0] = p;
        L.state[1] = offset;
        L.state[2] = err;
        L.state[3] = records;
        if (L.prof) {
            for (int k = 0; k < 5; k++) L.prof[k] = prof[k];
            L.prof[6] = prof[5];
            L.prof[7] = prof[6];
        }
    }
}
