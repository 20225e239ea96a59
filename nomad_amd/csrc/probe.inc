// Test probes of the fp64 scoring math and of Go's sort.Slice (included by
// kernels.hip after namespace pe; pe_probe_math / pe_probe_go_sort in
// include/nomad_pe.h). Each probe calls the function the kernels call, on the
// host (device = 0, no GPU needed) or from a trivial kernel with one input per
// lane (device = 1), so a test can compare the gfx950 code object with the host
// build of the same header bit for bit. Nothing on the placement path calls
// them.

namespace pe {

// One item of a scalar op; the result as raw bits (order_key's is the key).
__host__ __device__ __forceinline__ uint64_t probe_math_one(uint32_t op, const double* xd, const int64_t* xi, uint32_t i,
                                                            double log10) {
    switch (op) {
        case PE_PROBE_POW10_UNIT: return gm::f2u(gm::pow10_unit(xd[i], log10));
        case PE_PROBE_POW10: return gm::f2u(gm::pow10_go(xd[i], log10));
        case PE_PROBE_EXP: return gm::f2u(gm::exp_go(xd[i]));
        case PE_PROBE_LOG: return gm::f2u(gm::log_go(xd[i]));
        case PE_PROBE_POW2: return gm::f2u(pow2_go(xd[i]));
        case PE_PROBE_ORDER_KEY: return (uint64_t)order_key(xd[i]);
        case PE_PROBE_FIT_SCORE: {
            const int64_t* v = xi + 5u * (size_t)i;
            return gm::f2u(gm::fit_score(v[0], v[1], v[2], v[3], v[4] != 0, log10));
        }
        case PE_PROBE_BASIC_DISTANCE: {
            const int64_t* v = xi + 6u * (size_t)i;
            PreemptAlloc u{};
            u.cpu = v[3];
            u.mem = v[4];
            u.disk = v[5];
            return gm::f2u(basic_distance(v[0], v[1], v[2], u));
        }
        default: return 0;
    }
}

// preemption_score over a node of `count` allocs, all of them preempted
template <int W>
__host__ __device__ __forceinline__ uint64_t probe_pscore(const PreemptAlloc* na, uint32_t count) {
    EvictCtx<W> c;
    c.A = nullptr;
    c.na = na;
    c.m = count;
    c.L = c.t0 = c.t1 = c.t2 = nullptr;
    c.key = nullptr;
    c.nL = 0;
    c.unsupported = false;
    AMask<W> mask = AMask<W>::zero();
    for (uint32_t i = 0; i < count; i++) mask.set(i);
    return gm::f2u(preemption_score(c, mask));
}

__host__ __device__ __forceinline__ uint64_t probe_pscore_one(const PreemptAlloc* na, const uint32_t* off, uint32_t i) {
    const uint32_t count = off[i + 1] - off[i];
    return count <= EvW<1>::kAllocs ? probe_pscore<1>(na + off[i], count) : probe_pscore<8>(na + off[i], count);
}

// The Preemptor's keyed sort of the identity permutation of array `a`
// (keys[off[a] .. off[a + 1])); `idx` is scratch of the arrays' total length.
template <class Idx>
__host__ __device__ __forceinline__ void probe_sort_one(const double* keys, const uint32_t* off, uint32_t a, Idx* idx,
                                                        uint32_t* perm) {
    const uint32_t lo = off[a], n = off[a + 1] - lo;
    for (uint32_t i = 0; i < n; i++) idx[lo + i] = (Idx)i;
    go_sort_keyed<Idx>(idx + lo, (int)n, keys + lo);
    for (uint32_t i = 0; i < n; i++) perm[lo + i] = idx[lo + i];
}

__global__ void k_probe_math(uint32_t op, const double* xd, const int64_t* xi, uint32_t n, double log10, uint64_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = probe_math_one(op, xd, xi, i, log10);
}

__global__ void k_probe_pscore(const PreemptAlloc* na, const uint32_t* off, uint32_t n, uint64_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = probe_pscore_one(na, off, i);
}

template <class Idx>
__global__ void k_probe_sort(const double* keys, const uint32_t* off, uint32_t n_arrays, Idx* idx, uint32_t* perm) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < n_arrays) probe_sort_one<Idx>(keys, off, a, idx, perm);
}

// Device buffers of one probe call, freed when it returns.
struct ProbeBufs {
    void* p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int n = 0;
    bool ok = true;
    void* alloc(size_t bytes, const void* src) {
        void* d = nullptr;
        if (!ok || hipMalloc(&d, bytes ? bytes : 1) != hipSuccess) { ok = false; return nullptr; }
        p[n++] = d;
        if (src && bytes && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) ok = false;
        return d;
    }
    ~ProbeBufs() {
        for (int i = 0; i < n; i++) (void)hipFree(p[i]);
    }
};

static bool probe_have_device() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

static bool probe_finish(void* out_host, const void* out_dev, size_t bytes) {
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return false;
    return !bytes || hipMemcpy(out_host, out_dev, bytes, hipMemcpyDeviceToHost) == hipSuccess;
}

}  // namespace pe

extern "C" int pe_probe_math(uint32_t op, const double* xd, const int64_t* xi, uint32_t n, uint64_t* out, int device) {
    using namespace pe;
    if (op > PE_PROBE_PREEMPTION_SCORE || (n && !out)) return PE_EINVAL;
    const bool ints = op == PE_PROBE_FIT_SCORE || op == PE_PROBE_BASIC_DISTANCE || op == PE_PROBE_PREEMPTION_SCORE;
    if (n && (ints ? !xi : !xd)) return PE_EINVAL;
    if (!n) return PE_OK;
    const double log10 = gm::log_go(10.0);   // as the engine computes it, on the host
    if (op == PE_PROBE_PREEMPTION_SCORE) {
        // xi: n + 1 offsets, then the priorities they slice
        std::vector<uint32_t> off((size_t)n + 1);
        for (uint32_t i = 0; i <= n; i++) {
            const int64_t o = xi[i];
            if (o < 0 || o > 0x7FFFFFFF || (i == 0 && o != 0) || (i && o < xi[i - 1]) ||
                (i && o - xi[i - 1] > (int64_t)EvW<8>::kAllocs))
                return PE_EINVAL;
            off[i] = (uint32_t)o;
        }
        std::vector<PreemptAlloc> na(off[n]);
        for (uint32_t j = 0; j < off[n]; j++) {
            const int64_t p = xi[(size_t)n + 1 + j];
            if (p < -0x7FFFFFFF || p > 0x7FFFFFFF) return PE_EINVAL;
            na[j] = PreemptAlloc{};
            na[j].priority = (int32_t)p;
        }
        if (!device) {
            for (uint32_t i = 0; i < n; i++) out[i] = probe_pscore_one(na.data(), off.data(), i);
            return PE_OK;
        }
        if (!probe_have_device()) return PE_EHIP;
        ProbeBufs b;
        auto* d_na = (const PreemptAlloc*)b.alloc(sizeof(PreemptAlloc) * na.size(), na.data());
        auto* d_off = (const uint32_t*)b.alloc(sizeof(uint32_t) * off.size(), off.data());
        auto* d_out = (uint64_t*)b.alloc(sizeof(uint64_t) * n, nullptr);
        if (!b.ok) return PE_EHIP;
        hipLaunchKernelGGL(k_probe_pscore, dim3((n + 255u) / 256u), dim3(256), 0, 0, d_na, d_off, n, d_out);
        return probe_finish(out, d_out, sizeof(uint64_t) * n) ? PE_OK : PE_EHIP;
    }
    const size_t per = op == PE_PROBE_FIT_SCORE ? 5 : 6;
    if (!device) {
        for (uint32_t i = 0; i < n; i++) out[i] = probe_math_one(op, xd, xi, i, log10);
        return PE_OK;
    }
    if (!probe_have_device()) return PE_EHIP;
    ProbeBufs b;
    auto* d_xd = ints ? nullptr : (const double*)b.alloc(sizeof(double) * n, xd);
    auto* d_xi = ints ? (const int64_t*)b.alloc(sizeof(int64_t) * per * n, xi) : nullptr;
    auto* d_out = (uint64_t*)b.alloc(sizeof(uint64_t) * n, nullptr);
    if (!b.ok) return PE_EHIP;
    hipLaunchKernelGGL(k_probe_math, dim3((n + 255u) / 256u), dim3(256), 0, 0, op, d_xd, d_xi, n, log10, d_out);
    return probe_finish(out, d_out, sizeof(uint64_t) * n) ? PE_OK : PE_EHIP;
}

extern "C" int pe_probe_go_sort(const double* keys, const uint32_t* off, uint32_t n_arrays, uint32_t idx_width,
                                uint32_t* perm_out, int device) {
    using namespace pe;
    if (!off || (idx_width != 1u && idx_width != 2u) || off[0] != 0u) return PE_EINVAL;
    const uint32_t max_n = idx_width == 1u ? 255u : 65535u;   // every index below the type's placeholder value
    for (uint32_t a = 0; a < n_arrays; a++)
        if (off[a + 1] < off[a] || off[a + 1] - off[a] > max_n) return PE_EINVAL;
    const uint32_t total = off[n_arrays];
    if (total > 0x7FFFFFFFu || (total && (!keys || !perm_out))) return PE_EINVAL;
    if (!n_arrays || !total) return PE_OK;
    if (!device) {
        if (idx_width == 1u) {
            std::vector<uint8_t> idx(total);
            for (uint32_t a = 0; a < n_arrays; a++) probe_sort_one<uint8_t>(keys, off, a, idx.data(), perm_out);
        } else {
            std::vector<uint16_t> idx(total);
            for (uint32_t a = 0; a < n_arrays; a++) probe_sort_one<uint16_t>(keys, off, a, idx.data(), perm_out);
        }
        return PE_OK;
    }
    if (!probe_have_device()) return PE_EHIP;
    ProbeBufs b;
    auto* d_keys = (const double*)b.alloc(sizeof(double) * total, keys);
    auto* d_off = (const uint32_t*)b.alloc(sizeof(uint32_t) * ((size_t)n_arrays + 1), off);
    void* d_idx = b.alloc((size_t)idx_width * total, nullptr);
    auto* d_perm = (uint32_t*)b.alloc(sizeof(uint32_t) * total, nullptr);
    if (!b.ok) return PE_EHIP;
    const dim3 grid((n_arrays + 63u) / 64u), block(64);
    if (idx_width == 1u)
        hipLaunchKernelGGL(k_probe_sort<uint8_t>, grid, block, 0, 0, d_keys, d_off, n_arrays, (uint8_t*)d_idx, d_perm);
    else
        hipLaunchKernelGGL(k_probe_sort<uint16_t>, grid, block, 0, 0, d_keys, d_off, n_arrays, (uint16_t*)d_idx, d_perm);
    return probe_finish(perm_out, d_perm, sizeof(uint32_t) * total) ? PE_OK : PE_EHIP;
}
