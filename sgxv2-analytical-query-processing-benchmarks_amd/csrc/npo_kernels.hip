// No-partitioning hash join on gfx950: the reference's PHT_overflow / PHT_int
// (no_partitioning_hash_join.cpp:51-88,166-249, probe HashLinkTableCommon.cpp:54-89)
// as two kernels over one global table in HBM.  Layout: npo_internal.hpp.
//
//   k_npo_build  R -> table: one returning atomic add on the bucket's count per tuple;
//                slots 0 and 1 take the key with a store, later tuples take a node from
//                the pool (one cursor add per wave) and push it at the bucket's head.
//   k_npo_probe  S -> count (or triples): K bucket loads in flight per thread, slots
//                compared below count, the chain walked while next is set.
//
// Nothing reads the table during the build: the probe sees it through the kernel
// boundary.  Both kernels read their relation with 16-byte non-temporal loads, two
// tuples per load, several loads in flight (the input read of k_scatter_pool); a
// relation that starts on an odd tuple gives its first and last tuple to one wave.
#include "common.hpp"
#include "npo_internal.hpp"

namespace sgxamd {
namespace npo {

namespace {

constexpr int kNpoBlock = 256;
constexpr int kBuildLoads = 4;  // 16-byte loads (8 tuples) per thread and step
constexpr int kProbeLoads = 4;  // materialising probe: 8 keys, 8 bucket loads in flight
constexpr uint32_t kMaxGrid = 2048;

// The relation as an optional head tuple, 16-byte pairs and an optional tail tuple.
struct Split {
    const uint4 *body;
    uint64_t pairs;
    bool head, tail;
};
__device__ __forceinline__ Split split_relation(const row_t *T, uint64_t n) {
    Split sp;
    sp.head = n > 0 && ((reinterpret_cast<uintptr_t>(T) >> 3) & 1);
    sp.body = reinterpret_cast<const uint4 *>(T + (sp.head ? 1 : 0));
    const uint64_t rest = n - (sp.head ? 1 : 0);
    sp.pairs = rest >> 1;
    sp.tail = rest & 1;
    return sp;
}

template <bool WT>
__device__ __forceinline__ void st_u32(uint32_t *p, uint32_t v) {
    if (WT)
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *p = v;
}
template <bool WT>
__device__ __forceinline__ void st_u64(uint64_t *p, uint64_t v) {
    if (WT)
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *p = v;
}

// The returning add on the bucket's count: the tuple's position in its bucket.
__device__ __forceinline__ uint32_t take_slot(const Table &t, uint32_t key, bool valid) {
    uint32_t *bw = reinterpret_cast<uint32_t *>(t.buckets + (key & t.mask));
    return valid ? __hip_atomic_fetch_add(bw, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
}

// One tuple per lane (valid: this lane has one) at position slot of its bucket.  Called
// by whole waves: the node allocation is one cursor add per wave.
template <bool PAY, bool WT>
__device__ __forceinline__ void place(const Table &t, uint32_t key, uint32_t pay, uint32_t slot, bool valid) {
    const uint32_t b = key & t.mask;
    uint32_t *bw = reinterpret_cast<uint32_t *>(t.buckets + b);
    if (valid && slot < kBucketCap) {
        st_u32<WT>(bw + 2 + slot, key);
        if (PAY) st_u32<WT>(t.bpay + 2ull * b + slot, pay);
    }
    const bool ovf = valid && slot >= kBucketCap;
    const uint64_t m = __ballot(ovf);
    if (m) {  // wave-uniform
        const uint32_t leader = (uint32_t)__builtin_ctzll(m);
        uint32_t base = 0;
        if (__lane_id() == leader)
            base = __hip_atomic_fetch_add(t.ctrl + kCtrlCursor, popc64(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        base = __shfl(base, (int)leader, kWave);
        const uint32_t idx = base + popc64(m & lanemask_lt());
        // a pool that is too small: the nodes are only counted and the host runs the
        // join again with a pool that holds them
        if (ovf && idx < t.pool_cap) {
            const uint32_t old = __hip_atomic_exchange(bw + 1, idx + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            st_u64<WT>(reinterpret_cast<uint64_t *>(t.nodes + idx), ((uint64_t)old << 32) | key);
            if (PAY) st_u32<WT>(t.npay + idx, pay);
        }
    }
}

template <bool PAY, bool WT>
__global__ __launch_bounds__(kNpoBlock) void k_npo_build(const row_t *__restrict__ R, uint64_t n, Table t) {
    const Split sp = split_relation(R, n);
    const uint64_t tid = (uint64_t)blockIdx.x * kNpoBlock + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * kNpoBlock;
    // the bound is the same for every thread, so whole waves reach place()
    for (uint64_t it = 0; it < sp.pairs; it += stride * kBuildLoads) {
        uint4 v[kBuildLoads];
        bool ok[kBuildLoads];
#pragma unroll
        for (int j = 0; j < kBuildLoads; ++j) {
            const uint64_t i = it + (uint64_t)j * stride + tid;
            ok[j] = i < sp.pairs;
            v[j] = ok[j] ? ld_nt(sp.body + i) : make_uint4(0, 0, 0, 0);
        }
        // all the step's count adds are issued before the first slot is used
        uint32_t slot[2 * kBuildLoads];
#pragma unroll
        for (int j = 0; j < kBuildLoads; ++j) {
            slot[2 * j] = take_slot(t, v[j].x, ok[j]);
            slot[2 * j + 1] = take_slot(t, v[j].z, ok[j]);
        }
#pragma unroll
        for (int j = 0; j < kBuildLoads; ++j) {
            place<PAY, WT>(t, v[j].x, v[j].y, slot[2 * j], ok[j]);
            place<PAY, WT>(t, v[j].z, v[j].w, slot[2 * j + 1], ok[j]);
        }
    }
    if (tid < kWave && (sp.head || sp.tail)) {  // the first wave: the odd tuples
        const bool mine = (tid == 0 && sp.head) || (tid == 1 && sp.tail);
        const row_t r = mine ? R[tid == 0 ? 0 : n - 1] : row_t{0, 0};
        place<PAY, WT>(t, r.key, r.payload, take_slot(t, r.key, mine), mine);
    }
}

// Matches of key k in its bucket bk (count variant).
__device__ __forceinline__ uint64_t count_key(const Table &t, uint4 bk, uint32_t k) {
    uint64_t m = (bk.x > 0 && bk.z == k) + (bk.x > 1 && bk.w == k);
    uint32_t nxt = bk.y;
    while (nxt) {
        const uint2 nd = t.nodes[nxt - 1];
        m += nd.x == k;
        nxt = nd.y;
    }
    return m;
}

// Adds the block's matches to the result word: per wave, then one atomic per workgroup.
__device__ __forceinline__ void report_matches(const Table &t, uint64_t m) {
    __shared__ uint64_t wsum[kNpoBlock / kWave];
    m = wave_sum_u64(m);
    if (__lane_id() == 0) wsum[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t tot = 0;
        for (int w = 0; w < kNpoBlock / kWave; ++w) tot += wsum[w];
        if (tot)
            __hip_atomic_fetch_add(reinterpret_cast<uint64_t *>(t.ctrl) + kCtrlMatches, tot, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int L>
__global__ __launch_bounds__(kNpoBlock) void k_npo_probe(const row_t *__restrict__ S, uint64_t n, Table t) {
    const Split sp = split_relation(S, n);
    const uint64_t tid = (uint64_t)blockIdx.x * kNpoBlock + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * kNpoBlock;
    uint64_t m = 0;
    for (uint64_t it = 0; it < sp.pairs; it += stride * L) {
        uint4 v[L];
        bool ok[L];
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const uint64_t i = it + (uint64_t)j * stride + tid;
            ok[j] = i < sp.pairs;
            v[j] = ok[j] ? ld_nt(sp.body + i) : make_uint4(0, 0, 0, 0);
        }
        // every bucket load of the step is issued before the first one is consumed
        uint4 b[2 * L];
#pragma unroll
        for (int j = 0; j < L; ++j) {
            b[2 * j] = t.buckets[v[j].x & t.mask];
            b[2 * j + 1] = t.buckets[v[j].z & t.mask];
        }
#pragma unroll
        for (int j = 0; j < L; ++j) {
            if (ok[j]) m += count_key(t, b[2 * j], v[j].x) + count_key(t, b[2 * j + 1], v[j].z);
        }
    }
    if (blockIdx.x == 0 && ((threadIdx.x == 0 && sp.head) || (threadIdx.x == 1 && sp.tail))) {
        const uint32_t k = S[threadIdx.x == 0 ? 0 : n - 1].key;
        m += count_key(t, t.buckets[k & t.mask], k);
    }
    report_matches(t, m);
}

// One S tuple per lane, whole waves: the lanes' match counts are scanned and the wave
// takes its output range with one cursor add, then every lane walks its bucket again
// and writes.  Returns the lane's matches.
__device__ __forceinline__ uint64_t emit_key(const Table &t, uint4 bk, uint32_t k, uint32_t spay, bool valid,
                                             output_triple_t *out, uint64_t cap) {
    const uint64_t cnt = valid ? count_key(t, bk, k) : 0;
    const uint64_t incl = wave_incl_scan_u64(cnt);
    const uint64_t total = __shfl(incl, kWave - 1, kWave);
    if (total == 0) return 0;  // wave-uniform
    uint64_t base = 0;
    if (__lane_id() == 0)
        base = __hip_atomic_fetch_add(reinterpret_cast<uint64_t *>(t.ctrl) + kCtrlOut, total, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, 0, kWave);
    uint64_t pos = base + incl - cnt;
    if (cnt) {
        const uint64_t b = k & t.mask;
        auto put = [&](uint32_t rpay) {
            if (pos < cap) out[pos] = output_triple_t{k, rpay, spay};
            ++pos;
        };
        if (bk.x > 0 && bk.z == k) put(t.bpay[2 * b]);
        if (bk.x > 1 && bk.w == k) put(t.bpay[2 * b + 1]);
        uint32_t nxt = bk.y;
        while (nxt) {
            const uint2 nd = t.nodes[nxt - 1];
            if (nd.x == k) put(t.npay[nxt - 1]);
            nxt = nd.y;
        }
    }
    return cnt;
}

__global__ __launch_bounds__(kNpoBlock) void k_npo_probe_mat(const row_t *__restrict__ S, uint64_t n, Table t,
                                                             output_triple_t *__restrict__ out, uint64_t cap) {
    const Split sp = split_relation(S, n);
    const uint64_t tid = (uint64_t)blockIdx.x * kNpoBlock + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * kNpoBlock;
    uint64_t m = 0;
    for (uint64_t it = 0; it < sp.pairs; it += stride * kProbeLoads) {
        uint4 v[kProbeLoads];
        bool ok[kProbeLoads];
#pragma unroll
        for (int j = 0; j < kProbeLoads; ++j) {
            const uint64_t i = it + (uint64_t)j * stride + tid;
            ok[j] = i < sp.pairs;
            v[j] = ok[j] ? ld_nt(sp.body + i) : make_uint4(0, 0, 0, 0);
        }
        uint4 b[2 * kProbeLoads];
#pragma unroll
        for (int j = 0; j < kProbeLoads; ++j) {
            b[2 * j] = t.buckets[v[j].x & t.mask];
            b[2 * j + 1] = t.buckets[v[j].z & t.mask];
        }
#pragma unroll
        for (int j = 0; j < kProbeLoads; ++j) {
            m += emit_key(t, b[2 * j], v[j].x, v[j].y, ok[j], out, cap);
            m += emit_key(t, b[2 * j + 1], v[j].z, v[j].w, ok[j], out, cap);
        }
    }
    if (tid < kWave && (sp.head || sp.tail)) {
        const bool mine = (tid == 0 && sp.head) || (tid == 1 && sp.tail);
        const row_t r = mine ? S[tid == 0 ? 0 : n - 1] : row_t{0, 0};
        m += emit_key(t, t.buckets[r.key & t.mask], r.key, r.payload, mine, out, cap);
    }
    report_matches(t, m);
}

inline uint32_t grid_for(uint64_t n, int loads) {
    const uint64_t per_block = (uint64_t)kNpoBlock * loads;  // pairs per workgroup and step
    const uint64_t g = ((n >> 1) + per_block - 1) / per_block;
    return (uint32_t)(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g);
}

}  // namespace

hipError_t launch_build(const row_t *R, uint64_t n, const Table &t, bool write_through, hipStream_t s) {
    const dim3 grid(grid_for(n, kBuildLoads)), block(kNpoBlock);
    if (t.bpay) {
        if (write_through)
            hipLaunchKernelGGL((k_npo_build<true, true>), grid, block, 0, s, R, n, t);
        else
            hipLaunchKernelGGL((k_npo_build<true, false>), grid, block, 0, s, R, n, t);
    } else {
        if (write_through)
            hipLaunchKernelGGL((k_npo_build<false, true>), grid, block, 0, s, R, n, t);
        else
            hipLaunchKernelGGL((k_npo_build<false, false>), grid, block, 0, s, R, n, t);
    }
    return hipGetLastError();
}

hipError_t launch_probe(const row_t *S, uint64_t n, const Table &t, int keys_in_flight, hipStream_t s) {
    const dim3 block(kNpoBlock);
    if (keys_in_flight == 4)
        hipLaunchKernelGGL(k_npo_probe<2>, dim3(grid_for(n, 2)), block, 0, s, S, n, t);
    else if (keys_in_flight == 16)
        hipLaunchKernelGGL(k_npo_probe<8>, dim3(grid_for(n, 8)), block, 0, s, S, n, t);
    else
        hipLaunchKernelGGL(k_npo_probe<4>, dim3(grid_for(n, 4)), block, 0, s, S, n, t);
    return hipGetLastError();
}

hipError_t launch_probe_materialize(const row_t *S, uint64_t n, const Table &t, output_triple_t *out, uint64_t cap,
                                    hipStream_t s) {
    hipLaunchKernelGGL(k_npo_probe_mat, dim3(grid_for(n, kProbeLoads)), dim3(kNpoBlock), 0, s, S, n, t, out, cap);
    return hipGetLastError();
}

}  // namespace npo
}  // namespace sgxamd
