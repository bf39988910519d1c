// Sort-merge join on gfx950: a device-wide stable LSD radix sort of tuples (or of their
// keys) and a merge join over the two sorted relations.  Geometry and workspace layout:
// smj_internal.hpp.  The only synchronisation between workgroups is the kernel boundary.
//
//   k_smj_min        input -> the relation's smallest key.  The sort orders by key - min,
//                    which is the order of the keys, so that a dense key range that does
//                    not start at 0 (the reference's primary keys 1..n) needs no pass for
//                    the one key that carries into the next digit.
//   k_smj_digits     input -> the relation's four 256-bin digit histograms of key - min;
//                    the host skips every pass whose histogram has a single non-empty bin.
//   per pass that runs:
//   k_smj_tile_hist  tile -> its 256 digit counts, written bin-major [digit][tile]
//   k_smj_scan       workgroup d turns row d into the global offsets of digit d's tiles:
//                    the digits below d come from the relation's histogram of this pass
//   k_smj_scatter    re-reads the tile, ranks every element among the tile's elements of
//                    its digit (wave-level match, below) and writes it to offset + rank
//   k_smj_partition  merge-path split of the merged sequence into chunks, R first on ties
//   k_smj_merge_*    one chunk per workgroup: R section in LDS, every S element of the
//                    chunk finds its R run there by binary search
#include "common.hpp"
#include "smj_internal.hpp"

namespace sgxamd {
namespace smj {

namespace {

constexpr uint32_t kSortWaves = kSortBlock / kWave;
constexpr uint32_t kWaveElems = kWave * kSortItems;  // consecutive elements of one wave
constexpr uint32_t kMaxGrid = 2048;

__device__ __forceinline__ uint32_t key_of(uint32_t e) { return e; }
__device__ __forceinline__ uint32_t key_of(uint64_t e) { return (uint32_t)e; }  // row_t: key first

// Block-wide exclusive scan of one u32 per thread (kSortBlock threads); scratch holds
// kSortWaves words.  Contains __syncthreads().
__device__ __forceinline__ uint32_t block_excl_scan_u32(uint32_t v, uint32_t *scratch, uint32_t *total) {
    const uint32_t wave = threadIdx.x / kWave;
    const uint32_t incl = wave_incl_scan_u32(v);
    if (__lane_id() == kWave - 1) scratch[wave] = incl;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < kSortWaves; ++w) {
        const uint32_t t = scratch[w];
        pre += w < wave ? t : 0u;
        tot += t;
    }
    __syncthreads();
    *total = tot;
    return pre + incl - v;
}

// The lanes of the wave that hold the same digit as this one (valid lanes only), found by
// one ballot per digit bit.
__device__ __forceinline__ uint64_t match_digit(uint32_t d, bool valid) {
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t m = __ballot(valid && bit);
        peers &= bit ? m : ~m;
    }
    return valid ? peers : 0ull;
}

// One count into an LDS histogram per valid lane; a wave whose lanes all hold the same
// digit (the constant high digits of small keys) adds once.
__device__ __forceinline__ void lds_count(uint32_t *h, uint32_t d, bool valid) {
    const uint64_t vm = __ballot(valid);
    if (vm == 0) return;
    const uint32_t d0 = __shfl(d, (int)__builtin_ctzll(vm), kWave);
    if (__ballot(valid && d != d0) == 0) {
        if (__lane_id() == (uint32_t)__builtin_ctzll(vm)) atomicAdd(&h[d0], popc64(vm));
    } else if (valid) {
        atomicAdd(&h[d], 1u);
    }
}

// *inv_min = max(~key): the complement, so that the cleared word is the neutral element.
__global__ __launch_bounds__(kSortBlock) void k_smj_min(const uint64_t *__restrict__ in, uint64_t n,
                                                        uint32_t *__restrict__ inv_min) {
    const uint64_t stride = (uint64_t)gridDim.x * kSortBlock;
    uint32_t m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x; i < n; i += stride)
        m = max(m, ~key_of(ld_nt(in + i)));
    m = wave_max_u32(m);
    if (__lane_id() == 0) atomicMax(inv_min, m);
}

__global__ __launch_bounds__(kSortBlock) void k_smj_digits(const uint64_t *__restrict__ in, uint64_t n,
                                                           uint32_t *__restrict__ ghist,
                                                           const uint32_t *__restrict__ inv_min) {
    const uint32_t bias = ~*inv_min;
    __shared__ uint32_t h[kPasses * kDigits];
    for (uint32_t i = threadIdx.x; i < kPasses * kDigits; i += kSortBlock) h[i] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * kSortBlock;
    // the bound is the same for every thread of a wave's step, so whole waves reach lds_count
    for (uint64_t it = (uint64_t)blockIdx.x * kSortBlock; it < n; it += stride) {
        const uint64_t i = it + threadIdx.x;
        const bool valid = i < n;
        const uint32_t k = valid ? key_of(ld_nt(in + i)) - bias : 0u;
#pragma unroll
        for (uint32_t p = 0; p < kPasses; ++p) lds_count(h + p * kDigits, (k >> (8 * p)) & 255u, valid);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kPasses * kDigits; i += kSortBlock)
        if (h[i]) atomicAdd(&ghist[i], h[i]);
}

template <typename In>
__global__ __launch_bounds__(kSortBlock) void k_smj_tile_hist(const In *__restrict__ src, uint32_t n, uint32_t bias,
                                                              uint32_t shift,
                                                              uint32_t *__restrict__ tile_hist, uint32_t tiles) {
    __shared__ uint32_t h[kDigits];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kSortTile;  // < n <= 2^31
#pragma unroll 4
    for (uint32_t j = 0; j < kSortItems; ++j) {
        const uint32_t i = base + j * kSortBlock + threadIdx.x;
        const bool valid = i < n;
        const uint32_t k = valid ? key_of(src[i]) - bias : 0u;
        lds_count(h, (k >> shift) & 255u, valid);
    }
    __syncthreads();
    tile_hist[(size_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// Workgroup d: row d of the bin-major counters becomes exclusive global offsets.
__global__ __launch_bounds__(kSortBlock) void k_smj_scan(uint32_t *__restrict__ tile_hist, uint32_t tiles,
                                                         const uint32_t *__restrict__ ghist_pass) {
    __shared__ uint32_t scratch[kSortWaves];
    __shared__ uint32_t below[kDigits];
    uint32_t total;
    below[threadIdx.x] = block_excl_scan_u32(ghist_pass[threadIdx.x], scratch, &total);
    __syncthreads();
    uint32_t carry = below[blockIdx.x];
    uint32_t *row = tile_hist + (size_t)blockIdx.x * tiles;
    constexpr uint32_t kPer = 16;  // consecutive counters per thread and step
    for (uint32_t t0 = 0; t0 < tiles; t0 += kSortBlock * kPer) {
        const uint32_t first = t0 + threadIdx.x * kPer;
        uint32_t v[kPer], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) {
            v[j] = first + j < tiles ? row[first + j] : 0u;
            sum += v[j];
        }
        uint32_t acc = carry + block_excl_scan_u32(sum, scratch, &total);
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) {
            if (first + j < tiles) row[first + j] = acc;
            acc += v[j];
        }
        carry += total;
    }
}

template <typename In, typename E, bool STAGED>
__global__ __launch_bounds__(kSortBlock) void k_smj_scatter(const In *__restrict__ src, uint32_t n, E *__restrict__ dst,
                                                            uint32_t bias, uint32_t shift,
                                                            const uint32_t *__restrict__ tile_hist, uint32_t tiles) {
    __shared__ uint32_t wcnt[kSortWaves][kDigits];  // per wave and digit: count, then first position
    __shared__ uint32_t delta[kDigits];             // staged: global offset minus position in the tile
    __shared__ uint32_t scratch[kSortWaves];
    __shared__ E stage[STAGED ? kSortTile : 1];
    const uint32_t wave = threadIdx.x / kWave, lane = __lane_id();
    const uint32_t tile = blockIdx.x;
    const uint32_t tile_base = tile * kSortTile;
    const uint32_t base = tile_base + wave * kWaveElems + lane;
#pragma unroll
    for (uint32_t w = 0; w < kSortWaves; ++w) wcnt[w][threadIdx.x] = 0;

    E e[kSortItems];
#pragma unroll
    for (uint32_t j = 0; j < kSortItems; ++j) {
        const uint32_t i = base + j * kWave;
        e[j] = i < n ? (E)src[i] : (E)0;
    }
    __syncthreads();

    // rank inside the wave: elements of the same digit in the wave's earlier items (the
    // running count in LDS, one update per distinct digit) plus the lower lanes of this item
    const uint64_t lt = lanemask_lt();
    uint32_t rank[kSortItems];
#pragma unroll
    for (uint32_t j = 0; j < kSortItems; ++j) {
        const bool valid = base + j * kWave < n;
        const uint32_t d = ((key_of(e[j]) - bias) >> shift) & 255u;
        const uint64_t peers = match_digit(d, valid);
        const uint32_t leader = peers ? (uint32_t)__builtin_ctzll(peers) : 0u;
        uint32_t before = 0;
        if (valid && lane == leader) before = atomicAdd(&wcnt[wave][d], popc64(peers));
        before = __shfl(before, (int)leader, kWave);
        rank[j] = before + popc64(peers & lt);
    }
    __syncthreads();

    // thread d: the waves' counts of digit d become their first positions, waves in tile order
    {
        const uint32_t d = threadIdx.x;
        uint32_t c[kSortWaves], tot = 0;
#pragma unroll
        for (uint32_t w = 0; w < kSortWaves; ++w) {
            c[w] = wcnt[w][d];
            tot += c[w];
        }
        uint32_t unused;
        const uint32_t local = block_excl_scan_u32(tot, scratch, &unused);  // digit d's run starts here in the tile
        const uint32_t global = tile_hist[(size_t)d * tiles + tile];
        uint32_t first = STAGED ? local : global;
        if (STAGED) delta[d] = global - local;
#pragma unroll
        for (uint32_t w = 0; w < kSortWaves; ++w) {
            wcnt[w][d] = first;
            first += c[w];
        }
    }
    __syncthreads();

#pragma unroll
    for (uint32_t j = 0; j < kSortItems; ++j) {
        if (base + j * kWave < n) {
            const uint32_t d = ((key_of(e[j]) - bias) >> shift) & 255u;
            const uint32_t pos = wcnt[wave][d] + rank[j];
            if (STAGED)
                stage[pos] = e[j];  // pos < elements of the tile <= kSortTile
            else
                dst[pos] = e[j];  // pos < n: offsets of all tiles and digits partition [0, n)
        }
    }
    if (STAGED) {
        __syncthreads();
        const uint32_t cnt = min(kSortTile, n - tile_base);
        for (uint32_t i = threadIdx.x; i < cnt; i += kSortBlock) {
            const E v = stage[i];
            dst[delta[((key_of(v) - bias) >> shift) & 255u] + i] = v;
        }
    }
}

// ------------------------------------------------------------------------- merge ---

// First index in a[0, n) whose key is not below k / is above k.
template <typename T>
__device__ __forceinline__ uint32_t lower_bound(const T *a, uint32_t lo, uint32_t hi, uint32_t k) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key_of(a[mid]) < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}
template <typename T>
__device__ __forceinline__ uint32_t upper_bound(const T *a, uint32_t lo, uint32_t hi, uint32_t k) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key_of(a[mid]) <= k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Thread c: the merge-path split at diagonal min(c * kMergeTile, nR + nS) of the merged
// sequence in which an R element precedes an S element of the same key, and how many of
// the R elements in front of it carry the key of the first S element behind it.
template <typename ER, typename ES>
__global__ __launch_bounds__(kMergeBlock) void k_smj_partition(const ER *__restrict__ R, uint32_t nR,
                                                               const ES *__restrict__ S, uint32_t nS,
                                                               uint2 *__restrict__ split, uint32_t chunks) {
    const uint32_t c = blockIdx.x * kMergeBlock + threadIdx.x;
    if (c > chunks) return;
    const uint64_t total = (uint64_t)nR + nS;
    const uint64_t diag = min((uint64_t)c * kMergeTile, total);
    uint32_t lo = diag > nS ? (uint32_t)(diag - nS) : 0u;
    uint32_t hi = (uint32_t)min(diag, (uint64_t)nR);
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;  // mid < nR, 0 <= diag - 1 - mid < nS
        if (key_of(R[mid]) <= key_of(S[diag - 1 - mid])) lo = mid + 1; else hi = mid;
    }
    const uint32_t i = lo, j = (uint32_t)(diag - lo);
    uint32_t before = 0;
    if (j < nS && i > 0) before = i - lower_bound(R, 0u, i, key_of(S[j]));
    split[c] = make_uint2(i, before);
}

struct Chunk {
    uint32_t i0, i1, j0, j1, before;
};
__device__ __forceinline__ Chunk chunk_of(const uint2 *split, uint32_t c, uint64_t total) {
    const uint2 a = split[c], b = split[c + 1];
    const uint64_t d0 = (uint64_t)c * kMergeTile, d1 = min(d0 + kMergeTile, total);
    Chunk ch;
    ch.i0 = a.x;
    ch.i1 = b.x;
    ch.j0 = (uint32_t)(d0 - a.x);
    ch.j1 = (uint32_t)(d1 - b.x);
    ch.before = a.y;
    return ch;
}

// Every S element of the chunk contributes the length of its R run: the part inside the
// chunk's R section, and for the chunk's first S key the part in front of the chunk.
template <typename ER, typename ES>
__global__ __launch_bounds__(kMergeBlock) void k_smj_merge_count(const ER *__restrict__ R, uint32_t nR,
                                                                 const ES *__restrict__ S, uint32_t nS,
                                                                 const uint2 *__restrict__ split,
                                                                 uint64_t *__restrict__ result) {
    __shared__ uint32_t rk[kMergeTile];
    __shared__ uint64_t wsum[kMergeBlock / kWave];
    const Chunk ch = chunk_of(split, blockIdx.x, (uint64_t)nR + nS);
    const uint32_t nr = ch.i1 - ch.i0;  // <= kMergeTile
    for (uint32_t t = threadIdx.x; t < nr; t += kMergeBlock) rk[t] = key_of(R[ch.i0 + t]);
    __syncthreads();
    uint64_t m = 0;
    if (ch.j0 < ch.j1) {
        const uint32_t k0 = key_of(S[ch.j0]);
        for (uint32_t j = ch.j0 + threadIdx.x; j < ch.j1; j += kMergeBlock) {
            const uint32_t k = key_of(S[j]);
            const uint32_t lb = lower_bound(rk, 0u, nr, k);
            const uint32_t ub = upper_bound(rk, lb, nr, k);
            m += (uint64_t)(ub - lb) + (k == k0 ? ch.before : 0u);
        }
    }
    m = wave_sum_u64(m);
    if (__lane_id() == 0) wsum[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t tot = 0;
        for (uint32_t w = 0; w < kMergeBlock / kWave; ++w) tot += wsum[w];
        if (tot) __hip_atomic_fetch_add(result + kResMatches, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kMergeBlock) void k_smj_merge_emit(const uint64_t *__restrict__ R, uint32_t nR,
                                                                const uint64_t *__restrict__ S, uint32_t nS,
                                                                const uint2 *__restrict__ split,
                                                                uint64_t *__restrict__ result,
                                                                output_triple_t *__restrict__ out, uint64_t cap) {
    __shared__ uint64_t rt[kMergeTile];
    const Chunk ch = chunk_of(split, blockIdx.x, (uint64_t)nR + nS);
    const uint32_t nr = ch.i1 - ch.i0;
    for (uint32_t t = threadIdx.x; t < nr; t += kMergeBlock) rt[t] = R[ch.i0 + t];
    __syncthreads();
    if (ch.j0 >= ch.j1) return;
    const uint32_t k0 = key_of(S[ch.j0]);
    // the bound is the same for every thread: whole waves take their output range together
    for (uint32_t jb = ch.j0; jb < ch.j1; jb += kMergeBlock) {
        const uint32_t j = jb + threadIdx.x;
        const bool valid = j < ch.j1;
        const uint64_t s = valid ? S[j] : 0ull;
        const uint32_t k = key_of(s);
        uint32_t lb = 0, ub = 0, front = 0;
        if (valid) {
            lb = lower_bound(rt, 0u, nr, k);
            ub = upper_bound(rt, lb, nr, k);
            front = k == k0 ? ch.before : 0u;
        }
        const uint64_t cnt = (uint64_t)(ub - lb) + front;
        const uint64_t incl = wave_incl_scan_u64(cnt);
        const uint64_t total = __shfl(incl, kWave - 1, kWave);
        if (total == 0) continue;  // wave-uniform
        uint64_t base = 0;
        if (__lane_id() == 0)
            base = __hip_atomic_fetch_add(result + kResOut, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        base = __shfl(base, 0, kWave);
        uint64_t pos = base + incl - cnt;
        const uint32_t spay = (uint32_t)(s >> 32);
        for (uint32_t x = ch.i0 - front; x < ch.i0; ++x, ++pos)  // the run's part in front of the chunk
            if (pos < cap) out[pos] = output_triple_t{k, (uint32_t)(R[x] >> 32), spay};
        for (uint32_t x = lb; x < ub; ++x, ++pos)
            if (pos < cap) out[pos] = output_triple_t{k, (uint32_t)(rt[x] >> 32), spay};
    }
}

}  // namespace

static dim3 stream_grid(uint64_t n) {
    const uint64_t g = (n + kSortTile - 1) / kSortTile;
    return dim3((uint32_t)(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g));
}

hipError_t launch_min(const row_t *in, uint64_t n, uint32_t *inv_min, hipStream_t s) {
    hipLaunchKernelGGL(k_smj_min, stream_grid(n), dim3(kSortBlock), 0, s, reinterpret_cast<const uint64_t *>(in), n,
                       inv_min);
    return hipGetLastError();
}

hipError_t launch_digits(const row_t *in, uint64_t n, uint32_t *ghist, const uint32_t *inv_min, hipStream_t s) {
    hipLaunchKernelGGL(k_smj_digits, stream_grid(n), dim3(kSortBlock), 0, s, reinterpret_cast<const uint64_t *>(in), n,
                       ghist, inv_min);
    return hipGetLastError();
}

hipError_t launch_tile_hist(const void *src, int src_bytes, uint64_t n, uint32_t bias, uint32_t shift,
                            uint32_t *tile_hist, hipStream_t s) {
    const uint32_t tiles = tiles_of(n);
    const dim3 grid(tiles), block(kSortBlock);
    if (src_bytes == 8)
        hipLaunchKernelGGL(k_smj_tile_hist<uint64_t>, grid, block, 0, s, static_cast<const uint64_t *>(src), (uint32_t)n,
                           bias, shift, tile_hist, tiles);
    else
        hipLaunchKernelGGL(k_smj_tile_hist<uint32_t>, grid, block, 0, s, static_cast<const uint32_t *>(src), (uint32_t)n,
                           bias, shift, tile_hist, tiles);
    return hipGetLastError();
}

hipError_t launch_scan(uint32_t *tile_hist, uint64_t n, const uint32_t *ghist_pass, hipStream_t s) {
    hipLaunchKernelGGL(k_smj_scan, dim3(kDigits), dim3(kSortBlock), 0, s, tile_hist, tiles_of(n), ghist_pass);
    return hipGetLastError();
}

template <typename In, typename E>
static void scatter(const void *src, void *dst, uint64_t n, uint32_t bias, uint32_t shift, const uint32_t *tile_hist,
                    bool staged, hipStream_t s) {
    const uint32_t tiles = tiles_of(n);
    const dim3 grid(tiles), block(kSortBlock);
    if (staged)
        hipLaunchKernelGGL((k_smj_scatter<In, E, true>), grid, block, 0, s, static_cast<const In *>(src), (uint32_t)n,
                           static_cast<E *>(dst), bias, shift, tile_hist, tiles);
    else
        hipLaunchKernelGGL((k_smj_scatter<In, E, false>), grid, block, 0, s, static_cast<const In *>(src), (uint32_t)n,
                           static_cast<E *>(dst), bias, shift, tile_hist, tiles);
}

hipError_t launch_scatter(const void *src, int src_bytes, void *dst, int dst_bytes, uint64_t n, uint32_t bias,
                          uint32_t shift, const uint32_t *tile_hist, bool staged, hipStream_t s) {
    if (src_bytes == 8 && dst_bytes == 8)
        scatter<uint64_t, uint64_t>(src, dst, n, bias, shift, tile_hist, staged, s);
    else if (src_bytes == 8 && dst_bytes == 4)
        scatter<uint64_t, uint32_t>(src, dst, n, bias, shift, tile_hist, staged, s);
    else if (src_bytes == 4 && dst_bytes == 4)
        scatter<uint32_t, uint32_t>(src, dst, n, bias, shift, tile_hist, staged, s);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

template <typename ER, typename ES>
static void partition(const void *R, uint64_t nR, const void *S, uint64_t nS, uint2 *split, hipStream_t s) {
    const uint32_t chunks = chunks_of(nR + nS);
    hipLaunchKernelGGL((k_smj_partition<ER, ES>), dim3(chunks / kMergeBlock + 1), dim3(kMergeBlock), 0, s,
                       static_cast<const ER *>(R), (uint32_t)nR, static_cast<const ES *>(S), (uint32_t)nS, split, chunks);
}

hipError_t launch_partition(const void *R, int r_bytes, uint64_t nR, const void *S, int s_bytes, uint64_t nS,
                            uint2 *split, hipStream_t s) {
    if (r_bytes == 8 && s_bytes == 8) partition<uint64_t, uint64_t>(R, nR, S, nS, split, s);
    else if (r_bytes == 8) partition<uint64_t, uint32_t>(R, nR, S, nS, split, s);
    else if (s_bytes == 8) partition<uint32_t, uint64_t>(R, nR, S, nS, split, s);
    else partition<uint32_t, uint32_t>(R, nR, S, nS, split, s);
    return hipGetLastError();
}

template <typename ER, typename ES>
static void merge_count(const void *R, uint64_t nR, const void *S, uint64_t nS, const uint2 *split, uint64_t *result,
                        hipStream_t s) {
    hipLaunchKernelGGL((k_smj_merge_count<ER, ES>), dim3(chunks_of(nR + nS)), dim3(kMergeBlock), 0, s,
                       static_cast<const ER *>(R), (uint32_t)nR, static_cast<const ES *>(S), (uint32_t)nS, split, result);
}

hipError_t launch_merge_count(const void *R, int r_bytes, uint64_t nR, const void *S, int s_bytes, uint64_t nS,
                              const uint2 *split, uint64_t *result, hipStream_t s) {
    if (r_bytes == 8 && s_bytes == 8) merge_count<uint64_t, uint64_t>(R, nR, S, nS, split, result, s);
    else if (r_bytes == 8) merge_count<uint64_t, uint32_t>(R, nR, S, nS, split, result, s);
    else if (s_bytes == 8) merge_count<uint32_t, uint64_t>(R, nR, S, nS, split, result, s);
    else merge_count<uint32_t, uint32_t>(R, nR, S, nS, split, result, s);
    return hipGetLastError();
}

hipError_t launch_merge_emit(const uint64_t *R, uint64_t nR, const uint64_t *S, uint64_t nS, const uint2 *split,
                             uint64_t *result, output_triple_t *out, uint64_t cap, hipStream_t s) {
    hipLaunchKernelGGL(k_smj_merge_emit, dim3(chunks_of(nR + nS)), dim3(kMergeBlock), 0, s, R, (uint32_t)nR, S,
                       (uint32_t)nS, split, result, out, cap);
    return hipGetLastError();
}

}  // namespace smj
}  // namespace sgxamd
