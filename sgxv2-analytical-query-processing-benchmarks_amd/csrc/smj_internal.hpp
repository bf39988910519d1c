// Sort-merge join (the reference's MWAY / PSM / RSM): the geometry of the device-wide
// radix sort and of the merge, the workspace layout and the launch functions
// smj_kernels.hip gives smj_host.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sgxamd/data_types.h"

namespace sgxamd {
namespace smj {

// Sort: stable LSD radix sort, 8-bit digits.  One workgroup of kSortBlock threads owns one
// tile of kSortTile consecutive elements; wave w of the workgroup owns elements
// [w * 64 * kSortItems, (w + 1) * 64 * kSortItems) of the tile and item j of lane l is
// element j * 64 + l of the wave's part, so (wave, item, lane) is the input order.
constexpr uint32_t kSortBlock = 256;
constexpr uint32_t kSortItems = 16;
constexpr uint32_t kSortTile = kSortBlock * kSortItems;  // 4096
constexpr uint32_t kDigits = 256;
constexpr uint32_t kPasses = 4;

// Merge: the merged sequence of R and S (R first on ties) is cut into chunks of
// kMergeTile elements, one workgroup each.
constexpr uint32_t kMergeBlock = 256;
constexpr uint32_t kMergeTile = 4096;

// The control buffer (Context::smj_ctrl): the four 256-bin digit histograms of R, those
// of S, the complements of the two smallest keys, the result words, then the per-tile
// histogram of the pass that is running (bin-major: counter [digit][tile]).  Everything in
// front of the per-tile histogram is cleared at the start of a call.
constexpr size_t kGhistWords = kPasses * kDigits;             // per relation
constexpr size_t kOffGhistR = 0;                              // bytes
constexpr size_t kOffGhistS = kGhistWords * sizeof(uint32_t);
constexpr size_t kOffMin = 2 * kGhistWords * sizeof(uint32_t);  // u32 words: ~min key of R, of S
constexpr size_t kOffResult = kOffMin + 64;                     // u64 words: matches, out cursor
constexpr size_t kOffTileHist = kOffResult + 192;
constexpr size_t kPlanWords = 2 * kGhistWords + 2;              // what the host reads to plan the passes
constexpr uint32_t kResMatches = 0;
constexpr uint32_t kResOut = 1;

inline uint32_t tiles_of(uint64_t n) { return (uint32_t)((n + kSortTile - 1) / kSortTile); }
inline uint32_t chunks_of(uint64_t total) { return (uint32_t)((total + kMergeTile - 1) / kMergeTile); }

// Elements are 8 bytes (a tuple, key in the low word) or 4 bytes (a key); *_bytes says which.

// The sort orders by key - bias, bias = the relation's smallest key: *inv_min (zeroed before)
// receives its complement.
hipError_t launch_min(const row_t *in, uint64_t n, uint32_t *inv_min, hipStream_t s);
// All four digit histograms of key - bias over the n tuples at in, added to ghist[4][256]
// (zeroed before).
hipError_t launch_digits(const row_t *in, uint64_t n, uint32_t *ghist, const uint32_t *inv_min, hipStream_t s);
// One pass over digit ((key - bias) >> shift) & 255: per-tile histogram, exclusive scan (ghist_pass:
// the relation's 256-bin histogram of this digit), stable scatter.  src_bytes = 8 with
// dst_bytes = 4 extracts the key on the way.  staged: the tile leaves through LDS, each
// digit's run as consecutive addresses; otherwise every lane stores its elements directly.
hipError_t launch_tile_hist(const void *src, int src_bytes, uint64_t n, uint32_t bias, uint32_t shift,
                            uint32_t *tile_hist, hipStream_t s);
hipError_t launch_scan(uint32_t *tile_hist, uint64_t n, const uint32_t *ghist_pass, hipStream_t s);
hipError_t launch_scatter(const void *src, int src_bytes, void *dst, int dst_bytes, uint64_t n, uint32_t bias,
                          uint32_t shift, const uint32_t *tile_hist, bool staged, hipStream_t s);

// Merge over two ascending relations.  split[c] = {R elements in front of chunk c, R elements
// in front of chunk c that equal the chunk's first S key}, c = 0 .. chunks.
hipError_t launch_partition(const void *R, int r_bytes, uint64_t nR, const void *S, int s_bytes, uint64_t nS,
                            uint2 *split, hipStream_t s);
hipError_t launch_merge_count(const void *R, int r_bytes, uint64_t nR, const void *S, int s_bytes, uint64_t nS,
                              const uint2 *split, uint64_t *result, hipStream_t s);
// Tuples on both sides.  Writes every match to out[0, cap) through the cursor
// result[kResOut] (never past cap).
hipError_t launch_merge_emit(const uint64_t *R, uint64_t nR, const uint64_t *S, uint64_t nS, const uint2 *split,
                             uint64_t *result, output_triple_t *out, uint64_t cap, hipStream_t s);

}  // namespace smj
}  // namespace sgxamd
