// No-partitioning hash join (the reference's PHT family): the table layout and the
// launch functions npo_kernels.hip gives npo_host.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sgxamd/data_types.h"

namespace sgxamd {
namespace npo {

// One global hash table over all of R (HashLinkTableCommon.cpp:31-47, BUCKET_SIZE 2):
//   bucket b = key & mask, 16 bytes {count, next, key0, key1}: a probe of a primary-key
//   R is one dwordx4 load.  count = tuples hashed here (slots in use = min(count, 2));
//   next = 1 + index of the first overflow node, 0 = none (so that clearing the table
//   is one memset and key 0 is an ordinary key: occupancy comes from count alone).
//   The R payloads of the two slots live in bpay[2 b + slot] (materialising joins
//   only), so a counting probe touches 16 bytes per key.
//   node i = 8 bytes {key, next}, its payload in npay[i]; nodes are pushed at the
//   bucket's head.
// The table buffer starts with kCtrlBytes of control words, cleared with the buckets.
constexpr uint32_t kBucketCap = 2;
constexpr size_t kCtrlBytes = 256;
constexpr uint32_t kCtrlCursor = 0;   // u32 word: overflow nodes the build asked for
constexpr uint32_t kCtrlMatches = 1;  // u64 word: the probe's match count
constexpr uint32_t kCtrlOut = 2;      // u64 word: the materialising probe's output cursor

struct Table {
    uint4 *buckets;
    uint32_t *bpay;     // null for counting joins
    uint2 *nodes;       // null while no join overflowed a bucket
    uint32_t *npay;
    uint32_t *ctrl;     // kCtrlBytes in front of buckets
    uint32_t mask;      // num_buckets - 1
    uint32_t pool_cap;  // nodes that fit; a build that needs more only counts them
};

inline uint64_t next_pow2(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

// write_through: the slot and node stores are agent-scope relaxed atomic stores (sc1)
// instead of plain stores (DESIGN.md §3 "No-partitioning join", build visibility).
hipError_t launch_build(const row_t *R, uint64_t n, const Table &t, bool write_through, hipStream_t s);
// Counts every match into ctrl[kCtrlMatches]; keys_in_flight: 4, 8 or 16 bucket loads
// issued per thread before the first is consumed.
hipError_t launch_probe(const row_t *S, uint64_t n, const Table &t, int keys_in_flight, hipStream_t s);
// Writes every match to out[0, cap) through the cursor ctrl[kCtrlOut] (never past cap).
hipError_t launch_probe_materialize(const row_t *S, uint64_t n, const Table &t, output_triple_t *out, uint64_t cap,
                                    hipStream_t s);

}  // namespace npo
}  // namespace sgxamd
