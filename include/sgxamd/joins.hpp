// sgxamd/joins.hpp — C++-linkage drop-ins for the reference's join entry points.
//
// Same declarations (and therefore the same mangled symbols) as the reference:
//   result_t *RHO(const table_t*, const table_t*, const joinconfig_t*)
//       Join-Benchmarks/lib/Joins/include/radix/radix_join.h:29-30   (_Z3RHOPK7table_tS1_PK12joinconfig_t)
//   result_t *RHT(const table_t*, const table_t*, const joinconfig_t*)
//       radix_join.h (RHT, implemented at radix_join.cpp:1645-1648)    (_Z3RHTPK7table_tS1_PK12joinconfig_t)
//   void run_join(result_t*, const table_t*, const table_t*, const char*, const joinconfig_t*)
//       Join-Benchmarks/lib/Joins/include/joins.hpp / src/joins.cpp:55-78
//   result_t *PHT / PHT_no_overflow / PHT_unrolled / PHT_overflow(const table_t*, const table_t*, const joinconfig_t*)
//       Join-Benchmarks/lib/Joins/include/npj/no_partitioning_hash_join.hpp:6-16
//       (_Z3PHTPK7table_tS1_PK12joinconfig_t, _Z15PHT_no_overflowPK7table_tS1_PK12joinconfig_t,
//        _Z12PHT_unrolledPK7table_tS1_PK12joinconfig_t, _Z12PHT_overflowPK7table_tS1_PK12joinconfig_t)
//       All four run the one no-partitioning GPU join (mi355_npo_join): the count is exact
//       for any input, also where the reference's no-overflow variants write past a full
//       bucket.  They print the npj print_timing lines (HashLinkTableCommon.cpp:13-29).
//       run_join also knows the table names NPO_st and NPO_no (joins.cpp:38-39), but no
//       C++ symbol is exported for them: the reference's header declares NPO_st / NPO_no
//       while its table names NPO_single_thread / NPO_no_overflow, so no consistent
//       symbol exists to match.
//   result_t *MWAY / PSM / RSM(const table_t*, const table_t*, const joinconfig_t*)
//       mway/sortmergejoin_multiway.h:40-41, psm/parallel_sortmerge_join.h:16,
//       radix/radix_sortmerge_join.hpp:4
//       (_Z4MWAYPK7table_tS1_PK12joinconfig_t, _Z3PSMPK7table_tS1_PK12joinconfig_t,
//        _Z3RSMPK7table_tS1_PK12joinconfig_t)
//       All three run the one GPU sort-merge join (mi355_smj_join); relR->sorted / relS->sorted
//       skip that relation's sort.  PSM prints the lines of its own print_timing
//       (parallel_sortmerge_join.cpp:27-37), MWAY and RSM the 11-argument form
//       (radix_join.cpp:199-215): the sorts under "Partition Overall", the merge under
//       "Build+Join Overall", the pass, build and join in-depth values 0.
// so an unmodified run_join-style caller (App/TEEBench/native.cpp:137, the TPC-H
// queries) links against libsgxamd.so instead of the CPU join library.
// With config->MATERIALIZE = 1 the result carries the reference's chunked_table_t
// (result_type 1; release with mi355_free_chunked_table).
// RHO() / RHT() run the join on the current MI355X, prints the reference's timing log
// lines (radix_join.cpp:252-293) and exits on error like the reference
// (ocall_exit(EXIT_FAILURE)); the returned result_t is malloc'd by the callee.
#pragma once

#include "sgxamd/data_types.h"

result_t *RHO(const table_t *relR, const table_t *relS, const joinconfig_t *config);
result_t *RHT(const table_t *relR, const table_t *relS, const joinconfig_t *config);
result_t *PHT(const table_t *relR, const table_t *relS, const joinconfig_t *config);
result_t *PHT_no_overflow(const table_t *relR, const table_t *relS, const joinconfig_t *config);
result_t *PHT_unrolled(const table_t *relR, const table_t *relS, const joinconfig_t *config);
result_t *PHT_overflow(const table_t *relR, const table_t *relS, const joinconfig_t *config);
result_t *MWAY(const table_t *relR, const table_t *relS, const joinconfig_t *config);
result_t *PSM(const table_t *relR, const table_t *relS, const joinconfig_t *config);
result_t *RSM(const table_t *relR, const table_t *relS, const joinconfig_t *config);

void run_join(result_t *res, const table_t *relR, const table_t *relS, const char *algorithm_name,
              const joinconfig_t *config);
