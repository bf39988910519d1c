// C++-linkage drop-ins RHO() and run_join() (declared in sgxamd/joins.hpp).
//
// RHO / RHT: radix_join.cpp:1640-1648 -> mi355_rho_join / mi355_rht_join, plus the reference's
//      print_timing log lines (radix_join.cpp:252-293) so that
//      SGXv2Scripts/scripts/helpers/runner.py:14-55 parses our output unchanged.
// PHT / PHT_no_overflow / PHT_unrolled / PHT_overflow: no_partitioning_hash_join.cpp:166-249 ->
//      mi355_npo_join, plus the npj print_timing lines (HashLinkTableCommon.cpp:13-29).
// MWAY / PSM / RSM: sortmergejoin_multiway.cpp, parallel_sortmerge_join.cpp,
//      radix_sortmerge_join.cpp -> mi355_smj_join, plus their print_timing lines.
// run_join: joins.cpp:55-78 (strcmp lookup in an algorithm table, memcpy of the
//      result; like the reference, the callee's result_t is not freed).
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sgxamd/joins.hpp"
#include "sgxamd/multi.h"
#include "sgxamd/rho.h"

namespace {

const auto g_log_start = std::chrono::steady_clock::now();

// Logger.cpp:53-76 format: "<color>[%8.4f][%5s] msg<reset>\n"
void logger(const char *level, const char *color, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - g_log_start).count();
    std::printf("%s[%8.4f][%5s] %s\x1b[0m\n", color, t, level, buf);
}

#define LOG_INFO(...) logger("INFO", "\x1b[32m", __VA_ARGS__)
#define LOG_ERROR(...) logger("ERROR", "\x1b[31m", __VA_ARGS__)

uint64_t cpms() {  // CYCLES_PER_MICROSECOND of the reference build (J/CMakeLists.txt:17)
    const char *e = std::getenv("SGXAMD_CPMS");
    return e ? std::strtoull(e, nullptr, 10) : 2900ull;
}

// GPUs for RHO(): SGXAMD_GPUS (joinconfig_t has no spare field); > 1 runs
// the radix-shard exchange of sgxamd/multi.h (counting joins).
int gpus_from_env() {
    const char *e = std::getenv("SGXAMD_GPUS");
    return e ? std::max(1, std::atoi(e)) : 1;
}

int rho_entry(const table_t *relR, const table_t *relS, const joinconfig_t *config, result_t *out) {
    const int g = gpus_from_env();
    if (g > 1 && !(config && config->MATERIALIZE)) return mi355_rho_join_multi(relR, relS, config, g, out);
    return mi355_rho_join(relR, relS, config, out);
}

// NPO_st / NPO_no have no C++ symbol (sgxamd/joins.hpp): their table entries call this
result_t *npo_by_name(const table_t *relR, const table_t *relS, const joinconfig_t *config);

const algorithm_t mi355_algorithms[] = {  // joins.cpp:33-53, the joins this library replaces
    {"RHO", RHO},
    {"RHT", RHT},
    // the no-partitioning family (joins.cpp:34-39): one GPU join behind every name
    {"PHT", PHT},
    {"PHT_no", PHT_no_overflow},
    {"PHT_un", PHT_unrolled},
    {"PHT_o", PHT_overflow},
    {"NPO_st", npo_by_name},
    {"NPO_no", npo_by_name},
    // the sort-merge family (joins.cpp:44-47): one GPU join behind every name
    {"PSM", PSM},
    {"RSM", RSM},
    {"MWAY", MWAY},
    {"", nullptr},
};

result_t *radix_dropin(const char *name, const table_t *relR, const table_t *relS, const joinconfig_t *config,
                       int (*join)(const table_t *, const table_t *, const joinconfig_t *, result_t *)) {
    LOG_INFO("Running %s on MI355X (%s)", name, mi355_version());
    const auto t_start = std::chrono::steady_clock::now();
    auto *res = static_cast<result_t *>(std::malloc(sizeof(result_t)));
    const int rc = join(relR, relS, config, res);
    const auto t_end = std::chrono::steady_clock::now();
    if (rc != MI355_OK) {
        LOG_ERROR("%s failed (%d): %s", name, rc, mi355_last_error());
        std::exit(EXIT_FAILURE);
    }
    mi355_rho_stats st{};
    mi355_last_join_stats(&st);
    const uint64_t num = relR->num_tuples + relS->num_tuples;
    const double us = st.ms_total * 1000.0;
    const double wall_us = std::chrono::duration<double, std::micro>(t_end - t_start).count();

    // print_timing (radix_join.cpp:252-293): every phase line the reference logs, in its
    // order and format, so that SGXv2Scripts/scripts/helpers/runner.py:14-55 parses them.
    // Device times (HIP events) are converted to cycles at the reference build's CPMS.
    const uint64_t C = cpms();
    auto cyc = [&](double ms) { return static_cast<unsigned long>(ms * 1000.0 * C); };
    const double n = num ? (double)num : 1.0;
    if (join == rho_entry && gpus_from_env() > 1 && !(config && config->MATERIALIZE)) {
        mi355_multi_stats ms{};
        mi355_last_multi_stats(&ms);
        LOG_INFO("Radix-shard exchange over %d GPUs (%s, %d pieces per relation): received R %lu..%lu, "
                 "S %lu..%lu tuples per GPU, %lu bytes over the links; phase lines below: GPU 0's local join",
                 ms.world, ms.transport == MI355_TRANSPORT_RCCL ? "RCCL" : "one-GPU rehearsal", ms.pieces,
                 (unsigned long)ms.recv_r_min, (unsigned long)ms.recv_r_max, (unsigned long)ms.recv_s_min,
                 (unsigned long)ms.recv_s_max, (unsigned long)ms.sent_bytes);
    }
    LOG_INFO("Running %s with %u passes and %u radix bits", name, st.passes, st.radix_bits);
    LOG_INFO("Total input tuples : %u", (unsigned)num);
    LOG_INFO("Result tuples : %lu", (unsigned long)st.matches);
    LOG_INFO("Total Join Time (cycles)    : %lu", cyc(st.ms_total));
    LOG_INFO("Partition Overall (cycles)  : %lu", cyc(st.ms_partition));
    LOG_INFO("Partition Pass One (cycles) : %lu", cyc(st.ms_pass1));
    LOG_INFO("Partition R        (cycles) : %lu", cyc(st.ms_pass1_r));
    LOG_INFO("Partition S        (cycles) : %lu", cyc(st.ms_pass1_s));
    LOG_INFO("Partition One Hist (cycles) : %lu", cyc(st.ms_pass1_hist));
    LOG_INFO("Partition One Copy (cycles) : %lu", cyc(st.ms_pass1_copy));
    LOG_INFO("Partition Pass Two (cycles) : %lu", cyc(st.ms_pass2));
    LOG_INFO("Partition Two Hist (cycles) : %lu", cyc(st.ms_pass2_hist));
    LOG_INFO("Partition Two Copy (cycles) : %lu", cyc(st.ms_pass2_copy));
    LOG_INFO("Build+Join Overall (cycles) : %lu", cyc(st.ms_join));
    LOG_INFO("Build (cycles)              : %lu", cyc(st.ms_build));
    LOG_INFO("Join (cycles)               : %lu", cyc(st.ms_probe));
    LOG_INFO("Cycles-per-tuple            : %.4lf", cyc(st.ms_total) / n);
    LOG_INFO("Cycles-per-tuple-partition  : %.4lf", cyc(st.ms_partition) / n);
    LOG_INFO("Cycles-per-tuple-partitioning_pass_1_timer     : %.4lf", cyc(st.ms_pass1) / n);
    LOG_INFO("Cycles-per-tuple-partitioning_pass_2_timer     : %.4lf", cyc(st.ms_pass2) / n);
    LOG_INFO("Cycles-per-tuple-join      : %.4lf", cyc(st.ms_join) / n);
    LOG_INFO("Pure Join Runtime (us) : %lu ", (unsigned long)us);
    LOG_INFO("Preparation Time (us) : %lu ", (unsigned long)(st.ms_h2d * 1000.0));
    LOG_INFO("Join time arg + join time (us) : %lu ", (unsigned long)(wall_us - st.ms_h2d * 1000.0));
    LOG_INFO("Free time (us) : %lu ", 0ul);
    LOG_INFO("Throughput (M rec/sec) : %.2lf", res->throughput);
    LOG_INFO("Total Runtime (us)     : %lu ", (unsigned long)wall_us);
    return res;
}

// PHT and its variants: mi355_npo_join, then the npj print_timing lines
// (HashLinkTableCommon.cpp:13-29) in the reference's order and format.
result_t *npo_dropin(const char *name, const table_t *relR, const table_t *relS, const joinconfig_t *config) {
    LOG_INFO("Running %s on MI355X (%s)", name, mi355_version());
    const auto t_start = std::chrono::steady_clock::now();
    auto *res = static_cast<result_t *>(std::malloc(sizeof(result_t)));
    const int rc = mi355_npo_join(relR, relS, config, res);
    const auto t_end = std::chrono::steady_clock::now();
    if (rc != MI355_OK) {
        LOG_ERROR("%s failed (%d): %s", name, rc, mi355_last_error());
        std::exit(EXIT_FAILURE);
    }
    mi355_npo_stats st{};
    mi355_last_npo_stats(&st);
    const uint64_t num = relR->num_tuples + relS->num_tuples;
    const double wall_us = std::chrono::duration<double, std::micro>(t_end - t_start).count();
    const uint64_t C = cpms();
    auto cyc = [&](double ms) { return static_cast<unsigned long>(ms * 1000.0 * C); };
    const unsigned long total = cyc(st.ms_total);
    const unsigned long usec_tsc = total / C;
    LOG_INFO("Hash table: %lu buckets, %lu overflow nodes, %lu bytes; clear (cycles) %lu, inside the total",
             (unsigned long)st.num_buckets, (unsigned long)st.overflow_nodes, (unsigned long)st.table_bytes,
             cyc(st.ms_clear));
    LOG_INFO("Total input tuples : %lu", (unsigned long)num);
    LOG_INFO("Result tuples : %lu", (unsigned long)st.matches);
    LOG_INFO("Total Join Time (cycles)    : %lu", total);
    LOG_INFO("Build (cycles)              : %lu", cyc(st.ms_build));
    LOG_INFO("Join (cycles)               : %lu", cyc(st.ms_probe));
    LOG_INFO("Cycles-per-tuple : %.4lf", (double)total / (num ? (double)num : 1.0));
    LOG_INFO("Total Runtime (us) : %lu ", (unsigned long)wall_us);
    LOG_INFO("Total RT from TSC (us) : %lu ", usec_tsc);
    LOG_INFO("Throughput (M rec/sec) : %.2lf", usec_tsc ? (double)num / (double)usec_tsc : 0.0);
    return res;
}

result_t *npo_by_name(const table_t *relR, const table_t *relS, const joinconfig_t *config) {
    return npo_dropin("NPO", relR, relS, config);
}

// MWAY, PSM and RSM: mi355_smj_join, then the reference's phase lines.  psm_form: the
// lines of PSM's print_timing (parallel_sortmerge_join.cpp:27-37); otherwise the
// 11-argument print_timing MWAY and RSM call (radix_join.cpp:199-215).  Both sorts are the
// partition phase, the merge is the join phase; the in-depth values are 0.
result_t *smj_dropin(const char *name, bool psm_form, const table_t *relR, const table_t *relS,
                     const joinconfig_t *config) {
    LOG_INFO("Running %s on MI355X (%s)", name, mi355_version());
    const auto t_start = std::chrono::steady_clock::now();
    auto *res = static_cast<result_t *>(std::malloc(sizeof(result_t)));
    const int rc = mi355_smj_join(relR, relS, config, res);
    const auto t_end = std::chrono::steady_clock::now();
    if (rc != MI355_OK) {
        LOG_ERROR("%s failed (%d): %s", name, rc, mi355_last_error());
        std::exit(EXIT_FAILURE);
    }
    mi355_smj_stats st{};
    mi355_last_smj_stats(&st);
    const uint64_t num = relR->num_tuples + relS->num_tuples;
    const double wall_us = std::chrono::duration<double, std::micro>(t_end - t_start).count();
    const uint64_t C = cpms();
    auto cyc = [&](double ms) { return static_cast<unsigned long>(ms * 1000.0 * C); };
    const double n = num ? (double)num : 1.0;
    const unsigned long total = cyc(st.ms_total), partition = cyc(st.ms_sort_r + st.ms_sort_s), join = cyc(st.ms_merge);
    const unsigned long usec_tsc = total / C;
    const double throughput = usec_tsc ? (double)num / (double)usec_tsc : 0.0;
    LOG_INFO("Sort-merge join: %u + %u radix-sort passes over %u-byte elements (R sort %lu, S sort %lu cycles)",
             st.sort_passes_r, st.sort_passes_s, st.elem_bytes, cyc(st.ms_sort_r), cyc(st.ms_sort_s));
    LOG_INFO("Total input tuples : %u", (unsigned)num);
    LOG_INFO("Result tuples : %lu", (unsigned long)st.matches);
    LOG_INFO("Total Join Time (cycles)    : %lu", total);
    LOG_INFO("Partition Overall (cycles)  : %lu", partition);
    if (!psm_form) {
        LOG_INFO("Partition Pass One (cycles) : %lu", 0ul);
        LOG_INFO("Partition Pass Two (cycles) : %lu", 0ul);
    }
    LOG_INFO("Build+Join Overall (cycles) : %lu", join);
    if (!psm_form) {
        LOG_INFO("Build (cycles)              : %lu", 0ul);
        LOG_INFO("Join (cycles)               : %lu", 0ul);
    }
    LOG_INFO("Cycles-per-tuple            : %.4lf", (double)total / n);
    LOG_INFO("Cycles-per-tuple-partition  : %.4lf", (double)partition / n);
    if (!psm_form) {
        LOG_INFO("Cycles-per-tuple-partitioning_pass_1_timer     : %.4lf", 0.0);
        LOG_INFO("Cycles-per-tuple-partitioning_pass_2_timer     : %.4lf", 0.0);
    }
    LOG_INFO("Cycles-per-tuple-join      : %.4lf", (double)join / n);
    if (psm_form) {
        LOG_INFO("Total Runtime (us) : %lu ", (unsigned long)wall_us);
        LOG_INFO("Total RT from TSC (us) : %lu ", usec_tsc);
        LOG_INFO("Throughput (M rec/sec) : %.2lf", throughput);
    } else {
        LOG_INFO("Pure Join Runtime (us) : %lu ", usec_tsc);
        LOG_INFO("Throughput (M rec/sec) : %.2lf", throughput);
        LOG_INFO("Total Runtime (us)     : %lu ", (unsigned long)wall_us);
    }
    return res;
}

}  // namespace

result_t *PHT(const table_t *relR, const table_t *relS, const joinconfig_t *config) {
    return npo_dropin("PHT", relR, relS, config);
}

result_t *PHT_no_overflow(const table_t *relR, const table_t *relS, const joinconfig_t *config) {
    return npo_dropin("PHT_no_overflow", relR, relS, config);
}

result_t *PHT_unrolled(const table_t *relR, const table_t *relS, const joinconfig_t *config) {
    return npo_dropin("PHT_unrolled", relR, relS, config);
}

result_t *PHT_overflow(const table_t *relR, const table_t *relS, const joinconfig_t *config) {
    return npo_dropin("PHT_overflow", relR, relS, config);
}

result_t *MWAY(const table_t *relR, const table_t *relS, const joinconfig_t *config) {
    return smj_dropin("MWAY", false, relR, relS, config);
}

result_t *PSM(const table_t *relR, const table_t *relS, const joinconfig_t *config) {
    return smj_dropin("PSM", true, relR, relS, config);
}

result_t *RSM(const table_t *relR, const table_t *relS, const joinconfig_t *config) {
    return smj_dropin("RSM", false, relR, relS, config);
}

result_t *RHO(const table_t *relR, const table_t *relS, const joinconfig_t *config) {
    return radix_dropin("RHO", relR, relS, config, rho_entry);
}

result_t *RHT(const table_t *relR, const table_t *relS, const joinconfig_t *config) {
    return radix_dropin("RHT", relR, relS, config, mi355_rht_join);
}

void run_join(result_t *res, const table_t *relR, const table_t *relS, const char *algorithm_name,
              const joinconfig_t *config) {
    const algorithm_t *alg = nullptr;
    for (int i = 0; mi355_algorithms[i].join; ++i) {
        if (std::strcmp(algorithm_name, mi355_algorithms[i].name) == 0) {
            alg = &mi355_algorithms[i];
            break;
        }
    }
    if (!alg) {
        LOG_ERROR("Algorithm not found: %s", algorithm_name);
        std::exit(EXIT_FAILURE);
    }
    result_t *tmp = alg->join(relR, relS, config);
    if (tmp) std::memcpy(res, tmp, sizeof(result_t));
}
