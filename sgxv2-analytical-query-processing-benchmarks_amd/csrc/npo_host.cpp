// No-partitioning hash join (PHT family), host side: table and node-pool workspace,
// the clear / build / probe launches on the join's stream and the C-ABI of
// sgxamd/rho.h (mi355_npo_*).  Kernels: npo_kernels.hip; layout: npo_internal.hpp.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "common.hpp"
#include "npo_internal.hpp"
#include "rho_device.hpp"
#include "runtime.hpp"
#include "sgxamd/rho.h"

using namespace sgxamd;

namespace {

thread_local mi355_npo_stats g_last_npo{};

constexpr int kProbeKeys = 8;  // bucket loads in flight per thread (SGXAMD_NPO_KEYS)

// SGXAMD_NPO_PLAIN=1: plain slot and node stores instead of the write-through ones
// (development A/B switch, read at every call so that one process can alternate the two
// forms; DESIGN.md §3 "No-partitioning join").
bool write_through_enabled() {
    const char *e = std::getenv("SGXAMD_NPO_PLAIN");
    return !(e && std::atoi(e) == 1);
}

// SGXAMD_NPO_KEYS=4 / 8 / 16: the other arms of the probe-depth A/B (profiles/npo_ab.log),
// read at every call like the above.
int probe_keys_in_flight() {
    const char *e = std::getenv("SGXAMD_NPO_KEYS");
    const int k = e ? std::atoi(e) : kProbeKeys;
    return (k == 4 || k == 16) ? k : 8;
}

Timer &materialize_timer() {
    static thread_local Timer t;
    return t;
}

void publish(const mi355_npo_stats &st) {
    g_last_npo = st;
    mi355_rho_stats rs{};
    rs.matches = st.matches;
    rs.ms_h2d = st.ms_h2d;
    rs.ms_build = st.ms_build;
    rs.ms_probe = st.ms_probe;
    rs.ms_join = st.ms_clear + st.ms_build + st.ms_probe;
    rs.ms_total = st.ms_total;
    rho::set_last_join_stats(rs);
}

// The join on device-resident relations; out (device, cap triples) for a materialising
// join.  Caller holds ctx->mu.
int join_device(Context *ctx, hipStream_t s, const row_t *dR, uint64_t nR, const row_t *dS, uint64_t nS,
                int bucket_bits, bool materialize, bool timing, output_triple_t *out, uint64_t cap,
                mi355_npo_stats *st) {
    const uint64_t nb = bucket_bits ? 1ull << bucket_bits : npo::next_pow2(std::max<uint64_t>(1, nR / 2));
    st->num_buckets = nb;
    const size_t table_bytes = npo::kCtrlBytes + nb * sizeof(uint4);
    SGX_HIP(ctx->npo_table.ensure(table_bytes));
    if (materialize) SGX_HIP(ctx->npo_bpay.ensure(nb * npo::kBucketCap * sizeof(uint32_t)));

    npo::Table t{};
    t.ctrl = ctx->npo_table.as<uint32_t>();
    t.buckets = reinterpret_cast<uint4 *>(ctx->npo_table.as<char>() + npo::kCtrlBytes);
    t.bpay = materialize ? ctx->npo_bpay.as<uint32_t>() : nullptr;
    t.mask = (uint32_t)(nb - 1);

    Timer &tm = thread_timer();
    uint64_t *res = ctx->host_result;
    uint64_t overflow = 0;
    // The node pool exists once a join has overflowed a bucket.  A build that finds it
    // missing or too small only counts the nodes it needs; the join then runs again with
    // a pool for the worst case (every tuple beyond two in one bucket).
    for (int attempt = 0;; ++attempt) {
        const bool pool = ctx->npo_nodes.ptr && (!materialize || ctx->npo_npay.ptr);
        const uint64_t cap_nodes =
            pool ? std::min<uint64_t>(ctx->npo_nodes.bytes / sizeof(uint2),
                                      materialize ? ctx->npo_npay.bytes / sizeof(uint32_t) : ~0ull)
                 : 0;
        t.nodes = pool ? ctx->npo_nodes.as<uint2>() : nullptr;
        t.npay = pool && materialize ? ctx->npo_npay.as<uint32_t>() : nullptr;
        t.pool_cap = (uint32_t)std::min<uint64_t>(cap_nodes, 0x7FFFFFFFull);

        tm.begin_call(s, true, !timing);
        tm.mark("npo_clear");
        SGX_HIP(hipMemsetAsync(ctx->npo_table.ptr, 0, table_bytes, s));
        tm.mark("npo_build");
        SGX_HIP(npo::launch_build(dR, nR, t, write_through_enabled(), s));
        tm.mark("npo_probe");
        SGX_HIP(npo::launch_probe(dS, nS, t, probe_keys_in_flight(), s));
        tm.end_call();
        SGX_HIP(hipMemcpyAsync(res, t.ctrl, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        SGX_HIP(hipStreamSynchronize(s));
        tm.collect();
        overflow = res[0] & 0xFFFFFFFFull;
        if (overflow <= t.pool_cap) break;
        if (attempt > 0) {
            set_last_error("npo: the node pool overflowed after it was sized for the worst case");
            return MI355_ERR_HIP;
        }
        SGX_HIP(ctx->npo_nodes.ensure(nR * sizeof(uint2)));
        if (materialize) SGX_HIP(ctx->npo_npay.ensure(nR * sizeof(uint32_t)));
    }
    // (a counting join after a materialising one, or the reverse, may find only one of
    // the two pool buffers: the pool then counts as missing and the second round sizes both)
    st->matches = res[npo::kCtrlMatches];
    st->overflow_nodes = overflow;
    st->max_chain = 0;
    st->table_bytes = nb * sizeof(uint4) + (materialize ? nb * npo::kBucketCap * sizeof(uint32_t) : 0) +
                      overflow * (sizeof(uint2) + (materialize ? sizeof(uint32_t) : 0));
    st->ms_clear = tm.ms_of_prefix("npo_clear");
    st->ms_build = tm.ms_of_prefix("npo_build");
    st->ms_probe = tm.ms_of_prefix("npo_probe");
    st->ms_total = tm.coarse() ? tm.ms_of_prefix("total") : st->ms_clear + st->ms_build + st->ms_probe;
    if (!materialize) return MI355_OK;

    // materialise: the count is known, so a too-small buffer fails before anything is written
    if (st->matches > cap || (st->matches > 0 && out == nullptr)) {
        set_last_error("materialize: output capacity too small");
        return MI355_ERR_CAPACITY;
    }
    if (st->matches == 0) return MI355_OK;
    Timer &tw = materialize_timer();
    tw.begin_call(s, true, false);
    tw.mark("npo_materialize");
    SGX_HIP(npo::launch_probe_materialize(dS, nS, t, out, cap, s));
    tw.end_call();
    SGX_HIP(hipMemcpyAsync(res, t.ctrl, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    SGX_HIP(hipStreamSynchronize(s));
    tw.collect();
    if (res[npo::kCtrlOut] != st->matches) {
        set_last_error("npo: the materialising probe and the count probe disagree");
        return MI355_ERR_HIP;
    }
    const double ms_mat = tw.ms_of_prefix("npo_materialize");
    st->ms_probe += timing ? ms_mat : 0.0;
    st->ms_total += ms_mat;
    if (timing) tm.append(tw);
    return MI355_OK;
}

}  // namespace

extern "C" {

int mi355_last_npo_stats(mi355_npo_stats *out) {
    if (!out) return MI355_ERR_INVALID;
    *out = g_last_npo;
    return MI355_OK;
}

int mi355_npo_join_ex(const row_t *R, uint64_t nR, const row_t *S, uint64_t nS, const mi355_npo_opts *opts,
                      mi355_npo_stats *stats) {
    if ((!R && nR) || (!S && nS)) {
        set_last_error("null relation");
        return MI355_ERR_INVALID;
    }
    const bool materialize = opts && opts->materialize;
    if (materialize && opts->out_capacity > 0 && opts->out == nullptr) {
        set_last_error("materialize: out is NULL");
        return MI355_ERR_INVALID;
    }
    const int bits = opts ? opts->bucket_bits : 0;
    if (bits < 0 || bits > 31 || nR > (1ull << 31) || nS > (1ull << 31)) {
        set_last_error("npo: bucket_bits must be 0..31 and the relations at most 2^31 tuples");
        return MI355_ERR_INVALID;
    }
    int status = MI355_OK;
    Context *ctx = current_context(&status);
    if (!ctx) return status;
    std::lock_guard<std::mutex> lk(ctx->mu);
    hipStream_t s = thread_stream(ctx, opts ? opts->stream : nullptr);
    mi355_npo_stats local{};
    mi355_npo_stats *st = stats ? stats : &local;
    std::memset(st, 0, sizeof(*st));
    struct Remember {  // publish the stats of this call on every return path
        mi355_npo_stats *st;
        ~Remember() { publish(*st); }
    } remember{st};
    if (nR == 0 || nS == 0) return MI355_OK;

    const row_t *dR = R, *dS = S;
    const auto t0 = std::chrono::steady_clock::now();
    bool staged = false;
    if (!is_device_pointer(R)) {
        SGX_HIP(ctx->inR.ensure(nR * sizeof(row_t)));
        SGX_HIP(hipMemcpyAsync(ctx->inR.ptr, R, nR * sizeof(row_t), hipMemcpyHostToDevice, s));
        dR = ctx->inR.as<row_t>();
        staged = true;
    }
    if (!is_device_pointer(S)) {
        SGX_HIP(ctx->inS.ensure(nS * sizeof(row_t)));
        SGX_HIP(hipMemcpyAsync(ctx->inS.ptr, S, nS * sizeof(row_t), hipMemcpyHostToDevice, s));
        dS = ctx->inS.as<row_t>();
        staged = true;
    }
    if (staged) {
        SGX_HIP(hipStreamSynchronize(s));
        st->ms_h2d = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    const bool timing = (opts && opts->timing) || thread_timing_enabled();
    if (!materialize) return join_device(ctx, s, dR, nR, dS, nS, bits, false, timing, nullptr, 0, st);
    // materialise: straight into a device buffer, or through the context's buffer into host memory
    const uint64_t cap = opts->out_capacity;
    if (opts->out == nullptr || is_device_pointer(opts->out))
        return join_device(ctx, s, dR, nR, dS, nS, bits, true, timing, opts->out, cap, st);
    SGX_HIP(ctx->mat.ensure(std::max<uint64_t>(cap, 1) * sizeof(output_triple_t)));
    const int rc = join_device(ctx, s, dR, nR, dS, nS, bits, true, timing, ctx->mat.as<output_triple_t>(), cap, st);
    if (rc) return rc;
    SGX_HIP(hipMemcpyAsync(opts->out, ctx->mat.ptr, st->matches * sizeof(output_triple_t), hipMemcpyDeviceToHost, s));
    SGX_HIP(hipStreamSynchronize(s));
    return MI355_OK;
}

// Drop-in for PHT() and its variants (no_partitioning_hash_join.cpp:166-249): fills
// result_t as mi355_rho_join does.
int mi355_npo_join(const table_t *relR, const table_t *relS, const joinconfig_t *config, result_t *out) {
    if (!relR || !relS || !out) {
        set_last_error("null argument");
        return MI355_ERR_INVALID;
    }
    const bool materialize = config && config->MATERIALIZE;
    mi355_npo_stats st{};
    int rc;
    output_triple_t *host = nullptr;
    mi355_npo_opts o{};
    o.timing = 1;  // the drop-in logs the reference's phase lines (print_timing)
    if (!materialize) {
        rc = mi355_npo_join_ex(relR->tuples, relR->num_tuples, relS->tuples, relS->num_tuples, &o, &st);
    } else {
        // count first (capacity 0 -> MI355_ERR_CAPACITY with the size), then materialise
        o.materialize = 1;
        rc = mi355_npo_join_ex(relR->tuples, relR->num_tuples, relS->tuples, relS->num_tuples, &o, &st);
        if (rc == MI355_ERR_CAPACITY || (rc == MI355_OK && st.matches > 0)) {
            const uint64_t need = st.matches;
            host = static_cast<output_triple_t *>(std::malloc(std::max<uint64_t>(need, 1) * sizeof(output_triple_t)));
            if (!host) {
                set_last_error("host allocation of the materialised result failed");
                return MI355_ERR_OOM;
            }
            o.out = host;
            o.out_capacity = need;
            rc = mi355_npo_join_ex(relR->tuples, relR->num_tuples, relS->tuples, relS->num_tuples, &o, &st);
        }
    }
    if (rc) {
        std::free(host);
        return rc;
    }
    out->totalresults = (int64_t)st.matches;
    out->nthreads = config ? config->NTHREADS : 1;
    const double us = st.ms_total * 1000.0;
    out->throughput = us > 0 ? (double)(relR->num_tuples + relS->num_tuples) / us : 0.0;  // M rec/s
    out->materialized = materialize ? 1 : 0;
    out->result = nullptr;
    out->result_type = 0;
    if (materialize) {
        chunked_table_t *t = rho::make_chunked_table(host, st.matches);
        std::free(host);
        if (!t) {
            set_last_error("host allocation of the chunked table failed");
            return MI355_ERR_OOM;
        }
        out->result = t;
        out->result_type = 1;
    }
    return MI355_OK;
}

}  // extern "C"
