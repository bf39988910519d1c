// Sort-merge join (MWAY / PSM / RSM), host side: the sort's ping-pong workspace, the plan
// of the passes that run, the sort and merge launches on the join's stream and the C-ABI
// of sgxamd/rho.h (mi355_smj_*, mi355_sort_rows).  Kernels: smj_kernels.hip; geometry and
// workspace layout: smj_internal.hpp.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "rho_device.hpp"
#include "runtime.hpp"
#include "sgxamd/rho.h"
#include "smj_internal.hpp"

using namespace sgxamd;

namespace {

thread_local mi355_smj_stats g_last_smj{};

// SGXAMD_SMJ_DIRECT=1: the scatter stores every element from its lane instead of staging
// the tile through LDS (development A/B switch, read at every call so that one process can
// alternate the two forms; DESIGN.md §3 "Sort-merge join", profiles/smj_ab.log).
bool staged_scatter() {
    const char *e = std::getenv("SGXAMD_SMJ_DIRECT");
    return !(e && std::atoi(e) == 1);
}

Timer &materialize_timer() {
    static thread_local Timer t;
    return t;
}

void publish(const mi355_smj_stats &st) {
    g_last_smj = st;
    mi355_rho_stats rs{};
    rs.matches = st.matches;
    rs.ms_h2d = st.ms_h2d;
    rs.ms_partition = st.ms_sort_r + st.ms_sort_s;
    rs.ms_join = st.ms_merge;
    rs.ms_total = st.ms_total;
    rho::set_last_join_stats(rs);
}

// Bit p set: digit p of key - min takes more than one value over the relation, so pass p runs.
uint32_t passes_to_run(const uint32_t *ghist) {
    uint32_t mask = 0;
    for (uint32_t p = 0; p < smj::kPasses; ++p) {
        uint32_t bins = 0;
        for (uint32_t d = 0; d < smj::kDigits; ++d) bins += ghist[p * smj::kDigits + d] != 0;
        if (bins > 1) mask |= 1u << p;
    }
    return mask;
}

uint32_t popcount4(uint32_t m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1); }

struct Sorted {
    const void *ptr;  // the relation in ascending key order
    int bytes;        // 8: tuples, 4: keys
};

// Enqueues the passes of `mask` over the n tuples at in.  The last pass writes ping[0],
// the one before it ping[1], and so on; elements are elem_bytes wide after the first read.
// in is only read.  bias: the relation's smallest key (the passes order by key - bias);
// tag names the relation in the timing records.
int enqueue_sort(hipStream_t s, Timer &tm, const std::string &tag, const row_t *in, uint64_t n, uint32_t mask,
                 uint32_t bias, int elem_bytes, void *const ping[2], const uint32_t *ghist, uint32_t *tile_hist,
                 Sorted *res) {
    const uint32_t P = popcount4(mask);
    const bool staged = staged_scatter();
    const void *src = in;
    int src_bytes = 8;
    uint32_t i = 0;
    for (uint32_t p = 0; p < smj::kPasses; ++p) {
        if (!(mask & (1u << p))) continue;
        void *dst = ping[(P - 1 - i) & 1];
        tm.mark((tag + "_hist").c_str());
        SGX_HIP(smj::launch_tile_hist(src, src_bytes, n, bias, 8 * p, tile_hist, s));
        tm.mark((tag + "_scan").c_str());
        SGX_HIP(smj::launch_scan(tile_hist, n, ghist + p * smj::kDigits, s));
        tm.mark((tag + "_scatter").c_str());
        SGX_HIP(smj::launch_scatter(src, src_bytes, dst, elem_bytes, n, bias, 8 * p, tile_hist, staged, s));
        src = dst;
        src_bytes = elem_bytes;
        ++i;
    }
    res->ptr = src;
    res->bytes = src_bytes;
    return MI355_OK;
}

std::vector<uint32_t> &host_ghist() {
    static thread_local std::vector<uint32_t> v(smj::kPlanWords);
    return v;
}

// The join on device-resident relations; out (device, cap triples) for a materialising
// join.  Caller holds ctx->mu.
int join_device(Context *ctx, hipStream_t s, const row_t *dR, uint64_t nR, const row_t *dS, uint64_t nS, bool r_sorted,
                bool s_sorted, bool materialize, bool timing, output_triple_t *out, uint64_t cap,
                mi355_smj_stats *st) {
    const int eb = materialize ? 8 : 4;
    st->elem_bytes = (uint32_t)eb;
    const uint64_t tiles = std::max(smj::tiles_of(nR), smj::tiles_of(nS));
    SGX_HIP(ctx->smj_ctrl.ensure(smj::kOffTileHist + tiles * smj::kDigits * sizeof(uint32_t)));
    SGX_HIP(ctx->smj_split.ensure(((uint64_t)smj::chunks_of(nR + nS) + 1) * sizeof(uint2)));
    char *ctrl = ctx->smj_ctrl.as<char>();
    uint32_t *ghR = reinterpret_cast<uint32_t *>(ctrl + smj::kOffGhistR);
    uint32_t *ghS = reinterpret_cast<uint32_t *>(ctrl + smj::kOffGhistS);
    uint32_t *inv_min = reinterpret_cast<uint32_t *>(ctrl + smj::kOffMin);
    uint64_t *result = reinterpret_cast<uint64_t *>(ctrl + smj::kOffResult);
    uint32_t *tile_hist = reinterpret_cast<uint32_t *>(ctrl + smj::kOffTileHist);
    uint2 *split = ctx->smj_split.as<uint2>();

    Timer &tm = thread_timer();
    SGX_HIP(hipMemsetAsync(ctrl, 0, smj::kOffTileHist, s));
    tm.begin_call(s, true, !timing);
    uint32_t maskR = 0, maskS = 0, biasR = 0, biasS = 0;
    if (!r_sorted || !s_sorted) {
        if (!r_sorted) {
            tm.mark("smj_sort_r_min");
            SGX_HIP(smj::launch_min(dR, nR, inv_min, s));
            tm.mark("smj_sort_r_digits");
            SGX_HIP(smj::launch_digits(dR, nR, ghR, inv_min, s));
        }
        if (!s_sorted) {
            tm.mark("smj_sort_s_min");
            SGX_HIP(smj::launch_min(dS, nS, inv_min + 1, s));
            tm.mark("smj_sort_s_digits");
            SGX_HIP(smj::launch_digits(dS, nS, ghS, inv_min + 1, s));
        }
        // the host decides which passes run: the wait lies in a span of its own
        tm.mark("smj_plan");
        std::vector<uint32_t> &gh = host_ghist();
        SGX_HIP(hipMemcpyAsync(gh.data(), ghR, smj::kPlanWords * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        SGX_HIP(hipStreamSynchronize(s));
        biasR = ~gh[2 * smj::kGhistWords];
        biasS = ~gh[2 * smj::kGhistWords + 1];
        maskR = r_sorted ? 0 : passes_to_run(gh.data());
        maskS = s_sorted ? 0 : passes_to_run(gh.data() + smj::kGhistWords);
    }
    st->sort_passes_r = popcount4(maskR);
    st->sort_passes_s = popcount4(maskS);
    if (st->sort_passes_r > 0) SGX_HIP(ctx->smj_ra.ensure(nR * eb));
    if (st->sort_passes_r > 1) SGX_HIP(ctx->smj_rb.ensure(nR * eb));
    if (st->sort_passes_s > 0) SGX_HIP(ctx->smj_sa.ensure(nS * eb));
    if (st->sort_passes_s > 1) SGX_HIP(ctx->smj_sb.ensure(nS * eb));

    Sorted sr{dR, 8}, ss{dS, 8};  // a relation passed as sorted, or of one key, is read where it lies
    void *const pingR[2] = {ctx->smj_ra.ptr, ctx->smj_rb.ptr};
    void *const pingS[2] = {ctx->smj_sa.ptr, ctx->smj_sb.ptr};
    if (int rc = enqueue_sort(s, tm, "smj_sort_r", dR, nR, maskR, biasR, eb, pingR, ghR, tile_hist, &sr)) return rc;
    if (int rc = enqueue_sort(s, tm, "smj_sort_s", dS, nS, maskS, biasS, eb, pingS, ghS, tile_hist, &ss)) return rc;
    tm.mark("smj_merge_partition");
    SGX_HIP(smj::launch_partition(sr.ptr, sr.bytes, nR, ss.ptr, ss.bytes, nS, split, s));
    tm.mark("smj_merge_count");
    SGX_HIP(smj::launch_merge_count(sr.ptr, sr.bytes, nR, ss.ptr, ss.bytes, nS, split, result, s));
    tm.end_call();
    uint64_t *res = ctx->host_result;
    SGX_HIP(hipMemcpyAsync(res, result, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    SGX_HIP(hipStreamSynchronize(s));
    tm.collect();
    st->matches = res[smj::kResMatches];
    st->ms_sort_r = tm.ms_of_prefix("smj_sort_r");
    st->ms_sort_s = tm.ms_of_prefix("smj_sort_s");
    st->ms_merge = tm.ms_of_prefix("smj_merge");
    st->ms_total = tm.coarse() ? tm.ms_of_prefix("total") : st->ms_sort_r + st->ms_sort_s + st->ms_merge;
    if (!materialize) return MI355_OK;

    // materialise: the count is known, so a too-small buffer fails before anything is written
    if (st->matches > cap || (st->matches > 0 && out == nullptr)) {
        set_last_error("materialize: output capacity too small");
        return MI355_ERR_CAPACITY;
    }
    if (st->matches == 0) return MI355_OK;
    Timer &tw = materialize_timer();
    tw.begin_call(s, true, false);
    tw.mark("smj_merge_emit");
    SGX_HIP(smj::launch_merge_emit(static_cast<const uint64_t *>(sr.ptr), nR, static_cast<const uint64_t *>(ss.ptr), nS,
                                   split, result, out, cap, s));
    tw.end_call();
    SGX_HIP(hipMemcpyAsync(res, result, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    SGX_HIP(hipStreamSynchronize(s));
    tw.collect();
    if (res[smj::kResOut] != st->matches) {
        set_last_error("smj: the materialising merge and the counting merge disagree");
        return MI355_ERR_HIP;
    }
    const double ms_emit = tw.ms_of_prefix("smj_merge_emit");
    st->ms_merge += timing ? ms_emit : 0.0;
    st->ms_total += ms_emit;
    if (timing) tm.append(tw);
    return MI355_OK;
}

}  // namespace

extern "C" {

int mi355_last_smj_stats(mi355_smj_stats *out) {
    if (!out) return MI355_ERR_INVALID;
    *out = g_last_smj;
    return MI355_OK;
}

int mi355_smj_join_ex(const row_t *R, uint64_t nR, const row_t *S, uint64_t nS, const mi355_smj_opts *opts,
                      mi355_smj_stats *stats) {
    if ((!R && nR) || (!S && nS)) {
        set_last_error("null relation");
        return MI355_ERR_INVALID;
    }
    const bool materialize = opts && opts->materialize;
    if (materialize && opts->out_capacity > 0 && opts->out == nullptr) {
        set_last_error("materialize: out is NULL");
        return MI355_ERR_INVALID;
    }
    if (nR > (1ull << 31) || nS > (1ull << 31)) {
        set_last_error("smj: the relations hold at most 2^31 tuples");
        return MI355_ERR_INVALID;
    }
    int status = MI355_OK;
    Context *ctx = current_context(&status);
    if (!ctx) return status;
    std::lock_guard<std::mutex> lk(ctx->mu);
    hipStream_t s = thread_stream(ctx, opts ? opts->stream : nullptr);
    mi355_smj_stats local{};
    mi355_smj_stats *st = stats ? stats : &local;
    std::memset(st, 0, sizeof(*st));
    st->sort_tile = smj::kSortTile;
    st->merge_tile = smj::kMergeTile;
    struct Remember {  // publish the stats of this call on every return path
        mi355_smj_stats *st;
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
    const bool rs = opts && opts->r_sorted, ssrt = opts && opts->s_sorted;
    if (!materialize) return join_device(ctx, s, dR, nR, dS, nS, rs, ssrt, false, timing, nullptr, 0, st);
    // materialise: straight into a device buffer, or through the context's buffer into host memory
    const uint64_t cap = opts->out_capacity;
    if (opts->out == nullptr || is_device_pointer(opts->out))
        return join_device(ctx, s, dR, nR, dS, nS, rs, ssrt, true, timing, opts->out, cap, st);
    SGX_HIP(ctx->mat.ensure(std::max<uint64_t>(cap, 1) * sizeof(output_triple_t)));
    const int rc = join_device(ctx, s, dR, nR, dS, nS, rs, ssrt, true, timing, ctx->mat.as<output_triple_t>(), cap, st);
    if (rc) return rc;
    SGX_HIP(hipMemcpyAsync(opts->out, ctx->mat.ptr, st->matches * sizeof(output_triple_t), hipMemcpyDeviceToHost, s));
    SGX_HIP(hipStreamSynchronize(s));
    return MI355_OK;
}

// Drop-in for MWAY(), PSM() and RSM(): fills result_t as mi355_npo_join does.
int mi355_smj_join(const table_t *relR, const table_t *relS, const joinconfig_t *config, result_t *out) {
    if (!relR || !relS || !out) {
        set_last_error("null argument");
        return MI355_ERR_INVALID;
    }
    const bool materialize = config && config->MATERIALIZE;
    mi355_smj_stats st{};
    int rc;
    output_triple_t *host = nullptr;
    mi355_smj_opts o{};
    o.timing = 1;  // the drop-ins log the reference's phase lines (print_timing)
    o.r_sorted = relR->sorted != 0;
    o.s_sorted = relS->sorted != 0;
    if (!materialize) {
        rc = mi355_smj_join_ex(relR->tuples, relR->num_tuples, relS->tuples, relS->num_tuples, &o, &st);
    } else {
        // count first (capacity 0 -> MI355_ERR_CAPACITY with the size), then materialise
        o.materialize = 1;
        rc = mi355_smj_join_ex(relR->tuples, relR->num_tuples, relS->tuples, relS->num_tuples, &o, &st);
        if (rc == MI355_ERR_CAPACITY || (rc == MI355_OK && st.matches > 0)) {
            const uint64_t need = st.matches;
            host = static_cast<output_triple_t *>(std::malloc(std::max<uint64_t>(need, 1) * sizeof(output_triple_t)));
            if (!host) {
                set_last_error("host allocation of the materialised result failed");
                return MI355_ERR_OOM;
            }
            o.out = host;
            o.out_capacity = need;
            rc = mi355_smj_join_ex(relR->tuples, relR->num_tuples, relS->tuples, relS->num_tuples, &o, &st);
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

int mi355_sort_rows(const row_t *in, uint64_t n, row_t *out, uint32_t *passes, void *stream) {
    if (n && (!in || !out)) {
        set_last_error("null relation");
        return MI355_ERR_INVALID;
    }
    if (n && in == out) {
        set_last_error("sort_rows: out must not be in");
        return MI355_ERR_INVALID;
    }
    if (n > (1ull << 31)) {
        set_last_error("sort_rows: at most 2^31 tuples");
        return MI355_ERR_INVALID;
    }
    if (passes) *passes = 0;
    if (n == 0) return MI355_OK;
    int status = MI355_OK;
    Context *ctx = current_context(&status);
    if (!ctx) return status;
    std::lock_guard<std::mutex> lk(ctx->mu);
    hipStream_t s = thread_stream(ctx, stream);
    const row_t *dIn = in;
    if (!is_device_pointer(in)) {
        SGX_HIP(ctx->inR.ensure(n * sizeof(row_t)));
        SGX_HIP(hipMemcpyAsync(ctx->inR.ptr, in, n * sizeof(row_t), hipMemcpyHostToDevice, s));
        dIn = ctx->inR.as<row_t>();
    }
    const bool host_out = !is_device_pointer(out);
    SGX_HIP(ctx->smj_ctrl.ensure(smj::kOffTileHist + (uint64_t)smj::tiles_of(n) * smj::kDigits * sizeof(uint32_t)));
    char *ctrl = ctx->smj_ctrl.as<char>();
    uint32_t *gh_dev = reinterpret_cast<uint32_t *>(ctrl + smj::kOffGhistR);
    uint32_t *inv_min = reinterpret_cast<uint32_t *>(ctrl + smj::kOffMin);
    uint32_t *tile_hist = reinterpret_cast<uint32_t *>(ctrl + smj::kOffTileHist);
    Timer &tm = thread_timer();
    SGX_HIP(hipMemsetAsync(ctrl, 0, smj::kOffTileHist, s));
    tm.begin_call(s, thread_timing_enabled(), false);
    tm.mark("smj_sort_min");
    SGX_HIP(smj::launch_min(dIn, n, inv_min, s));
    tm.mark("smj_sort_digits");
    SGX_HIP(smj::launch_digits(dIn, n, gh_dev, inv_min, s));
    tm.mark("smj_plan");
    std::vector<uint32_t> &gh = host_ghist();
    SGX_HIP(hipMemcpyAsync(gh.data(), gh_dev, smj::kPlanWords * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    SGX_HIP(hipStreamSynchronize(s));
    const uint32_t bias = ~gh[2 * smj::kGhistWords];
    const uint32_t mask = passes_to_run(gh.data());
    const uint32_t P = popcount4(mask);
    if (passes) *passes = P;
    if (P == 0) {  // one key: the input is its own stable order
        tm.mark("smj_sort_copy");
        SGX_HIP(hipMemcpyAsync(out, dIn, n * sizeof(row_t), host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
        tm.end_call();
        SGX_HIP(hipStreamSynchronize(s));
        tm.collect();
        return MI355_OK;
    }
    if (host_out) SGX_HIP(ctx->smj_ra.ensure(n * sizeof(row_t)));
    if (P > 1) SGX_HIP(ctx->smj_rb.ensure(n * sizeof(row_t)));
    void *const ping[2] = {host_out ? ctx->smj_ra.ptr : static_cast<void *>(out), ctx->smj_rb.ptr};
    Sorted res{};
    if (int rc = enqueue_sort(s, tm, "smj_sort", dIn, n, mask, bias, 8, ping, gh_dev, tile_hist, &res)) return rc;
    tm.end_call();
    if (host_out) SGX_HIP(hipMemcpyAsync(out, res.ptr, n * sizeof(row_t), hipMemcpyDeviceToHost, s));
    SGX_HIP(hipStreamSynchronize(s));
    tm.collect();
    return MI355_OK;
}

}  // extern "C"
