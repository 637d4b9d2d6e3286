// ctx.cpp -- context lifetime, error strings, the option table, HIP-event kernel timing (include/pantax_hip.h).
#include <cstdarg>
#include <algorithm>
#include <cstring>
#include <cstdio>
#include <mutex>
#include <sched.h>
#include <fstream>
#include <cctype>
#include <cstddef>
#include <cstdlib>
#include "common.hpp"
#include "lad.hpp"

namespace ptx {

// error text of the calling thread's last failed call: messages are per thread, so concurrent callers of one ctx
// never read each other's
static thread_local std::string g_init_err;
static thread_local std::string g_thread_err;
static thread_local const Ctx *g_thread_err_ctx = nullptr;

int fail(Ctx *ctx, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) {
        // the per-thread copy is what pantax_hip_last_error returns to the failing thread; the shared one (for other threads)
        // has its own lock: fail() is also reached before an entry point takes the ctx lock
        { std::lock_guard<std::mutex> g(ctx->err_mu); ctx->err = buf; }
        g_thread_err = buf; g_thread_err_ctx = ctx;
    } else g_init_err = buf;
    return code;
}

KTimer::KTimer(Ctx *c, const char *nm) : ctx(c), name(nm) {
    if (!ctx->timing) return;
    if (!ctx->timing_filter.empty()) {   // only the named launches are bracketed ("a" or "a|b|c")
        const std::string &f = ctx->timing_filter;
        const size_t len = std::strlen(nm);
        bool hit = false;
        for (size_t pos = 0; pos <= f.size() && !hit;) {
            const size_t bar = std::min(f.find('|', pos), f.size());
            hit = bar - pos == len && f.compare(pos, len, nm) == 0;
            pos = bar + 1;
        }
        if (!hit) return;
    }
    if (!ctx->free_events.empty()) {
        start = ctx->free_events.back().first;
        stop = ctx->free_events.back().second;
        ctx->free_events.pop_back();
    } else {
        if (hipEventCreate(&start) != hipSuccess || hipEventCreate(&stop) != hipSuccess) { start = stop = nullptr; return; }
    }
    (void)hipEventRecord(start, ctx->stream);
}
KTimer::~KTimer() {
    if (!start) return;
    (void)hipEventRecord(stop, ctx->stream);
    ctx->pending.push_back({name, start, stop});
}

int collect_timings(Ctx *ctx) {
    if (ctx->pending.empty()) return 0;
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (auto &t : ctx->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess) {
            auto &a = ctx->acc[t.name];
            a.first += 1;
            a.second += ms;
        }
        ctx->free_events.push_back({t.start, t.stop});
    }
    ctx->pending.clear();
    return 0;
}

// ---- options: one table, filled from the environment at init, changed through pantax_hip_set_option ----
namespace {
enum OptKind { O_BOOL, O_INT, O_U32, O_U64, O_STR };
struct OptDesc { const char *name; OptKind kind; size_t off; };
#define OPT(nm, kind, field) {nm, kind, offsetof(CtxConfig, field)}
const OptDesc OPTIONS[] = {
    OPT("hip_trace", O_BOOL, trace), OPT("stage_threads", O_INT, stage_threads), OPT("stage_ch_mb", O_INT, stage_ch_mb), OPT("stream_prio", O_BOOL, stream_prio), OPT("numa_bind", O_BOOL, numa_bind), OPT("dev_cache_gb", O_INT, dev_cache_gb),
    OPT("gaf_piece_bytes", O_U64, gaf_piece_bytes), OPT("db_path_steps_max", O_U64, db_path_steps_max), OPT("db_groups", O_INT, db_groups), OPT("trio_path", O_STR, trio_path), OPT("trio_rows", O_STR, trio_rows), OPT("trio_two_pass", O_BOOL, trio_two_pass), OPT("uniq_hash", O_INT, uniq_hash),
    OPT("mask", O_STR, mask), OPT("row_sort", O_STR, row_sort), OPT("objective", O_STR, objective), OPT("read_strain_route", O_STR, read_strain_route), OPT("evidence_route", O_STR, evidence_route), OPT("depth_route", O_STR, depth_route), OPT("depth_grid", O_INT, depth_grid), OPT("near_miss_route", O_STR, near_miss_route), OPT("near_miss_words", O_INT, near_miss_words), OPT("hap_pairs_route", O_STR, hap_pairs_route), OPT("fit_route", O_STR, fit_route), OPT("bootstrap_route", O_STR, bootstrap_route), OPT("bootstrap_rows_max", O_U64, bootstrap_rows_max), OPT("dropout_route", O_STR, dropout_route), OPT("dropout_patterns_max", O_U64, dropout_patterns_max), OPT("dropout_yardstick", O_BOOL, dropout_yardstick), OPT("addin_route", O_STR, addin_route), OPT("addin_patterns_max", O_U64, addin_patterns_max), OPT("addin_yardstick", O_BOOL, addin_yardstick), OPT("rarefy_route", O_STR, rarefy_route), OPT("growth_route", O_STR, growth_route), OPT("rarefy_levels_max", O_U64, rarefy_levels_max), OPT("read_class_slots", O_U64, read_class_slots), OPT("read_em_lds_classes", O_INT, read_em_lds_classes), OPT("hap_pairs_chunk", O_INT, hap_pairs_chunk),
    OPT("cov_general", O_BOOL, cov_general), OPT("cov_long", O_STR, cov_long), OPT("covl_shape", O_INT, covl_shape), OPT("cov_count", O_BOOL, cov_count), OPT("cov_self_clean", O_BOOL, cov_readers_clean), OPT("cov_clean_async", O_INT, cov_clean_async), OPT("cov_arena_verify", O_BOOL, cov_arena_verify), OPT("ncs_no_prefix", O_BOOL, ncs_no_prefix), OPT("ncs_prefix_min", O_INT, ncs_prefix_min), OPT("walk_sum_in_bin", O_BOOL, walk_sum_in_bin), OPT("cov_item_groups", O_INT, cov_item_groups), OPT("tv_u", O_INT, tv_u), OPT("tv_rounds", O_INT, tv_rounds), OPT("tf_u", O_INT, tf_u), OPT("tf_rounds", O_INT, tf_rounds),
    OPT("rows_u", O_INT, rows_u), OPT("tb_slots", O_INT, tb_slots), OPT("trio_xcd", O_INT, trio_xcd), OPT("cov_shape", O_INT, cov_shape),
    OPT("covf_shape", O_INT, covf_shape), OPT("cov_spec", O_STR, cov_spec), OPT("cov_xcd", O_INT, cov_xcd), OPT("group_bucket_bits", O_INT, group_bucket_bits), OPT("tv_ablate", O_U32, tv_ablate),
    OPT("cov_ablate", O_U32, cov_ablate), OPT("ssn_ablate", O_U32, ssn_ablate), OPT("no_absent_skip", O_BOOL, no_absent_skip), OPT("node_pass", O_STR, node_pass), OPT("bin_route", O_STR, bin_route), OPT("node_bits", O_STR, node_bits), OPT("node_bits_words", O_INT, node_bits_words), OPT("lad_shape", O_STR, lad_shape), OPT("ssn_debug", O_BOOL, ssn_debug),
    OPT("ssn_keys", O_STR, ssn_keys), OPT("ssn_poison_keys", O_BOOL, ssn_poison_keys), OPT("ssn_ties_async", O_INT, ssn_ties_async),
    OPT("scan_no_huge", O_BOOL, scan_no_huge), OPT("scan_tile", O_STR, scan_tile), OPT("flag_rank_chained", O_BOOL, flag_rank_chained), OPT("ratio_kernel", O_BOOL, ratio_kernel),
    OPT("mask_pass", O_BOOL, mask_pass), OPT("trio_free_at_filter", O_BOOL, trio_free_at_filter), OPT("trio_after_step", O_BOOL, trio_after_step),
};
#undef OPT
}  // namespace

int ctx_set_option(CtxConfig &cfg, const char *name, const char *value) {
    if (!name) return PANTAX_HIP_E_INVALID;
    static const CtxConfig defaults;
    for (const OptDesc &o : OPTIONS) {
        if (std::strcmp(o.name, name) != 0) continue;
        char *dst = reinterpret_cast<char *>(&cfg) + o.off;
        const char *def = reinterpret_cast<const char *>(&defaults) + o.off;
        char *end = nullptr;
        switch (o.kind) {
        case O_BOOL: *reinterpret_cast<bool *>(dst) = value ? !(value[0] == '0' || value[0] == '\0' || value[0] == 'n' || value[0] == 'f') : *reinterpret_cast<const bool *>(def); return 0;
        case O_INT: { if (!value) { *reinterpret_cast<int *>(dst) = *reinterpret_cast<const int *>(def); return 0; }
                      const long v = std::strtol(value, &end, 10); if (end == value) return PANTAX_HIP_E_INVALID; *reinterpret_cast<int *>(dst) = (int)v; return 0; }
        case O_U32: { if (!value) { *reinterpret_cast<uint32_t *>(dst) = *reinterpret_cast<const uint32_t *>(def); return 0; }
                      const unsigned long long v = std::strtoull(value, &end, 10); if (end == value) return PANTAX_HIP_E_INVALID; *reinterpret_cast<uint32_t *>(dst) = (uint32_t)v; return 0; }
        case O_U64: { if (!value) { *reinterpret_cast<uint64_t *>(dst) = *reinterpret_cast<const uint64_t *>(def); return 0; }
                      const unsigned long long v = std::strtoull(value, &end, 10); if (end == value) return PANTAX_HIP_E_INVALID; *reinterpret_cast<uint64_t *>(dst) = (uint64_t)v; return 0; }
        case O_STR: *reinterpret_cast<std::string *>(dst) = value ? value : ""; return 0;
        }
    }
    return PANTAX_HIP_E_INVALID;
}

// the environment, once: PANTAX_<NAME> for every option of the table
static void config_from_env(CtxConfig &cfg) {
    for (const OptDesc &o : OPTIONS) {
        std::string env = "PANTAX_";
        for (const char *p = o.name; *p; ++p) env += (char)std::toupper((unsigned char)*p);
        if (const char *v = std::getenv(env.c_str())) (void)ctx_set_option(cfg, o.name, v);
    }
}

}  // namespace ptx

using namespace ptx;

extern "C" {

const char *pantax_hip_version(void) { return "pantax-hip 0.1.0 (gfx950)"; }

int pantax_hip_set_option(pantax_hip_ctx *ctx, const char *name, const char *value) {
    if (!ctx || !name) return PANTAX_HIP_E_INVALID;
    std::lock_guard<std::recursive_mutex> ptx_lock__(ctx->mu);
    const int rc = ctx_set_option(ctx->cfg, name, value);
    if (rc == 0 && std::strcmp(name, "dev_cache_gb") == 0) dev_cache_set_max(ctx->cfg.dev_cache_gb < 0 ? -1 : (long long)ctx->cfg.dev_cache_gb << 30);
    return rc == 0 ? 0 : fail(ctx, rc, "set_option: unknown option or unparsable value: %s=%s", name, value ? value : "(default)");
}

const char *pantax_hip_lad_shape_name(const pantax_hip_ctx *ctx, uint32_t n_species, int max_columns) {
    if (!ctx) return nullptr;
    return lad_shape_name(lad_shape(ctx->cfg.lad_shape, n_species, ctx->n_cu, max_columns));
}

const char *pantax_hip_last_error(const pantax_hip_ctx *ctx) {
    if (!ctx) return g_init_err.c_str();
    if (g_thread_err_ctx == ctx) return g_thread_err.c_str();   // this thread's own last failure on this ctx
    std::lock_guard<std::mutex> g(const_cast<pantax_hip_ctx *>(ctx)->err_mu);   // another thread's failure: a copy that outlives the lock
    g_thread_err = ctx->err;
    return g_thread_err.c_str();
}

int pantax_hip_init(pantax_hip_ctx **out, const int *device_ids, int n_devices) {
    if (!out) return PANTAX_HIP_E_INVALID;
    *out = nullptr;
    if (n_devices != 1) return fail(nullptr, PANTAX_HIP_E_INVALID, "one ctx drives one GPU (one process per GPU); n_devices=%d", n_devices);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return fail(nullptr, PANTAX_HIP_E_NO_DEVICE, "no HIP device visible (%s); this library has no CPU path",
                    e == hipSuccess ? "count=0" : hipGetErrorString(e));
    int dev = device_ids ? device_ids[0] : 0;
    if (dev < 0 || dev >= count) return fail(nullptr, PANTAX_HIP_E_INVALID, "device id %d out of range (count %d)", dev, count);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, dev)) != hipSuccess) return fail(nullptr, PANTAX_HIP_E_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, PANTAX_HIP_E_NO_DEVICE, "device %d is %s; this build carries gfx950 code only", dev, prop.gcnArchName);
    if ((e = hipSetDevice(dev)) != hipSuccess) return fail(nullptr, PANTAX_HIP_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    pantax_hip_ctx *ctx = new pantax_hip_ctx();
    ctx->device = dev;
    ctx->n_cu = prop.multiProcessorCount;
    config_from_env(ctx->cfg);   // the only place the library reads the environment
    if (ctx->cfg.dev_cache_gb >= 0) dev_cache_set_max((long long)ctx->cfg.dev_cache_gb << 30);
    {   // the GPU's NUMA node and its CPUs (sysfs); anything missing = nothing is bound
        char bus[64] = {0};
        if (hipDeviceGetPCIBusId(bus, sizeof(bus), dev) == hipSuccess) {
            for (char *c = bus; *c; ++c) *c = (char)std::tolower((unsigned char)*c);
            std::ifstream f(std::string("/sys/bus/pci/devices/") + bus + "/numa_node");
            int node = -1;
            if (f >> node && node >= 0) {
                std::ifstream g("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist");
                std::string list;
                if (std::getline(g, list)) {
                    for (size_t pos = 0; pos < list.size();) {
                        const size_t comma = std::min(list.find(',', pos), list.size());
                        const std::string part = list.substr(pos, comma - pos);
                        const size_t dash = part.find('-');
                        const int a = std::atoi(part.c_str()), b = dash == std::string::npos ? a : std::atoi(part.c_str() + dash + 1);
                        for (int c = a; c <= b && c < CPU_SETSIZE; ++c) ctx->numa.cpus.push_back(c);
                        pos = comma + 1;
                    }
                    if (!ctx->numa.cpus.empty()) ctx->numa.node = node;
                }
            }
        }
    }
    // The main stream at the highest priority, the side stream (index rebuild) at the lowest: in a stream of steps the rebuild for
    // step i+1 runs beside the tail of step i, which is the critical chain -- the rebuild has 2 ms of slack and fills what the
    // chain's narrow kernels (sample ranking, the LP workgroups) leave idle instead of taking wave slots from its wide ones
    // (cfg3: 6.80 -> 6.51 ms per step; option stream_prio=0 = equal priorities, for measurements)
    int prio_lo = 0, prio_hi = 0;
    const bool prio = ctx->cfg.stream_prio && hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) == hipSuccess && prio_lo != prio_hi;
    if ((e = prio ? hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, prio_hi) : hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) {
        delete ctx;
        return fail(nullptr, PANTAX_HIP_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    if ((prio ? hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, prio_lo) : hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking)) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_seq, hipEventDisableTiming) != hipSuccess) {
        delete ctx;
        return fail(nullptr, PANTAX_HIP_E_HIP, "hipStreamCreate failed");
    }
    dev_cache_register_stream(dev, ctx->stream, true);
    dev_cache_register_stream(dev, ctx->stream2, true);
    if (ctx->d_scalars.alloc(64) != hipSuccess) {
        delete ctx;
        return fail(nullptr, PANTAX_HIP_E_HIP, "hipMalloc failed");
    }
    *out = ctx;
    return 0;
}

void pantax_hip_destroy(pantax_hip_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &t : ctx->pending) { (void)hipEventDestroy(t.start); (void)hipEventDestroy(t.stop); }
    for (auto &p : ctx->free_events) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    ctx->d_scalars.release();
    ctx->d_scan_ws.release();
    ctx->pin_down.release();
    ctx->pin_up.release();
    for (auto &half : ctx->pin_up_ev) for (hipEvent_t &e : half) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    ctx->pin_text.release();
    if (ctx->stream2) { (void)hipStreamSynchronize(ctx->stream2); dev_cache_register_stream(ctx->device, ctx->stream2, false); (void)hipStreamDestroy(ctx->stream2); }
    if (ctx->stream_up) { (void)hipStreamSynchronize(ctx->stream_up); (void)hipStreamDestroy(ctx->stream_up); }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_seq) (void)hipEventDestroy(ctx->ev_seq);
    if (ctx->ev_ssn_fork) (void)hipEventDestroy(ctx->ev_ssn_fork);
    if (ctx->ev_ssn_join) (void)hipEventDestroy(ctx->ev_ssn_join);
    dev_cache_register_stream(ctx->device, ctx->stream, false);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    dev_cache_trim();   // nothing of this process stays cached on the device once a ctx is gone
}

int pantax_hip_sync(pantax_hip_ctx *ctx) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    std::lock_guard<std::recursive_mutex> ptx_lock__(ctx->mu);
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int pantax_hip_timing_enable(pantax_hip_ctx *ctx, int on) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    std::lock_guard<std::recursive_mutex> ptx_lock__(ctx->mu);
    PTX_TRY(collect_timings(ctx));
    ctx->timing = on != 0;
    return 0;
}

int pantax_hip_timing_filter(pantax_hip_ctx *ctx, const char *name) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    std::lock_guard<std::recursive_mutex> ptx_lock__(ctx->mu);
    ctx->timing_filter = name ? name : "";
    return 0;
}

int pantax_hip_timing_reset(pantax_hip_ctx *ctx) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    std::lock_guard<std::recursive_mutex> ptx_lock__(ctx->mu);
    PTX_TRY(collect_timings(ctx));
    ctx->acc.clear();
    return 0;
}

int pantax_hip_timing_get(pantax_hip_ctx *ctx, int cap, const char **names_out, uint64_t *launches_out, double *total_ms_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    std::lock_guard<std::recursive_mutex> ptx_lock__(ctx->mu);
    PTX_TRY(collect_timings(ctx));
    int i = 0;
    for (auto &kv : ctx->acc) {
        if (i < cap) {
            if (names_out) names_out[i] = kv.first.c_str();
            if (launches_out) launches_out[i] = kv.second.first;
            if (total_ms_out) total_ms_out[i] = kv.second.second;
        }
        ++i;
    }
    return i;
}

}  // extern "C"
