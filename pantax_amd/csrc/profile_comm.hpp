// profile_comm.hpp -- the rank protocol of the file seam (api_profile.cpp): the caller's collectives behind one object, and the trace clock.
#pragma once
#include <chrono>
#include "common.hpp"

namespace ptx {
// One process per GPU; the ranks meet in the caller's all-reduce / alltoallv (RCCL / MPI / ...).  THE RULE: every rank-local failure travels in a
// flag of the next collective: either all ranks go on or all return (nobody is left waiting in an exchange); the failing rank reports its own error,
// the others E_STATE.  So a phase between two collectives hands its status to the next one ("local status in, agreed status out") and returns only
// behind it; a plain PTX_TRY is right only where every rank fails alike, or on a collective's own status.
struct RankComm {
    pantax_hip_ctx *ctx; const pantax_hip_profiling_config *cfg;
    int W = 1, rk = 0; bool use_comm = false;   // W > 1, or a one-rank world that was given the callbacks: it still goes through them
    int allreduce(double *buf, uint64_t n) const {
        if (!use_comm) return 0;
        const int rc = cfg->allreduce_sum(cfg->comm_user, buf, n);
        return rc == 0 ? 0 : fail(ctx, PANTAX_HIP_E_STATE, "profile: the caller's allreduce_sum returned %d", rc);
    }
    int others_failed() const { return fail(ctx, PANTAX_HIP_E_STATE, "profile: another rank failed; this rank stopped with it"); }
    // one all-reduce of a flag: 0 everywhere, or the local error / E_STATE everywhere
    int agree(int local_rc) const {
        if (!use_comm) return local_rc;
        double f = local_rc != 0 ? 1.0 : 0.0;
        PTX_TRY(allreduce(&f, 1));
        if (f != 0.0) return local_rc ? local_rc : others_failed();
        return 0;
    }
    // who sends how many bytes to whom: every rank fills its row of a W x W matrix, one all-reduce (it also carries the
    // failure flag of the phase before).  -> recv_off [W+1] of this rank
    int exchange_sizes(const uint64_t *send_off, std::vector<uint64_t> &recv_off, int local_rc) const {
        std::vector<double> m((size_t)W * W + 1, 0.0);
        if (local_rc == 0) for (int j = 0; j < W; ++j) m[(size_t)rk * W + j] = (double)(send_off[j + 1] - send_off[j]);
        m[(size_t)W * W] = local_rc != 0 ? 1.0 : 0.0;
        PTX_TRY(allreduce(m.data(), m.size()));
        if (m[(size_t)W * W] != 0.0) return local_rc ? local_rc : others_failed();
        recv_off.assign(W + 1, 0);
        for (int i = 0; i < W; ++i) recv_off[i + 1] = recv_off[i] + (uint64_t)m[(size_t)i * W + rk];
        return 0;
    }
    // bytes between the ranks (sharded ingest).  The callback takes host or device pointers (comm_device_buffers); both
    // forms are offered here so that neither the small id exchange nor the read payload is staged more than needed.
    int a2a(const void *send, const uint64_t *send_off, void *recv, const uint64_t *recv_off) const {
        const int rc = cfg->alltoallv(cfg->comm_user, send, send_off, recv, recv_off);
        return rc == 0 ? 0 : fail(ctx, PANTAX_HIP_E_STATE, "profile: the caller's alltoallv returned %d", rc);
    }
    int a2a_host(const void *send_h, const uint64_t *send_off, std::vector<uint8_t> &recv_h, const uint64_t *recv_off) const {
        recv_h.resize(recv_off[W] ? recv_off[W] : 1);
        if (!cfg->comm_device_buffers) return a2a(send_h, send_off, recv_h.data(), recv_off);
        DevBuf<uint8_t> ds, dr;
        PTX_HIP(ctx, ds.alloc(send_off[W] ? send_off[W] : 1)); PTX_HIP(ctx, dr.alloc(recv_off[W] ? recv_off[W] : 1));
        if (send_off[W]) PTX_HIP(ctx, hipMemcpyAsync(ds.p, send_h, send_off[W], hipMemcpyHostToDevice, ctx->stream));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        PTX_TRY(a2a(ds.p, send_off, dr.p, recv_off));
        if (recv_off[W]) PTX_HIP(ctx, hipMemcpyAsync(recv_h.data(), dr.p, recv_off[W], hipMemcpyDeviceToHost, ctx->stream));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return 0;
    }
    int a2a_dev(const void *send_d, const uint64_t *send_off, void *recv_d, const uint64_t *recv_off) const {
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (cfg->comm_device_buffers) return a2a(send_d, send_off, recv_d, recv_off);
        std::vector<uint8_t> hs(send_off[W] ? send_off[W] : 1), hrv(recv_off[W] ? recv_off[W] : 1);
        if (send_off[W]) PTX_HIP(ctx, hipMemcpy(hs.data(), send_d, send_off[W], hipMemcpyDeviceToHost));
        PTX_TRY(a2a(hs.data(), send_off, hrv.data(), recv_off));
        if (recv_off[W]) PTX_TRY(upload_big(ctx, recv_d, hrv.data(), recv_off[W]));
        return 0;
    }
};
// PANTAX_HIP_TRACE=1: wall time of each phase on stderr (the reference logs its phases through env_logger)
struct Lap {
    bool trace; int rk;
    std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
    void operator()(const char *what) {
        if (!trace) return;
        (void)hipDeviceSynchronize();
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[pantax_hip_profile r%d] %-28s %9.3f ms\n", rk, what, std::chrono::duration<double, std::milli>(now - t_prev).count());
        t_prev = now;
    }
};
}  // namespace ptx
