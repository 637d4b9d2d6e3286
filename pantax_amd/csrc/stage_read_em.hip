// stage_read_em.hip -- read classes and the read-based estimate (pantax_hip_strain_read_em, the --strain-em report): the counted reads of a species grouped
// by their candidate mask C(r), and a depth per candidate from EM over those classes.  Not a stage of the reference.
//
// Contract (include/pantax_hip.h, DESIGN.md "Read classes and the read-based estimate"): a counted read, N(r), C(r) and Q(r) = (1, #steps, span) are those of
// the per-strain read support (stage_read_support.hip).  A class is a distinct non-zero mask over the candidates of a species of 1 <= K_s <= 64 in ascending
// haplotype index, with the u64 sums of Q over its reads; the estimate is the fixed f64 iteration of the header over a species' classes in ascending mask.
//
// read_class_kernel forms C(r) exactly as read_support_kernel does (read_pass_device.hpp: a wave per 64-step group, a lane per step, the segmented AND
// on the DPP path; the lane of a walk's last step decides); on route 1 the word's haplotype bits are compressed to candidate ranks.  The WAVE reduces before
// it touches memory: it takes the species of its first deciding lane left (counted: one reduction), then within the species the mask of the first lane
// left, ballots the lanes that carry the same mask, reduces their Q and lane 0 files ONE class -- core reads share one mask, so the hot class costs one set
// of atomics per wave and not 64.  Filing: every species owns a region of an open-addressed table (keys u64, 0 = empty; mask 0 never enters: it is the
// species' unexplained counter; three u64 counters per slot, zero-filled once).  Lane 0 probes from a hash of the mask: a slot whose key is the mask, or that
// an atomicCAS(0 -> mask) claims or finds claimed for the mask, takes the atomicAdds; else the next slot, for at most the region's slot count.  Nothing waits
// for another thread's progress; a probe sequence without room sets the species' overflow flag and drops the class's reads of this wave.  The host then
// reruns the pass for the overflowing species alone (fresh tables of 8 times the slots, every other species switched off) until none overflows: the loop is
// bounded and the result never truncated (read_em_plan.hpp).  Species of more than 64 candidates own no candidate in the pass's table: counted only.
// Walks of more than 64 steps AND their per-group partials into one word per slot; read_class_long_kernel takes a lane per slot and reduces the same way.
// Ordering: occupied slots are flagged, exclusive_scan_u8 ranks them, read_class_gather_kernel writes the dense (slot, mask, Q) arrays; the host downloads
// them (the caller gets them anyway), sorts every species' classes by mask and uploads the ordered (mask, span) for read_em_kernel: one workgroup per
// species with classes; phase D / r strides the threads over the classes, phase R is lane k of ONE wave looping j ascending (the sequential loop is what
// makes every bit reproducible), delta and top by a wave max.  (mask, r) sit in LDS while J fits, else they come from global memory through L2.
//
// Algorithmic bytes of read_class_kernel (T' padded steps, R' slots), route 1: those of read_support_kernel in -- 4T' + 1T' + 8T' + 16R' + 8R'; out: per
// wave and distinct (species, mask) one key probe and three counters.
#include <algorithm>
#include <cmath>
#include "common.hpp"
#include "read_em_plan.hpp"
#include "read_pass_device.hpp"

namespace ptx {

namespace {

enum : uint32_t { RC_OFF = 0, RC_COUNT = 1, RC_CLASSES = 2, RC_RERUN = 3 };   // nothing; counted only; counted, unexplained and classes; classes only
struct RcSpecies {
    uint64_t slot_base;   // first slot of the species' region
    uint64_t slot_mask;   // slots - 1 (slots: a power of two >= 2)
    uint32_t shift;       // 64 - log2(slots): the hash keeps its high bits
    uint32_t mode;
};
struct RcOut {
    unsigned long long *key;   // [slots]
    unsigned long long *cnt;   // [slots][3]
    unsigned long long *sp;    // [S][2][3]  counted, unexplained
    uint32_t *overflow;        // [S]
};

// route 1: haplotype bits -> candidate ranks (monotone: the compressed word sorts as the raw one)
__device__ __forceinline__ unsigned long long rc_rank_bits(unsigned long long m, unsigned long long bits) {
    if ((bits & (bits + 1ull)) == 0ull) return m;   // the chosen haplotypes are 0 .. K-1: rank = index
    unsigned long long out = 0ull;
    for (; m; m &= m - 1ull) out |= 1ull << __popcll(bits & ((1ull << __builtin_ctzll(m)) - 1ull));
    return out;
}
// one class of one wave -> the species' table (one lane calls it; m0 != 0)
__device__ __forceinline__ void rc_file(const RcSpecies &su, uint32_t s0, unsigned long long m0, unsigned long long n, unsigned long long steps,
                                        unsigned long long span, const RcOut &out) {
    uint64_t i = (m0 * 0x9E3779B97F4A7C15ull) >> su.shift;
    for (uint64_t t = 0; t <= su.slot_mask; ++t) {
        unsigned long long *const k = out.key + su.slot_base + i;
        unsigned long long old = __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a key never changes once set)
        if (old == 0ull) old = atomicCAS(k, 0ull, m0);
        if (old == 0ull || old == m0) {
            rs_add3(out.cnt + (su.slot_base + i) * 3u, n, steps, span);
            return;
        }
        i = (i + 1u) & su.slot_mask;
    }
    atomicOr(out.overflow + s0, 1u);
}
// the deciding lanes of the wave -> the counters and the tables, species by species, mask by mask.  All 64 lanes call it.
__device__ __forceinline__ void rc_wave_reduce(int lane, bool decide, uint32_t sp, unsigned long long m, uint32_t steps, uint32_t span,
                                               const RcSpecies *__restrict__ rc, const RcOut &out) {
    rs_species_rounds(decide, sp, [&](uint32_t s0, bool mine, unsigned long long sb) {
        const RcSpecies su = rc[s0];
        if (su.mode == RC_OFF) return;
        if (su.mode != RC_RERUN) rs_reduce_add(lane, mine, sb, steps, span, out.sp + (uint64_t)s0 * 6u);   // counted
        if (su.mode == RC_COUNT) return;
        unsigned long long left = sb;
        while (left) {
            const unsigned long long m0 = lane_get(m, __builtin_ctzll(left));   // the mask of the first lane left
            const bool same = mine && m == m0;
            const unsigned long long cb = __builtin_amdgcn_ballot_w64(same);
            left &= ~cb;
            if (m0 == 0ull && su.mode == RC_RERUN) continue;                 // (unexplained was counted by the first pass)
            const RsQ q = rs_reduce(same, cb, steps, span);
            if (lane == 0) {
                if (m0 == 0ull) rs_add3(out.sp + (uint64_t)s0 * 6u + 3u, q.n, q.steps, q.span);
                else rc_file(su, s0, m0, q.n, q.steps, q.span, out);
            }
        }
    });
}

// every species of the table has at most one mask word (a species of more than 64 candidates is in it without candidates)
__global__ void __launch_bounds__(256) read_class_kernel(uint32_t n_groups, uint32_t n_slots, const uint32_t *__restrict__ group_slot,
                                                         const uint8_t *__restrict__ step_code, const uint32_t *__restrict__ g_node_id,
                                                         const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
                                                         const RsSpecies *__restrict__ tab, const RcSpecies *__restrict__ rc,
                                                         const unsigned long long *__restrict__ node_haps, const unsigned long long *__restrict__ mask,
                                                         unsigned long long *__restrict__ long_acc, RcOut out) {
    const int lane = threadIdx.x & 63;
    for (uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += gridDim.x * 4) {
        const uint32_t gs = group_slot[g];                                   // (wave-uniform) NO_SLOT: a group of pads only
        if (gs == RS_NO_SLOT) continue;
        const RsLane L = rs_lane(g, gs, lane, n_slots, step_code, g_node_id, read_rec, slot_rec, tab);
        const bool decide = L.last && L.counted && !L.is_long;
        const unsigned long long w = rs_lane_word(L, 0u, lane, node_haps, mask);   // (every lane: seg_and wants all 64)
        unsigned long long cm = 0ull;
        if (L.tail && L.nw) {
            if (L.is_long) rs_long_partial(long_acc, 1u, L.slot, 0u, w);
            else if (L.last) cm = L.st.m.route == 1u ? rc_rank_bits(w, L.st.m.bits) : w;
        }
        rc_wave_reduce(lane, decide, L.sr.x, cm, L.rr.y, rs_span(L.rr), rc, out);
    }
}

// walks of more than 64 steps: the AND of their per-group partials, a lane per slot, the same reduction
__global__ void __launch_bounds__(256) read_class_long_kernel(uint32_t n_slots, const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
                                                              const RsSpecies *__restrict__ tab, const RcSpecies *__restrict__ rc,
                                                              const unsigned long long *__restrict__ long_acc, RcOut out) {
    const int lane = threadIdx.x & 63;
    for (uint64_t base = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64u; base < n_slots; base += (uint64_t)gridDim.x * 256u) {   // (wave-uniform)
        const RsLongSlot t = rs_long_slot(base, lane, n_slots, read_rec, slot_rec);
        unsigned long long cm = 0ull;
        if (t.decide) {
            const RsSpecies st = tab[t.sp];
            if (st.m.route) cm = st.m.route == 1u ? rc_rank_bits(long_acc[t.s], st.m.bits) : long_acc[t.s];
        }
        rc_wave_reduce(lane, t.decide, t.sp, cm, t.rr.y, rs_span(t.rr), rc, out);
    }
}

__global__ void __launch_bounds__(256) read_class_flag_kernel(uint64_t n, const unsigned long long *__restrict__ key, uint8_t *__restrict__ flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) flag[i] = key[i] != 0ull ? 1 : 0;
}
// occupied slot i -> dense entry rank[i] (< n_dense by the scan): its slot, its mask, its three sums
__global__ void __launch_bounds__(256) read_class_gather_kernel(uint64_t n, uint32_t n_dense, const unsigned long long *__restrict__ key,
                                                                const unsigned long long *__restrict__ cnt, const uint32_t *__restrict__ rank,
                                                                uint32_t *__restrict__ d_slot, unsigned long long *__restrict__ d_mask,
                                                                unsigned long long *__restrict__ d_q) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const unsigned long long k = key[i];
        if (k == 0ull) continue;
        const uint32_t at = rank[i];
        if (at >= n_dense) continue;
        d_slot[at] = (uint32_t)i;
        d_mask[at] = k;
        d_q[(uint64_t)at * 3u] = cnt[i * 3u]; d_q[(uint64_t)at * 3u + 1u] = cnt[i * 3u + 1u]; d_q[(uint64_t)at * 3u + 2u] = cnt[i * 3u + 2u];
    }
}

// ---- the estimate -------------------------------------------------------------------------------------------------------------------
struct EmSpecies {
    uint64_t cls0;    // first class of the species in the ordered arrays
    uint32_t J, K;    // classes, candidates (1 .. 64)
    uint32_t ent0;    // first candidate of the species (sorted order)
    uint32_t s;       // the species
};
struct EmOut { double *x; uint32_t *iter; int32_t *conv; double *delta; };   // x: [C] in sorted order; the rest per workgroup

// one workgroup per species with classes.  The iteration of the contract: every sum in the stated order, one rounding per operation.
__global__ void __launch_bounds__(256) read_em_kernel(const EmSpecies *__restrict__ sp, const unsigned long long *g_mask, const unsigned long long *__restrict__ g_b,
                                                      const unsigned long long *__restrict__ g_len, double *g_r, uint32_t lds_classes, uint32_t max_iter, double tol,
                                                      EmOut out) {
#pragma clang fp contract(off)
    __shared__ double s_x[64];
    __shared__ double s_r[READ_EM_LDS_CLASSES];
    __shared__ unsigned long long s_m[READ_EM_LDS_CLASSES];
    __shared__ int s_stop;
    const EmSpecies e = sp[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const bool in_lds = e.J <= lds_classes;                                   // (lds_classes <= READ_EM_LDS_CLASSES)
    const unsigned long long *const gb = g_b + e.cls0;
    const unsigned long long *const mp = in_lds ? s_m : g_mask + e.cls0;
    double *const rp = in_lds ? s_r : g_r + e.cls0;
    if (in_lds)
        for (uint32_t j = tid; j < e.J; j += 256u) s_m[j] = g_mask[e.cls0 + j];
    double G = 0.0, x = 0.0;
    bool live = false;
    if (tid < 64u) {
        if (tid < e.K) {
            const unsigned long long len = g_len[e.ent0 + tid];
            live = len > 0ull;
            G = (double)len;
        }
        x = live ? 1.0 : 0.0;
        s_x[tid] = x;
    }
    if (tid == 0u) s_stop = 0;
    uint32_t n_iter = 0u;
    int32_t conv = 0;
    double delta = 0.0;
    __syncthreads();
    for (uint32_t t = 1u; t <= max_iter; ++t) {
        for (uint32_t j = tid; j < e.J; j += 256u) {                          // D_j and r_j
            double D = 0.0;
            for (unsigned long long q = mp[j]; q; q &= q - 1ull) D = __dadd_rn(D, s_x[__builtin_ctzll(q)]);
            rp[j] = D > 0.0 ? (double)gb[j] / D : 0.0;
        }
        __syncthreads();
        if (wave == 0u) {                                                     // R_k, y_k: lane k, j ascending
            double R = 0.0;
            for (uint32_t j = 0u; j < e.J; ++j) {
                const double r = rp[j];
                if ((mp[j] >> lane) & 1ull) R = __dadd_rn(R, r);
            }
            double y = live ? __dmul_rn(x, R) / G : 0.0;
            if (y < 1e-200) y = 0.0;
            const auto mx = [](double a, double b) { return a > b ? a : b; };
            delta = wave_reduce(fabs(y - x), mx);
            const double top = wave_reduce(y, mx);
            x = y;
            s_x[lane] = y;
            n_iter = t;
            if (delta <= __dmul_rn(tol, top)) {
                conv = 1;
                if (lane == 0u) s_stop = 1;
            }
        }
        __syncthreads();
        if (s_stop) break;
    }
    if (wave == 0u) {
        if (lane < e.K) out.x[e.ent0 + lane] = x;
        if (lane == 0u) { out.iter[blockIdx.x] = n_iter; out.conv[blockIdx.x] = conv; out.delta[blockIdx.x] = delta; }
    }
}

struct RcClass { uint64_t mask, q[3]; };

}  // namespace

int read_em_launch(Ctx *ctx, Db *db, Reads *rd, const uint64_t *cand_off, const uint32_t *cand_hap, const uint64_t *cand_len, const uint64_t *entry_of, uint32_t max_iter,
                   double tol, uint64_t *species_out, uint64_t *cls_off_out, uint64_t cls_cap, uint64_t *cls_mask_out, uint64_t *cls_q_out, double *x_out, uint32_t *iter_out,
                   int32_t *converged_out, double *delta_out) {
    const uint32_t S = db->S;
    const uint64_t H = db->H, C = cand_off[S];
    PTX_TRY(rs_check_bits(ctx, "strain_read_em", H, C));
    // the table of the pass: a skipped species (K_s > 64) is in it without candidates -- it is counted, and no mask of it is formed
    std::vector<uint64_t> t_off(S + 1, 0);
    std::vector<uint32_t> t_hap;
    std::vector<uint64_t> K(S ? S : 1, 0), slots(S ? S : 1, 0);
    std::vector<uint32_t> mode(S ? S : 1, RC_COUNT);
    for (uint32_t s = 0; s < S; ++s) {
        K[s] = cand_off[s + 1] - cand_off[s];
        if (K[s] >= 1 && K[s] <= READ_EM_MAX_K) {
            t_hap.insert(t_hap.end(), cand_hap + cand_off[s], cand_hap + cand_off[s + 1]);
            mode[s] = RC_CLASSES;
            slots[s] = read_class_slots(K[s], ctx->cfg.read_class_slots);
        }
        t_off[s + 1] = t_hap.size();
    }
    RsTable rt;
    rs_table_build(ctx, db, t_off.data(), t_hap.data(), rt, [](uint64_t, uint64_t) {});
    std::vector<unsigned long long> h_sp((size_t)(S ? S : 1) * 6, 0ull);
    std::vector<std::vector<RcClass>> cls(S);
    if (S) {
        DevBuf<unsigned long long> d_sp, d_tabs, d_dmask, d_dq;
        RsLongAcc lng;
        DevBuf<RsSpecies> d_tab;
        DevBuf<RcSpecies> d_rc;
        DevBuf<uint32_t> d_over, d_rank, d_tmp, d_tot, d_dslot;
        DevBuf<uint8_t> d_flag;
        PTX_HIP(ctx, d_sp.alloc((size_t)S * 6));
        PTX_TRY(zero_fill(ctx, d_sp.p, (size_t)S * 6 * sizeof(unsigned long long)));
        PTX_HIP(ctx, d_over.alloc(S));
        PTX_HIP(ctx, d_tot.alloc(1));
        PTX_TRY(upload(ctx, d_tab, rt.tab.data(), rt.tab.size()));
        PTX_TRY(rt.wm.build(ctx, db));
        PTX_TRY(lng.init(ctx, rd, 1u));   // (a rerun ANDs the same partials in again)
        std::vector<RcSpecies> rc(S);
        std::vector<uint64_t> slot_off(S + 1, 0);
        std::vector<uint32_t> h_over(S, 0), h_dslot;
        std::vector<unsigned long long> h_dmask, h_dq;
        for (bool first = true;; first = false) {
            for (uint32_t s = 0; s < S; ++s) {
                const uint64_t n = (mode[s] == RC_CLASSES || mode[s] == RC_RERUN) ? slots[s] : 0;
                uint32_t lg = 0;
                while ((1ull << lg) < n) ++lg;
                rc[s] = RcSpecies{slot_off[s], n ? n - 1 : 0, 64u - (lg ? lg : 1u), mode[s]};
                slot_off[s + 1] = slot_off[s] + n;
            }
            const uint64_t total = slot_off[S];
            if (total >= 0xFFFFFFFFull)
                return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_read_em: %llu class table slots exceed 32-bit positions (option read_class_slots)", (unsigned long long)total);
            // one device block, zero-filled once: [key total][counters total x 3]
            PTX_HIP(ctx, d_tabs.alloc((size_t)(total ? total : 1) * 4));
            PTX_TRY(zero_fill(ctx, d_tabs.p, (size_t)(total ? total : 1) * 4 * sizeof(unsigned long long)));
            PTX_TRY(zero_fill(ctx, d_over.p, (size_t)S * sizeof(uint32_t)));
            PTX_TRY(upload(ctx, d_rc, rc.data(), rc.size()));
            const RcOut out{d_tabs.p, d_tabs.p + (total ? total : 1), d_sp.p, d_over.p};
            rs_launch_groups(ctx, rd, "read_class_kernel", read_class_kernel, d_tab.p, d_rc.p, rs_node_haps(rt, db), rt.wm.d_mask.p, lng.d_acc.p, out);
            rs_launch_slots(ctx, rd, "read_class_long_kernel", read_class_long_kernel, d_tab.p, d_rc.p, lng.d_acc.p, out);
            PTX_HIP(ctx, hipGetLastError());
            uint32_t n_dense = 0;
            if (total) {
                PTX_HIP(ctx, d_flag.alloc(total));
                PTX_HIP(ctx, d_rank.alloc(total));
                PTX_HIP(ctx, d_tmp.alloc(scan_tmp_elems(total)));
                {
                    KTimer tm(ctx, "read_class_flag_kernel");
                    hipLaunchKernelGGL(read_class_flag_kernel, dim3(grid_for(total, 256, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, total, d_tabs.p, d_flag.p);
                }
                PTX_TRY(exclusive_scan_u8(ctx, d_flag.p, d_rank.p, total, d_tmp.p, d_tot.p));
                PTX_TRY(download(ctx, &n_dense, d_tot.p, 1));
            }
            PTX_TRY(download(ctx, h_over.data(), d_over.p, S));
            if (first) PTX_TRY(download(ctx, h_sp.data(), d_sp.p, (size_t)S * 6));
            PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (n_dense) {
                PTX_HIP(ctx, d_dslot.alloc(n_dense));
                PTX_HIP(ctx, d_dmask.alloc(n_dense));
                PTX_HIP(ctx, d_dq.alloc((size_t)n_dense * 3));
                {
                    KTimer tm(ctx, "read_class_gather_kernel");
                    hipLaunchKernelGGL(read_class_gather_kernel, dim3(grid_for(total, 256, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, total, n_dense, d_tabs.p,
                                       d_tabs.p + total, d_rank.p, d_dslot.p, d_dmask.p, d_dq.p);
                }
                PTX_HIP(ctx, hipGetLastError());
                h_dslot.resize(n_dense); h_dmask.resize(n_dense); h_dq.resize((size_t)n_dense * 3);
                PTX_TRY(download(ctx, h_dslot.data(), d_dslot.p, n_dense));
                PTX_TRY(download(ctx, h_dmask.data(), d_dmask.p, n_dense));
                PTX_TRY(download(ctx, h_dq.data(), d_dq.p, (size_t)n_dense * 3));
                PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
            }
            // the dense entries are in slot order, so species after species; those of a species that overflowed are dropped with its table
            uint32_t s = 0;
            for (uint32_t i = 0; i < n_dense; ++i) {
                while (s < S && h_dslot[i] >= slot_off[s + 1]) ++s;
                if (s >= S) return fail(ctx, PANTAX_HIP_E_HIP, "strain_read_em: internal: a class in slot %u of %llu", h_dslot[i], (unsigned long long)total);
                if (!h_over[s]) cls[s].push_back(RcClass{h_dmask[i], {h_dq[(size_t)i * 3], h_dq[(size_t)i * 3 + 1], h_dq[(size_t)i * 3 + 2]}});
            }
            bool again = false;
            for (s = 0; s < S; ++s) {
                if (!h_over[s]) { mode[s] = RC_OFF; slots[s] = 0; continue; }
                const uint64_t next = read_class_grow(slots[s], K[s], h_sp[(size_t)s * 6]);
                if (next <= slots[s])
                    return fail(ctx, PANTAX_HIP_E_HIP, "strain_read_em: internal: the class table of species %u overflowed at %llu slots, its bound", s, (unsigned long long)slots[s]);
                slots[s] = next;
                mode[s] = RC_RERUN;
                again = true;
            }
            if (!again) break;
        }
    }
    // every species' classes in ascending mask
    std::vector<uint64_t> cls_off(S + 1, 0);
    for (uint32_t s = 0; s < S; ++s) {
        std::sort(cls[s].begin(), cls[s].end(), [](const RcClass &a, const RcClass &b) { return a.mask < b.mask; });
        cls_off[s + 1] = cls_off[s] + cls[s].size();
    }
    const uint64_t J_all = cls_off[S];
    for (uint32_t s = 0; s <= S; ++s) cls_off_out[s] = cls_off[s];
    if (cls_cap && J_all > cls_cap)
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_read_em: %llu classes, the caller's arrays hold %llu", (unsigned long long)J_all, (unsigned long long)cls_cap);
    // the estimate: one workgroup per species with classes, over the ordered (mask, span)
    std::vector<EmSpecies> em;
    std::vector<unsigned long long> h_mask(J_all ? J_all : 1), h_b(J_all ? J_all : 1), h_len(C ? C : 1);
    for (uint64_t c = 0; c < C; ++c) h_len[c] = cand_len[c];
    uint64_t j_max = 0;
    for (uint32_t s = 0; s < S; ++s) {
        for (size_t j = 0; j < cls[s].size(); ++j) { h_mask[cls_off[s] + j] = cls[s][j].mask; h_b[cls_off[s] + j] = cls[s][j].q[2]; }
        if (cls[s].empty()) continue;
        if (cls[s].size() > 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_read_em: species %u has %llu classes", s, (unsigned long long)cls[s].size());
        em.push_back(EmSpecies{cls_off[s], (uint32_t)cls[s].size(), (uint32_t)K[s], (uint32_t)cand_off[s], s});
        j_max = std::max<uint64_t>(j_max, cls[s].size());
    }
    std::vector<double> h_x(C ? C : 1, 0.0), h_delta(em.size() ? em.size() : 1, 0.0);
    std::vector<uint32_t> h_iter(em.size() ? em.size() : 1, 0);
    std::vector<int32_t> h_conv(em.size() ? em.size() : 1, 0);
    if (!em.empty()) {
        DevBuf<EmSpecies> d_em;
        DevBuf<unsigned long long> d_mask, d_b, d_len;
        DevBuf<double> d_r, d_x, d_delta;
        DevBuf<uint32_t> d_iter;
        DevBuf<int32_t> d_conv;
        PTX_TRY(upload(ctx, d_em, em.data(), em.size()));
        PTX_TRY(upload(ctx, d_mask, h_mask.data(), h_mask.size()));
        PTX_TRY(upload(ctx, d_b, h_b.data(), h_b.size()));
        PTX_TRY(upload(ctx, d_len, h_len.data(), h_len.size()));
        uint32_t lds_classes = READ_EM_LDS_CLASSES;
        if (ctx->cfg.read_em_lds_classes > 0) lds_classes = std::min<uint32_t>((uint32_t)ctx->cfg.read_em_lds_classes, READ_EM_LDS_CLASSES);
        PTX_HIP(ctx, d_r.alloc(j_max > lds_classes ? (size_t)J_all : 1));      // r of the species that do not fit LDS
        PTX_HIP(ctx, d_x.alloc(h_x.size()));
        PTX_TRY(zero_fill(ctx, d_x.p, h_x.size() * sizeof(double)));
        PTX_HIP(ctx, d_delta.alloc(em.size())); PTX_HIP(ctx, d_iter.alloc(em.size())); PTX_HIP(ctx, d_conv.alloc(em.size()));
        {
            KTimer tm(ctx, "read_em_kernel");
            hipLaunchKernelGGL(read_em_kernel, dim3((uint32_t)em.size()), dim3(256), 0, ctx->stream, d_em.p, d_mask.p, d_b.p, d_len.p, d_r.p, lds_classes, max_iter, tol,
                               EmOut{d_x.p, d_iter.p, d_conv.p, d_delta.p});
        }
        PTX_HIP(ctx, hipGetLastError());
        PTX_TRY(download(ctx, h_x.data(), d_x.p, h_x.size()));
        PTX_TRY(download(ctx, h_iter.data(), d_iter.p, em.size()));
        PTX_TRY(download(ctx, h_conv.data(), d_conv.p, em.size()));
        PTX_TRY(download(ctx, h_delta.data(), d_delta.p, em.size()));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host arrays are filled, the temporaries are released on return
    }
    // nothing has failed: the caller's arrays
    for (size_t i = 0; i < (size_t)S * 6; ++i) species_out[i] = h_sp[i];
    if (cls_cap)
        for (uint32_t s = 0; s < S; ++s)
            for (size_t j = 0; j < cls[s].size(); ++j) {
                cls_mask_out[cls_off[s] + j] = cls[s][j].mask;
                for (int q = 0; q < 3; ++q) cls_q_out[(cls_off[s] + j) * 3 + q] = cls[s][j].q[q];
            }
    for (uint64_t c = 0; c < C; ++c) x_out[entry_of[c]] = h_x[c];
    for (uint32_t s = 0; s < S; ++s) { iter_out[s] = 0; converged_out[s] = 0; delta_out[s] = 0.0; }
    for (size_t i = 0; i < em.size(); ++i) { iter_out[em[i].s] = h_iter[i]; converged_out[em[i].s] = h_conv[i]; delta_out[em[i].s] = h_delta[i]; }
    return 0;
}

}  // namespace ptx
