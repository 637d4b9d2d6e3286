// stage_read_strain.hip -- per-read strain assignment (pantax_hip_read_strains, the --read-strains report): which candidate strain of its
// species every read supports.  Not a stage of the reference; it answers, on data the strain step leaves in HBM, what a user of
// the tables would otherwise re-derive on the host from the graph files.
//
// Contract (DESIGN.md "Per-read strain assignment"):
//   N(r) = the distinct nodes of the walk of read r (order and orientation ignored: the node-level model of the LP, profile.rs:1333-1342);
//   C(r) = the candidates of r's species whose walk visits every node of N(r);
//   assigned strain = argmax of the weight over C(r), ties to the smallest species-local haplotype index;
//   posterior = w_assigned / sum of w over C(r), summed in f64 in ascending haplotype index;  n = |C(r)|.
// Only reads the coverage pass counts (slot species >= 0) are assigned; reads binned to a species of the db but dropped (flags,
// duplicate-id rule) and reads of species without candidates come out as "not counted" (n = -1).
//
// Membership of a node in the candidates' walks, as one mask per node (W_s words on route 2): the two routes of member_plan.hpp, option read_strain_route.
// read_strain_kernel walks the locus-grouped stream of the coverage pass (build_step_read, stage_read_layout.hip): a wave per 64-step group,
// a lane per step.  The AND of the masks over a walk's steps is a segmented scan over the lanes on the DPP path; walks of <= 64 steps
// never straddle a group, so the lane of the last step holds the walk's AND and decides there.  Walks of more than 64 steps (long
// reads) AND their per-group partials into a per-slot word set to all ones first (64-bit atomic AND), and read_strain_long_kernel
// decides them.  read_strain_gather_kernel brings the per-slot results into file order through Reads::d_slot_of.
//
// Algorithmic bytes of read_strain_kernel (T' padded steps, R' slots):
//   4T' (node ids) + 1T' (step codes) + 8T' (mask words, route 1) + 16R' (read records) + 8R' (slot records) + 16R' (results)
#include <algorithm>
#include <cmath>
#include "common.hpp"
#include "read_pass_device.hpp"
#include "wave.hpp"

namespace ptx {

namespace {

struct RsResult { uint32_t hap; int32_t n; double post; };

// the candidates of one mask word, ascending: count, sum (f64, in order), argmax (first of equal weights)
__device__ __forceinline__ void rs_take(unsigned long long m, uint32_t w, const double *__restrict__ bit_w, uint32_t bit_base, double &best,
                                        uint32_t &besti, double &sum, int &n) {
    while (m) {
        const uint32_t idx = w * 64u + (uint32_t)__builtin_ctzll(m);
        m &= m - 1ull;
        const double x = bit_w[bit_base + idx];
        ++n;
        sum += x;
        if (x > best) { best = x; besti = idx; }
    }
}
__device__ __forceinline__ RsResult rs_finish(const RsSpecies &st, const uint32_t *__restrict__ bit_hap, double best, uint32_t besti, double sum, int n) {
    RsResult o;
    if (st.m.route == 0) { o.hap = 0xFFFFFFFFu; o.n = -1; o.post = 0.0; }
    else if (n == 0) { o.hap = 0xFFFFFFFFu; o.n = 0; o.post = 0.0; }
    else { o.hap = bit_hap[st.bit_base + besti]; o.n = n; o.post = best / sum; }
    return o;
}

__global__ void __launch_bounds__(256) read_strain_kernel(uint32_t n_groups, uint32_t n_slots, const uint32_t *__restrict__ group_slot,
                                                          const uint8_t *__restrict__ step_code, const uint32_t *__restrict__ g_node_id,
                                                          const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
                                                          const RsSpecies *__restrict__ tab, const unsigned long long *__restrict__ node_haps,
                                                          const unsigned long long *__restrict__ mask, const double *__restrict__ bit_w,
                                                          const uint32_t *__restrict__ bit_hap, unsigned long long *__restrict__ long_acc, uint32_t long_nw,
                                                          RsResult *__restrict__ res) {
    const int lane = threadIdx.x & 63;
    for (uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += gridDim.x * 4) {
        const uint32_t gs = group_slot[g];                                   // (wave-uniform) NO_SLOT: a group of pads only
        if (gs == RS_NO_SLOT) continue;
        const RsLane L = rs_lane(g, gs, lane, n_slots, step_code, g_node_id, read_rec, slot_rec, tab);
        const uint32_t nw_max = wave_reduce(L.nw, [](uint32_t x, uint32_t y) { return x > y ? x : y; });
        double best = -INFINITY, sum = 0.0;
        uint32_t besti = 0;
        int n = 0;
        for (uint32_t w = 0; w < nw_max; ++w) {                              // (wave-uniform trip count: seg_and wants every lane)
            const unsigned long long m = rs_lane_word(L, w, lane, node_haps, mask);
            if (L.tail && w < L.nw) {
                if (L.is_long) rs_long_partial(long_acc, long_nw, L.slot, w, m);
                else if (L.last) rs_take(m, w, bit_w, L.st.bit_base, best, besti, sum, n);
            }
        }
        if (L.last && L.counted && !L.is_long) res[L.slot] = rs_finish(L.st, bit_hap, best, besti, sum, n);
    }
}

// walks of more than 64 steps: the AND of their per-group partials -> the decision
__global__ void __launch_bounds__(256) read_strain_long_kernel(uint32_t n_slots, const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
                                                               const RsSpecies *__restrict__ tab, const unsigned long long *__restrict__ long_acc,
                                                               uint32_t long_nw, const double *__restrict__ bit_w, const uint32_t *__restrict__ bit_hap,
                                                               RsResult *__restrict__ res) {
    for (uint32_t s = blockIdx.x * 256 + threadIdx.x; s < n_slots; s += gridDim.x * 256) {
        if (read_rec[s].y <= 64u) continue;
        const int32_t sp = (int32_t)slot_rec[s].x;
        if (sp < 0) continue;
        const RsSpecies st = tab[sp];
        double best = -INFINITY, sum = 0.0;
        uint32_t besti = 0;
        int n = 0;
        if (st.m.route)
            for (uint32_t w = 0; w < st.m.nw; ++w) rs_take(long_acc[(uint64_t)s * long_nw + w], w, bit_w, st.bit_base, best, besti, sum, n);
        res[s] = rs_finish(st, bit_hap, best, besti, sum, n);
    }
}

// file order: reads binned to a species of the db (counted: their slot's result; dropped: "not counted"); every other entry is left alone
__global__ void __launch_bounds__(256) read_strain_gather_kernel(uint64_t R, const uint32_t *__restrict__ slot_of, const uint2 *__restrict__ slot_rec,
                                                                 const RsResult *__restrict__ res, uint32_t *__restrict__ hap_out, int32_t *__restrict__ n_out,
                                                                 double *__restrict__ post_out) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 256) {
        const uint32_t s = slot_of[r];
        if (s == RS_NO_SLOT) continue;
        const int32_t x = (int32_t)slot_rec[s].x;
        if (x == -1) continue;                                                // "U" against this db
        if (x < -1) { hap_out[r] = 0xFFFFFFFFu; n_out[r] = -1; post_out[r] = 0.0; continue; }
        const RsResult o = res[s];
        hap_out[r] = o.hap; n_out[r] = o.n; post_out[r] = o.post;
    }
}

}  // namespace

int read_strains_launch(Ctx *ctx, Db *db, Reads *rd, const uint64_t *cand_off, const uint32_t *cand_hap, const double *cand_w, uint32_t *hap_out,
                        int32_t *n_out, double *post_out) {
    const uint32_t S = db->S;
    const uint64_t H = db->H, C = cand_off[S];
    PTX_TRY(rs_check_bits(ctx, "read_strains", H, C));
    std::vector<double> bit_w(H + C + 1, 0.0);
    std::vector<uint32_t> bit_hap(H + C + 1, 0u);
    RsTable rt;
    rs_table_build(ctx, db, cand_off, cand_hap, rt, [&](uint64_t at, uint64_t c) { bit_w[at] = cand_w[c]; bit_hap[at] = cand_hap[c]; });
    DevBuf<RsSpecies> d_tab;
    DevBuf<double> d_bit_w;
    DevBuf<uint32_t> d_bit_hap;
    DevBuf<RsResult> d_res;
    RsLongAcc lng;
    PTX_TRY(upload(ctx, d_tab, rt.tab.data(), rt.tab.size()));
    PTX_TRY(upload(ctx, d_bit_w, bit_w.data(), bit_w.size()));
    PTX_TRY(upload(ctx, d_bit_hap, bit_hap.data(), bit_hap.size()));
    PTX_TRY(rt.wm.build(ctx, db));
    PTX_HIP(ctx, d_res.alloc(rd->n_slots ? rd->n_slots : 1));
    PTX_TRY(lng.init(ctx, rd, rt.long_nw));
    rs_launch_groups(ctx, rd, "read_strain_kernel", read_strain_kernel, d_tab.p, rs_node_haps(rt, db), rt.wm.d_mask.p, d_bit_w.p, d_bit_hap.p, lng.d_acc.p, rt.long_nw,
                     d_res.p);
    rs_launch_slots(ctx, rd, "read_strain_long_kernel", read_strain_long_kernel, d_tab.p, lng.d_acc.p, rt.long_nw, d_bit_w.p, d_bit_hap.p, d_res.p);
    const uint64_t R = rd->R;
    if (R) {
        // the caller's arrays travel up first: entries of reads outside this db's species keep what the caller put there
        DevBuf<uint32_t> d_hap;
        DevBuf<int32_t> d_n;
        DevBuf<double> d_post;
        PTX_TRY(upload(ctx, d_hap, hap_out, R));
        PTX_TRY(upload(ctx, d_n, n_out, R));
        PTX_TRY(upload(ctx, d_post, post_out, R));
        {
            KTimer tm(ctx, "read_strain_gather_kernel");
            hipLaunchKernelGGL(read_strain_gather_kernel, dim3(grid_for(R, 256, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, R, rd->d_slot_of.p, rd->d_g_slot_rec.p,
                               d_res.p, d_hap.p, d_n.p, d_post.p);
        }
        PTX_TRY(download(ctx, hap_out, d_hap.p, R));
        PTX_TRY(download(ctx, n_out, d_n.p, R));
        PTX_TRY(download(ctx, post_out, d_post.p, R));
    }
    PTX_HIP(ctx, hipGetLastError());
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host arrays are filled, the temporaries are released on return
    return 0;
}

}  // namespace ptx
