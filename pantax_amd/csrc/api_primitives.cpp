// api_primitives.cpp -- pantax_hip_scan / pantax_hip_radix_sort / pantax_hip_fill: the device primitives of primitives.hpp behind host-buffer
// entry points, as pantax_hip_sort_rows (api_sort.cpp) is for the row sorts.  They exist so that the tests can pin the chained scan, the LSD
// radix sort and byte_fill against numpy at every shape the product runs them at: all three upload, run on ctx->stream, download and synchronise.
#include <vector>
#include "primitives.hpp"
#include "scan_chained.hpp"

using namespace ptx;

extern "C" int pantax_hip_scan(pantax_hip_ctx *ctx, uint64_t n, const void *in, int item_bytes, int in_place, uint32_t *out, uint32_t *total_out,
                               uint32_t *tile_items_out) {
    if (!ctx || (n && (!in || !out)) || (item_bytes != 1 && item_bytes != 4)) return PANTAX_HIP_E_INVALID;
    PTX_ENTER(ctx);
    if (in_place && item_bytes != 4) return fail(ctx, PANTAX_HIP_E_INVALID, "scan: only 4-byte items are scanned in place");
    const uint32_t tile = scan_tile_items(ctx->cfg, n);   // what exclusive_scan_fn launches with (0: it fails, naming the option)
    DevBuf<uint8_t> d_in8;
    DevBuf<uint32_t> d_in32, d_out, d_tot, tmp;
    PTX_HIP(ctx, d_out.alloc(n)); PTX_HIP(ctx, d_tot.alloc(1)); PTX_HIP(ctx, tmp.alloc(scan_tmp_elems(n)));
    if (item_bytes == 1) {
        PTX_TRY(upload(ctx, d_in8, static_cast<const uint8_t *>(in), n));
        PTX_TRY(exclusive_scan_u8(ctx, d_in8.p, d_out.p, n, tmp.p, d_tot.p));
    } else {
        DevBuf<uint32_t> &src = in_place ? d_out : d_in32;   // in place: d_in == d_out (a tile's loads happen before its stores)
        PTX_TRY(upload(ctx, src, static_cast<const uint32_t *>(in), n));
        PTX_TRY(exclusive_scan_u32(ctx, src.p, d_out.p, n, tmp.p, d_tot.p));
    }
    uint32_t tot = 0;
    PTX_TRY(download(ctx, out, d_out.p, n));
    PTX_TRY(download(ctx, &tot, d_tot.p, 1));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (total_out) *total_out = tot;
    if (tile_items_out) *tile_items_out = tile;
    return 0;
}

extern "C" int pantax_hip_radix_sort(pantax_hip_ctx *ctx, uint64_t n, uint64_t n_actual, int nw, uint64_t *k0, uint64_t *k1, uint64_t *k2, uint32_t *payload,
                                     const int32_t *pass_word, const int32_t *pass_shift, int n_passes, int *result_in_b_out) {
    if (!ctx || nw < 1 || nw > SORT_MAX_WORDS || n_passes < 0 || (n_passes && (!pass_word || !pass_shift))) return PANTAX_HIP_E_INVALID;
    uint64_t *h[SORT_MAX_WORDS] = {k0, k1, k2};
    for (int w = 0; w < nw; ++w) if (n && !h[w]) return PANTAX_HIP_E_INVALID;
    PTX_ENTER(ctx);
    if (n_actual > n) return fail(ctx, PANTAX_HIP_E_INVALID, "radix_sort: n_actual %llu exceeds n %llu", (unsigned long long)n_actual, (unsigned long long)n);
    if (n >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "radix_sort: %llu records exceed 32-bit positions", (unsigned long long)n);
    std::vector<SortPass> passes;
    for (int p = 0; p < n_passes; ++p) {
        if (pass_word[p] < 0 || pass_word[p] >= nw || pass_shift[p] < 0 || pass_shift[p] > 63)
            return fail(ctx, PANTAX_HIP_E_INVALID, "radix_sort: pass %d reads word %d at shift %d of %d-word keys", p, pass_word[p], pass_shift[p], nw);
        passes.push_back({pass_word[p], pass_shift[p]});
    }
    if (result_in_b_out) *result_in_b_out = 0;
    if (n == 0) return 0;
    DevBuf<uint64_t> a[SORT_MAX_WORDS], b[SORT_MAX_WORDS];
    DevBuf<uint32_t> va, vb, table, tmp, dn;
    SortBufs A, B;
    A.nw = B.nw = nw;
    // both sides start as the caller's records: whatever a pass leaves alone -- everything from n_actual on -- reads as it went in, on either side
    for (int w = 0; w < nw; ++w) {
        PTX_TRY(upload(ctx, a[w], h[w], n)); PTX_TRY(upload(ctx, b[w], h[w], n));
        A.k[w] = a[w].p; B.k[w] = b[w].p;
    }
    if (payload) {
        PTX_TRY(upload(ctx, va, payload, n)); PTX_TRY(upload(ctx, vb, payload, n));
        A.v = va.p; B.v = vb.p;
    }
    const uint32_t n32 = (uint32_t)n_actual;
    PTX_TRY(upload(ctx, dn, &n32, 1));
    PTX_HIP(ctx, table.alloc(sort_table_elems(n))); PTX_HIP(ctx, tmp.alloc(scan_tmp_elems(n)));
    bool in_b = false;
    PTX_TRY(radix_sort(ctx, A, B, n, passes.data(), (int)passes.size(), table.p, tmp.p, &in_b, dn.p));
    const SortBufs &R = in_b ? B : A;
    for (int w = 0; w < nw; ++w) PTX_TRY(download(ctx, h[w], R.k[w], n));
    if (payload) PTX_TRY(download(ctx, payload, R.v, n));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (result_in_b_out) *result_in_b_out = in_b ? 1 : 0;
    return 0;
}

extern "C" int pantax_hip_fill(pantax_hip_ctx *ctx, uint64_t buf_bytes, int sentinel, uint64_t off, uint64_t bytes, int byte, uint8_t *out) {
    if (!ctx || (buf_bytes && !out)) return PANTAX_HIP_E_INVALID;
    PTX_ENTER(ctx);
    if (off > buf_bytes || bytes > buf_bytes - off)
        return fail(ctx, PANTAX_HIP_E_INVALID, "fill: [%llu, +%llu) leaves the buffer of %llu bytes", (unsigned long long)off, (unsigned long long)bytes, (unsigned long long)buf_bytes);
    if (buf_bytes == 0) return 0;
    DevBuf<uint8_t> buf;
    PTX_HIP(ctx, buf.alloc(buf_bytes));
    PTX_HIP(ctx, hipMemsetAsync(buf.p, sentinel & 0xFF, buf_bytes, ctx->stream));
    PTX_TRY(byte_fill(ctx, buf.p + off, byte, bytes));
    PTX_HIP(ctx, hipGetLastError());
    PTX_TRY(download(ctx, out, buf.p, buf_bytes));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
