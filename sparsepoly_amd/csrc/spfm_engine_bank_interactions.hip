// spfm_engine_bank_interactions.hip -- spfm_bank_interaction_hist / _list / _counts
// (include/spfm.h): which feature pairs the members of the resident bank agree on.  Per pair the
// number of members that kept it, the number that kept it with a positive weight and the sum of
// the kept weights, formed tile by tile in registers from the bank image itself
// (spfm_bank_interactions.hip.h); no member's W and nothing of size d^2 or d_u x S is stored.
// Read-only views of the bank: scratch of their own, freed with the bank.  See DESIGN.md section 24.
#include "spfm_engine.hip.h"
#include "spfm_bank_interactions.hip.h"
#include "spfm_interactions_host.h"

#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

static_assert(kBiMaxModels == SPFM_BANK_MAX_MODELS, "a member per bit of a tile row's mask");
static_assert(sizeof(BiVal) == 16, "payload of the sorted list");

void spfm_engine::bank_interaction_release() {
    for (DevBuf* b : {&bi_flag, &bi_pos, &bi_ids, &bi_tot, &bi_tmp, &bi_mask, &bi_hist, &bi_cnt,
                      &bi_keys, &bi_vals, &bi_keys2, &bi_vals2, &bi_io, &bi_out})
        b->release();
    bi_du = bi_T = 0;
}

// the checks every entry shares, then the union compaction of the view: bi_ids, bi_du, bi_T and
// the member masks of the tile rows; *a = the arguments of a pass
int spfm_engine::bank_interaction_prepare(const char* what, int block, int32_t d_view, double tol,
                                          int64_t tile_budget, bool compact, BiArgs* a) {
    const std::string w(what);
    if (!bk_have) FAIL(SPFM_ERR_INVALID, w + ": no bank set (spfm_bank_set)");
    if (block < 0 || block >= bk_blocks) FAIL(SPFM_ERR_INVALID, w + ": bad block index");
    if (bk_degree[block] != 2 && bk_degree[block] != -1) {
        char buf[160];
        snprintf(buf, sizeof buf, "%s: block %d has degree %d; pairwise weights are defined for a "
                 "degree-2 block and for all-subsets members", what, block, bk_degree[block]);
        FAIL(SPFM_ERR_UNSUPPORTED, buf);
    }
    if (!(tol >= 0.0)) FAIL(SPFM_ERR_INVALID, w + ": tol must be >= 0");
    if (d_view < 1 || d_view > bk_d) FAIL(SPFM_ERR_INVALID, w + ": d_view must be in [1, d]");
    if (tile_budget < 0) FAIL(SPFM_ERR_INVALID, w + ": tile_budget must be >= 0");
    memset(a, 0, sizeof *a);
    a->pt = bk_pt.as<double>() + (size_t)block * bk_d * bk_S;
    a->lams = bk_lams.as<double>();
    a->koff = bk_koff.as<int32_t>();
    a->S = bk_S;
    a->F = bk_F;
    a->tol = tol;
    if (!compact) return SPFM_OK;
    const int d = bk_d;
    const unsigned nb = cdiv(d, kBlock);
    HIPC(bi_flag.alloc(sizeof(int32_t) * (size_t)d));
    HIPC(bi_pos.alloc(sizeof(int32_t) * (size_t)d));
    HIPC(bi_ids.alloc(sizeof(int32_t) * (size_t)d));
    HIPC(bi_tot.alloc(sizeof(int32_t) * 4));
    // a feature is active when any of the S stacked components is non-zero: the flag kernel of
    // the one-model unit over the image's strides (component stride 1, feature stride S)
    hipLaunchKernelGGL(int_flag_kernel, dim3(nb), dim3(kBlock), 0, stream, a->pt, (int64_t)1,
                       (int64_t)bk_S, bk_S, d, (int)d_view, bi_flag.as<int32_t>());
    size_t temp_bytes = 0;
    HIPC(rocprim::exclusive_scan(nullptr, temp_bytes, bi_flag.as<int32_t>(),
                                 bi_pos.as<int32_t>(), (int32_t)0, (size_t)d,
                                 rocprim::plus<int32_t>(), stream));
    HIPC(bi_tmp.alloc(temp_bytes));
    HIPC(rocprim::exclusive_scan(bi_tmp.p, temp_bytes, bi_flag.as<int32_t>(),
                                 bi_pos.as<int32_t>(), (int32_t)0, (size_t)d,
                                 rocprim::plus<int32_t>(), stream));
    hipLaunchKernelGGL(int_compact_kernel, dim3(nb), dim3(kBlock), 0, stream,
                       bi_flag.as<int32_t>(), bi_pos.as<int32_t>(), d, bi_ids.as<int32_t>(),
                       bi_tot.as<int32_t>());
    HIPC(hipGetLastError());
    int32_t du = 0;
    SPFM_TRY(download(&du, bi_tot.p, 1));
    SPFM_TRY(sync());
    if (du < 0 || du > d_view) FAIL(SPFM_ERR_RUNTIME, w + ": compaction failed");
    bi_du = du;
    bi_T = (int)cdiv(du, kIntTile);
    a->ids = bi_ids.as<int32_t>();
    a->du = du;
    a->T = bi_T;
    if (du < 2) return SPFM_OK;  // no pair
    HIPC(bi_mask.alloc(sizeof(uint64_t) * (size_t)bi_T));
    hipLaunchKernelGGL(bi_mask_kernel, dim3(bi_T), dim3(kBlock), 0, stream, a->pt, bk_S, bk_F,
                       a->koff, a->ids, du, bi_mask.as<unsigned long long>());
    HIPC(hipGetLastError());
    a->mask = bi_mask.as<unsigned long long>();
    return SPFM_OK;
}

// every tile of the union in `mode`, at most `tile_budget` of them per launch (0: a window of the
// one-model unit)
int spfm_engine::bank_interaction_run(int mode, BiArgs a, int64_t tile_budget) {
    const int64_t total = (int64_t)bi_T * (bi_T + 1) / 2;
    const int64_t per = tile_budget > 0 ? tile_budget : kIntWindow;
    bk_launches = 0;
    for (int64_t t0 = 0; t0 < total; t0 += per) {
        a.tile0 = t0;
        const unsigned n = (unsigned)std::min<int64_t>(per, total - t0);
        if (mode == BI_HIST)
            hipLaunchKernelGGL((bi_tile_kernel<BI_HIST>), dim3(n), dim3(kBlock), 0, stream, a);
        else
            hipLaunchKernelGGL((bi_tile_kernel<BI_EMIT>), dim3(n), dim3(kBlock), 0, stream, a);
        ++bk_launches;
    }
    HIPC(hipGetLastError());
    return SPFM_OK;
}

int spfm_engine::bank_interaction_hist(int block, int32_t d_view, double tol, int64_t tile_budget,
                                       int64_t* hist, int64_t* per_member) {
    if (!hist || !per_member) FAIL(SPFM_ERR_INVALID, "bank_interaction_hist: NULL output");
    BiArgs a;
    SPFM_TRY(bank_interaction_prepare("bank_interaction_hist", block, d_view, tol, tile_budget,
                                      true, &a));
    const int F = bk_F;
    std::vector<uint64_t> hh((size_t)2 * F + 1, 0);
    if (bi_du >= 2) {
        HIPC(bi_hist.alloc(sizeof(uint64_t) * hh.size()));
        HIPC(hipMemsetAsync(bi_hist.p, 0, sizeof(uint64_t) * hh.size(), stream));
        a.hist = bi_hist.as<unsigned long long>();
        SPFM_TRY(bank_interaction_run(BI_HIST, a, tile_budget));
        SPFM_TRY(download(hh.data(), bi_hist.p, hh.size()));
        SPFM_TRY(sync());
    }
    int64_t rest = 0;
    for (int c = 1; c <= F; ++c) rest += (hist[c] = (int64_t)hh[(size_t)c]);
    hist[0] = (int64_t)d_view * (d_view - 1) / 2 - rest;
    for (int f = 0; f < F; ++f) per_member[f] = (int64_t)hh[(size_t)F + 1 + f];
    return SPFM_OK;
}

int spfm_engine::bank_interaction_list(int block, int32_t d_view, double tol, int min_count,
                                       int64_t tile_budget, int64_t capacity, int32_t* rows,
                                       int32_t* cols, int32_t* count, int32_t* n_pos, double* sum,
                                       int64_t* n_out) {
    if (!n_out) FAIL(SPFM_ERR_INVALID, "bank_interaction_list: n_out is NULL");
    *n_out = 0;
    if (capacity < 0) FAIL(SPFM_ERR_INVALID, "bank_interaction_list: capacity must be >= 0");
    if (capacity > 0 && (!rows || !cols || !count || !n_pos || !sum))
        FAIL(SPFM_ERR_INVALID, "bank_interaction_list: NULL output");
    if (bk_have && (min_count < 1 || min_count > bk_F))
        FAIL(SPFM_ERR_INVALID, "bank_interaction_list: min_count must be in [1, F]");
    BiArgs a;
    SPFM_TRY(bank_interaction_prepare("bank_interaction_list", block, d_view, tol, tile_budget,
                                      true, &a));
    if (bi_du < 2) return SPFM_OK;
    const size_t cap = (size_t)std::max<int64_t>(capacity, 1);
    HIPC(bi_keys.alloc(sizeof(uint64_t) * cap));
    HIPC(bi_vals.alloc(sizeof(BiVal) * cap));
    HIPC(bi_cnt.alloc(sizeof(uint64_t)));
    HIPC(hipMemsetAsync(bi_cnt.p, 0, sizeof(uint64_t), stream));
    a.min_count = min_count;
    a.cap = (unsigned long long)capacity;
    a.counter = bi_cnt.as<unsigned long long>();
    a.keys = bi_keys.as<unsigned long long>();
    a.vals = bi_vals.as<BiVal>();
    SPFM_TRY(bank_interaction_run(BI_EMIT, a, tile_budget));
    uint64_t found = 0;
    SPFM_TRY(download(&found, bi_cnt.p, 1));
    SPFM_TRY(sync());
    *n_out = (int64_t)found;
    if ((int64_t)found > capacity) {
        char buf[160];
        snprintf(buf, sizeof buf,
                 "bank_interaction_list: %lld pairs kept by at least %d members, capacity %lld",
                 (long long)found, min_count, (long long)capacity);
        FAIL(SPFM_ERR_INVALID, buf);
    }
    if (found == 0) return SPFM_OK;
    // sorted by the ids = by key: the emission order does not matter
    const size_t nf = (size_t)found;
    HIPC(bi_keys2.alloc(sizeof(uint64_t) * nf));
    HIPC(bi_vals2.alloc(sizeof(BiVal) * nf));
    size_t temp_bytes = 0;
    HIPC(rocprim::radix_sort_pairs(nullptr, temp_bytes, bi_keys.as<uint64_t>(),
                                   bi_keys2.as<uint64_t>(), bi_vals.as<BiVal>(),
                                   bi_vals2.as<BiVal>(), nf, 0, 64, stream));
    HIPC(bi_tmp.alloc(temp_bytes));
    HIPC(rocprim::radix_sort_pairs(bi_tmp.p, temp_bytes, bi_keys.as<uint64_t>(),
                                   bi_keys2.as<uint64_t>(), bi_vals.as<BiVal>(),
                                   bi_vals2.as<BiVal>(), nf, 0, 64, stream));
    std::vector<uint64_t> hk(nf);
    std::vector<BiVal> hv(nf);  // the caller's arrays are written only once nothing can fail
    SPFM_TRY(download(hk.data(), bi_keys2.p, nf));
    SPFM_TRY(download(hv.data(), bi_vals2.p, nf));
    SPFM_TRY(sync());
    for (size_t q = 0; q < nf; ++q) {
        int_split_key(hk[q], rows + q, cols + q);
        count[q] = (int32_t)(hv[q].cn & 0xffu);
        n_pos[q] = (int32_t)(hv[q].cn >> 8);
        sum[q] = hv[q].sum;
    }
    return SPFM_OK;
}

int spfm_engine::bank_interaction_counts(int block, int32_t d_view, double tol, int64_t L,
                                         const int32_t* rows, const int32_t* cols, int32_t* count,
                                         int32_t* n_pos, double* sum) {
    if (L < 0) FAIL(SPFM_ERR_INVALID, "bank_interaction_counts: L must be >= 0");
    if (L > 0 && (!rows || !cols || !count || !n_pos || !sum))
        FAIL(SPFM_ERR_INVALID, "bank_interaction_counts: NULL array");
    BiArgs a;
    SPFM_TRY(bank_interaction_prepare("bank_interaction_counts", block, d_view, tol, 0, false, &a));
    for (int64_t q = 0; q < L; ++q)
        if (rows[q] < 0 || rows[q] >= d_view || cols[q] < 0 || cols[q] >= d_view)
            FAIL(SPFM_ERR_INVALID, "bank_interaction_counts: feature id outside the view");
    if (L == 0) return SPFM_OK;
    HIPC(bi_io.alloc(sizeof(int32_t) * 4 * (size_t)L));
    HIPC(bi_out.alloc(sizeof(double) * (size_t)L));
    int32_t* dr = bi_io.as<int32_t>();
    int32_t *dc = dr + L, *dn = dc + L, *dp = dn + L;
    return run_staged([&]() -> int {
        SPFM_TRY(upload_to(dr, rows, (size_t)L));
        SPFM_TRY(upload_to(dc, cols, (size_t)L));
        hipLaunchKernelGGL(bi_counts_kernel, dim3(cdiv(L, kBlock)), dim3(kBlock), 0, stream, a.pt,
                           a.S, a.F, a.koff, a.lams, tol, (long long)L, dr, dc, dn, dp,
                           bi_out.as<double>());
        HIPC(hipGetLastError());
        SPFM_TRY(download(count, dn, (size_t)L));
        SPFM_TRY(download(n_pos, dp, (size_t)L));
        return download(sum, bi_out.p, (size_t)L);
    });
}

extern "C" {

int spfm_bank_interaction_hist(spfm_handle h, int block, int32_t d_view, double tol,
                               int64_t tile_budget, int64_t* hist, int64_t* per_member) {
    SPFM_GUARD(h);
    return h->bank_interaction_hist(block, d_view, tol, tile_budget, hist, per_member);
}

int spfm_bank_interaction_list(spfm_handle h, int block, int32_t d_view, double tol, int min_count,
                               int64_t tile_budget, int64_t capacity, int32_t* rows, int32_t* cols,
                               int32_t* count, int32_t* n_pos, double* sum, int64_t* n_out) {
    SPFM_GUARD(h);
    return h->bank_interaction_list(block, d_view, tol, min_count, tile_budget, capacity, rows,
                                    cols, count, n_pos, sum, n_out);
}

int spfm_bank_interaction_counts(spfm_handle h, int block, int32_t d_view, double tol, int64_t L,
                                 const int32_t* rows, const int32_t* cols, int32_t* count,
                                 int32_t* n_pos, double* sum) {
    SPFM_GUARD(h);
    return h->bank_interaction_counts(block, d_view, tol, L, rows, cols, count, n_pos, sum);
}

}  // extern "C"
