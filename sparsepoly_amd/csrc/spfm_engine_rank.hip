// spfm_engine_rank.hip -- spfm_rank_set_candidates / _scores / _topk / _topk_excl / _eval
// (include/spfm.h): the scores of every (context row, candidate row) pair under the handle's
// parameters, the K best candidates of every context row (with or without a per-row list of
// candidates left out) and the exact ranks of held-out candidates.  score = rowconst + colconst +
// U V^T (spfm_rank.hip.h, spfm_rankeval.hip.h); the candidate towers are built once and kept,
// contexts go through in slabs of rows, the product is consumed tile by tile.  Read-only like the
// interaction unit: scratch of its own, the live parameter image is read through its strides and
// no validity flag changes.  See DESIGN.md sections 15 and 15a.
#include "spfm_engine.hip.h"
#include "spfm_rankeval.hip.h"

#include <algorithm>

static_assert(kRankMaxK == SPFM_RANK_MAX_K, "header and device agree on the cap");
static_assert(kRankMaxTargets == SPFM_RANK_MAX_TARGETS, "header and device agree on the cap");

namespace {
constexpr int64_t kRankDenseSlabBytes = 256ll << 20;  // device image of one dense slab
}  // namespace

void spfm_engine::rank_release() {
    for (DevBuf* b : {&rk_V, &rk_cc, &rk_U, &rk_rc, &rk_xp, &rk_xi, &rk_xv, &rk_dense, &rk_ep,
                      &rk_ei, &rk_tp, &rk_ti, &rk_ts, &rk_tr, &rk_pairs})
        b->release();
    rk_sel.release();
    rk_zflag.clear();
    rk_have = false;
    rk_C = 0;
}

int spfm_engine::check_csr(const char* what, int64_t rows, const int64_t* indptr,
                           const int32_t* indices, const double* data, int d_,
                           int64_t max_row_len) {
    const std::string w(what);
    if (rows < 0 || !indptr) FAIL(SPFM_ERR_INVALID, w + ": bad arguments");
    if (indptr[0] != 0) FAIL(SPFM_ERR_INVALID, w + ": indptr[0] must be 0");
    for (int64_t i = 0; i < rows; ++i) {
        if (indptr[i + 1] < indptr[i]) FAIL(SPFM_ERR_INVALID, w + ": indptr is not monotone");
        if (indptr[i + 1] - indptr[i] > max_row_len)  // (the one cap in use: INT32_MAX)
            FAIL(SPFM_ERR_UNSUPPORTED, w + ": a row with more than 2^31 - 1 stored entries");
    }
    const int64_t nz = indptr[rows];
    if (nz > 0 && (!indices || !data)) FAIL(SPFM_ERR_INVALID, w + ": NULL array");
    for (int64_t ii = 0; ii < nz; ++ii)
        if (indices[ii] < 0 || indices[ii] >= d_)
            FAIL(SPFM_ERR_INVALID, w + ": column index out of range");
    return SPFM_OK;
}

template <int M>
void spfm_engine::rank_launch_tower(int64_t row0, int64_t rows, int order_idx, bool lin, int side,
                                    int col0, double* img, double* cst) {
    const BlockView v = live_block(order_idx);
    hipLaunchKernelGGL((tower_kernel<double, M>), dim3(cdiv(rows * kWave, kBlock)), dim3(kBlock), 0,
                       stream, row0, rows, k, rk_xp.as<int64_t>(), rk_xi.as<int32_t>(),
                       rk_xv.as<double>(), v.base, v.ss, v.sj, lams.as<double>(),
                       lin ? w.as<double>() : (const double*)nullptr, side, rk_Rp, col0, img, cst);
}

// the towers of rows [row0, row0 + rows) of the staged CSR matrix into img / cst (cleared here)
int spfm_engine::rank_towers(int64_t row0, int64_t rows, int side, double* img, double* cst) {
    const int64_t pad = round_up(rows, kIntTile);
    HIPC(hipMemsetAsync(img, 0, sizeof(double) * (size_t)pad * rk_Rp, stream));
    HIPC(hipMemsetAsync(cst, 0, sizeof(double) * (size_t)pad, stream));
    const bool lin = rk_lin != 0;
    if (!SPFM_DISPATCH_KIND(kind_of(rk_degree), true,  // (all-subsets: no linear term)
                            rank_launch_tower<M>(row0, rows, 0, M != 0 && lin, side, 0, img, cst)))
        FAIL(SPFM_ERR_UNSUPPORTED, "rank: degree outside 2..6 and -1");
    if (rk_lower)  // the order-2 term on P[1]
        rank_launch_tower<2>(row0, rows, 1, false, side, k * (rk_degree - 1), img, cst);
    HIPC(hipGetLastError());
    return SPFM_OK;
}

int spfm_engine::rank_set_candidates(int degree, int fit_linear, int add_lower, int64_t n_cand,
                                     const int64_t* indptr, const int32_t* indices,
                                     const double* data) {
    if (!have_params) FAIL(SPFM_ERR_INVALID, "rank_set_candidates: no parameters set");
    if (degree != -1 && (degree < 2 || degree > SPFM_MAX_DEGREE))
        FAIL(SPFM_ERR_UNSUPPORTED, "rank_set_candidates: degree outside 2..6 and -1");
    if (add_lower && (n_orders < 2 || degree < 3))
        FAIL(SPFM_ERR_INVALID, "rank_set_candidates: add_lower_deg2 needs P_[1] and degree >= 3");
    if (n_cand < 1) FAIL(SPFM_ERR_INVALID, "rank_set_candidates: n_cand must be >= 1");
    if (n_cand > INT32_MAX - kIntTile)
        FAIL(SPFM_ERR_UNSUPPORTED, "rank_set_candidates: more than 2^31 - 65 candidates");
    SPFM_TRY(check_csr("rank_set_candidates", n_cand, indptr, indices, data, d, INT64_MAX));
    const int64_t R = (degree == -1 ? (int64_t)k : (int64_t)k * (degree - 1)) + (add_lower ? k : 0);
    const int64_t Rp = round_up(R, 4), pad = round_up(n_cand, kIntTile);
    rank_release();
    rk_degree = degree;
    rk_lin = (degree != -1 && fit_linear) ? 1 : 0;
    rk_lower = add_lower ? 1 : 0;
    rk_R = (int)R;
    rk_Rp = (int)Rp;
    const int64_t nz = indptr[n_cand];
    std::vector<uint8_t> flag((size_t)d, 0);
    for (int64_t ii = 0; ii < nz; ++ii) flag[(size_t)indices[ii]] = 1;
    std::vector<double> hv;
    SPFM_TRY(stage_csr_rows<double>(rk_xp, rk_xi, rk_xv, hv, indptr, indices, data, 0, n_cand));
    HIPC(rk_V.alloc(sizeof(double) * (size_t)pad * Rp));
    HIPC(rk_cc.alloc(sizeof(double) * (size_t)pad));
    SPFM_TRY(rank_towers(0, n_cand, RANK_CAND, rk_V.as<double>(), rk_cc.as<double>()));
    SPFM_TRY(sync());
    rk_zflag.swap(flag);
    rk_C = n_cand;
    rk_have = true;
    return SPFM_OK;
}

// checks of a context matrix (before any device work), then its CSR image on the device
int spfm_engine::rank_contexts(const char* what, int64_t n_ctx, const int64_t* indptr,
                               const int32_t* indices, const double* data) {
    if (!have_params) FAIL(SPFM_ERR_INVALID, std::string(what) + ": no parameters set");
    if (!rk_have) FAIL(SPFM_ERR_INVALID, std::string(what) + ": call spfm_rank_set_candidates first");
    SPFM_TRY(check_csr(what, n_ctx, indptr, indices, data, d, INT64_MAX));
    const int64_t nz = indptr[n_ctx];
    for (int64_t ii = 0; ii < nz; ++ii)
        if (rk_zflag[(size_t)indices[ii]]) {
            char buf[160];
            snprintf(buf, sizeof buf,
                     "%s: column %d has stored entries in the contexts and in the candidates "
                     "(their column sets must be disjoint)", what, (int)indices[ii]);
            FAIL(SPFM_ERR_INVALID, buf);
        }
    if (n_ctx == 0) return SPFM_OK;
    std::vector<double> hv;
    SPFM_TRY(stage_csr_rows<double>(rk_xp, rk_xi, rk_xv, hv, indptr, indices, data, 0, n_ctx));
    return sync();  // the caller's arrays are not read after this
}

// slab rows [r0, r0 + nrow) of the call against the candidates, in strips of strip_tiles tiles
static RankArgs rank_args(const spfm_engine* h, int64_t r0, int64_t nrow, int strip_tiles) {
    RankArgs a;
    memset(&a, 0, sizeof a);
    a.strip_tiles = strip_tiles;
    a.n_strips = (int)cdiv(cdiv(h->rk_C, kIntTile), strip_tiles);
    a.eptr = h->rk_ep.as<int64_t>();
    a.eidx = h->rk_ei.as<int32_t>();
    a.row0 = r0;
    a.U = h->rk_U.as<double>();
    a.V = h->rk_V.as<double>();
    a.rc = h->rk_rc.as<double>();
    a.cc = h->rk_cc.as<double>();
    a.Rp = h->rk_Rp;
    a.nrow = (int)nrow;
    a.C = (int)h->rk_C;
    a.rows_pad = (int)round_up(nrow, kIntTile);
    return a;
}

int spfm_engine::rank_scores(int64_t n_ctx, const int64_t* indptr, const int32_t* indices,
                             const double* data, double* out) {
    SPFM_TRY(rank_contexts("rank_scores", n_ctx, indptr, indices, data));
    if ((double)n_ctx * (double)rk_C * 8.0 > (double)SPFM_RANK_SCORES_MAX_BYTES) {
        char buf[160];
        snprintf(buf, sizeof buf, "rank_scores: %lld x %lld doubles exceed the budget of %lld bytes",
                 (long long)n_ctx, (long long)rk_C, (long long)SPFM_RANK_SCORES_MAX_BYTES);
        FAIL(SPFM_ERR_INVALID, buf);
    }
    if (n_ctx == 0) return SPFM_OK;
    if (!out) FAIL(SPFM_ERR_INVALID, "rank_scores: out is NULL");
    int64_t slab = round_up(rk_row_slab > 0 ? rk_row_slab : kSelSlabDefault, kIntTile);
    const int64_t fit = kRankDenseSlabBytes / (8 * rk_C) / kIntTile * kIntTile;
    slab = std::min(slab, std::max<int64_t>(fit, kIntTile));
    slab = std::min(slab, round_up(n_ctx, kIntTile));
    const int Tc = (int)cdiv(rk_C, kIntTile);
    int64_t strip = rk_cand_strip > 0 ? rk_cand_strip : 8192;
    const int strip_tiles = (int)std::min<int64_t>(cdiv(strip, kIntTile), Tc);
    HIPC(rk_U.alloc(sizeof(double) * (size_t)slab * rk_Rp));
    HIPC(rk_rc.alloc(sizeof(double) * (size_t)slab));
    HIPC(rk_dense.alloc(sizeof(double) * (size_t)slab * (size_t)rk_C));
    const size_t lds = int_stage_lds_bytes();
    DeviceTimer timer;
    rk_device_us = 0;
    for (int64_t r0 = 0; r0 < n_ctx; r0 += slab) {
        const int64_t nrow = std::min(slab, n_ctx - r0);
        timer.begin(stream);
        SPFM_TRY(rank_towers(r0, nrow, RANK_CTX, rk_U.as<double>(), rk_rc.as<double>()));
        RankArgs a = rank_args(this, r0, nrow, strip_tiles);
        a.dense = rk_dense.as<double>();
        hipLaunchKernelGGL((rank_tile_kernel<RANK_DENSE>),
                           dim3((unsigned)a.n_strips, (unsigned)(a.rows_pad / kIntTile)),
                           dim3(kBlock), lds, stream, a);
        HIPC(hipGetLastError());
        timer.end(stream);
        SPFM_TRY(download(out + (size_t)r0 * rk_C, rk_dense.p, (size_t)nrow * rk_C));
        SPFM_TRY(sync());
        timer.collect();
    }
    rk_device_us = (int)std::min(timer.ms * 1e3, 2e9);
    return SPFM_OK;
}

// a per-row list of candidates: pointers start at 0 and do not decrease, ids in [0, C) and
// strictly ascending within a row
int spfm_engine::rank_check_pattern(const char* what, const char* name, int64_t rows,
                                    const int64_t* ptr, const int32_t* idx) {
    const std::string w = std::string(what) + ": " + name;
    if (rows < 0 || !ptr) FAIL(SPFM_ERR_INVALID, w + ": bad arguments");
    if (ptr[0] != 0) FAIL(SPFM_ERR_INVALID, w + ": the pointers must start at 0");
    for (int64_t i = 0; i < rows; ++i)
        if (ptr[i + 1] < ptr[i]) FAIL(SPFM_ERR_INVALID, w + ": the pointers decrease");
    if (ptr[rows] > 0 && !idx) FAIL(SPFM_ERR_INVALID, w + ": NULL array");
    for (int64_t i = 0; i < rows; ++i)
        for (int64_t ii = ptr[i]; ii < ptr[i + 1]; ++ii) {
            if (idx[ii] < 0 || idx[ii] >= rk_C)
                FAIL(SPFM_ERR_INVALID, w + ": candidate id out of range");
            if (ii > ptr[i] && idx[ii] <= idx[ii - 1])
                FAIL(SPFM_ERR_INVALID, w + ": the ids of a row must be ascending without duplicates");
        }
    return SPFM_OK;
}

int spfm_engine::rank_topk(int64_t n_ctx, const int64_t* indptr, const int32_t* indices,
                           const double* data, const int64_t* eptr, const int32_t* eidx, int64_t K,
                           int32_t* idx_out, double* val_out, int64_t* k_out) {
    if (!k_out) FAIL(SPFM_ERR_INVALID, "rank_topk: k_out is NULL");
    *k_out = 0;
    if (K < 1) FAIL(SPFM_ERR_INVALID, "rank_topk: K must be >= 1");
    if (K > SPFM_RANK_MAX_K) {
        char buf[96];
        snprintf(buf, sizeof buf, "rank_topk: K must be <= SPFM_RANK_MAX_K = %d",
                 (int)SPFM_RANK_MAX_K);
        FAIL(SPFM_ERR_UNSUPPORTED, buf);
    }
    if (eptr) {
        if (!rk_have) FAIL(SPFM_ERR_INVALID, "rank_topk: call spfm_rank_set_candidates first");
        SPFM_TRY(rank_check_pattern("rank_topk", "excluded", n_ctx, eptr, eidx));
    }
    SPFM_TRY(rank_contexts("rank_topk", n_ctx, indptr, indices, data));
    const int Ko = (int)std::min<int64_t>(K, rk_C);
    if (n_ctx > 0 && (!idx_out || !val_out)) FAIL(SPFM_ERR_INVALID, "rank_topk: NULL output");
    if (n_ctx == 0) {
        *k_out = Ko;
        return SPFM_OK;
    }
    const SelPlan plan = sel_plan(rk_row_slab, rk_cand_strip, n_ctx, (int)cdiv(rk_C, kIntTile));
    const int64_t slab = plan.slab;
    const size_t lds = plan.lds + (eptr ? kRankExclLdsBytes : 0);
    HIPC(hipFuncSetAttribute(eptr ? (const void*)rank_tile_kernel<RANK_SELECT, true>
                                  : (const void*)rank_tile_kernel<RANK_SELECT>,
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (eptr) {
        SPFM_TRY(upload(rk_ep, eptr, (size_t)n_ctx + 1));
        SPFM_TRY(upload(rk_ei, eidx, (size_t)eptr[n_ctx]));
    }
    HIPC(rk_U.alloc(sizeof(double) * (size_t)slab * rk_Rp));
    HIPC(rk_rc.alloc(sizeof(double) * (size_t)slab));
    HIPC(rk_sel.alloc(plan.n_strips, slab, Ko));
    // the caller's arrays are written only once nothing can fail
    std::vector<int32_t> hi((size_t)n_ctx * Ko);
    std::vector<double> hv((size_t)n_ctx * Ko);
    DeviceTimer timer;
    rk_device_us = 0;
    for (int64_t r0 = 0; r0 < n_ctx; r0 += slab) {
        const int64_t nrow = std::min(slab, n_ctx - r0);
        timer.begin(stream);
        SPFM_TRY(rank_towers(r0, nrow, RANK_CTX, rk_U.as<double>(), rk_rc.as<double>()));
        RankArgs a = rank_args(this, r0, nrow, plan.strip_tiles);
        a.sel = {Ko, kSelCap, rk_sel.lv.as<double>(), rk_sel.li.as<int32_t>(),
                 rk_sel.ov.as<double>(), rk_sel.oi.as<int32_t>()};
        HIPC(rk_sel.clear(nrow, Ko, 0xFF, stream));  // slots no finite score fills: index -1, NaN
        const dim3 grid((unsigned)a.n_strips, (unsigned)(a.rows_pad / kIntTile));
        if (eptr)
            hipLaunchKernelGGL((rank_tile_kernel<RANK_SELECT, true>), grid, dim3(kBlock), lds,
                               stream, a);
        else
            hipLaunchKernelGGL((rank_tile_kernel<RANK_SELECT>), grid, dim3(kBlock), lds, stream, a);
        hipLaunchKernelGGL(rank_merge_kernel, dim3(cdiv(nrow * kWave, kBlock)), dim3(kBlock), 0,
                           stream, a);
        HIPC(hipGetLastError());
        timer.end(stream);
        SPFM_TRY(download(hv.data() + (size_t)r0 * Ko, rk_sel.ov.p, (size_t)nrow * Ko));
        SPFM_TRY(download(hi.data() + (size_t)r0 * Ko, rk_sel.oi.p, (size_t)nrow * Ko));
        SPFM_TRY(sync());
        timer.collect();
    }
    rk_device_us = (int)std::min(timer.ms * 1e3, 2e9);
    std::copy(hi.begin(), hi.end(), idx_out);
    std::copy(hv.begin(), hv.end(), val_out);
    *k_out = Ko;
    return SPFM_OK;
}

int spfm_engine::rank_eval(int64_t n_ctx, const int64_t* indptr, const int32_t* indices,
                           const double* data, const int64_t* tptr, const int32_t* tidx,
                           const int64_t* eptr, const int32_t* eidx, int32_t* rank_out,
                           double* score_out, int32_t* n_eff_out) {
    if (!have_params) FAIL(SPFM_ERR_INVALID, "rank_eval: no parameters set");
    if (!rk_have) FAIL(SPFM_ERR_INVALID, "rank_eval: call spfm_rank_set_candidates first");
    SPFM_TRY(rank_check_pattern("rank_eval", "targets", n_ctx, tptr, tidx));
    if (eptr) SPFM_TRY(rank_check_pattern("rank_eval", "excluded", n_ctx, eptr, eidx));
    int tcap = 1;
    for (int64_t i = 0; i < n_ctx; ++i) {
        const int64_t nt = tptr[i + 1] - tptr[i];
        if (nt > SPFM_RANK_MAX_TARGETS) {
            char buf[160];
            snprintf(buf, sizeof buf,
                     "rank_eval: row %lld has %lld targets, more than SPFM_RANK_MAX_TARGETS = %d",
                     (long long)i, (long long)nt, (int)SPFM_RANK_MAX_TARGETS);
            FAIL(SPFM_ERR_UNSUPPORTED, buf);
        }
        tcap = std::max(tcap, (int)nt);
        if (!eptr) continue;
        for (int64_t it = tptr[i], ie = eptr[i]; it < tptr[i + 1] && ie < eptr[i + 1];) {
            if (tidx[it] == eidx[ie]) {
                char buf[160];
                snprintf(buf, sizeof buf, "rank_eval: candidate %d is a target of row %lld and "
                         "excluded from it", (int)tidx[it], (long long)i);
                FAIL(SPFM_ERR_INVALID, buf);
            }
            if (tidx[it] < eidx[ie])
                ++it;
            else
                ++ie;
        }
    }
    SPFM_TRY(rank_contexts("rank_eval", n_ctx, indptr, indices, data));
    const int64_t nt = tptr[n_ctx];
    std::vector<int32_t> hr((size_t)nt, 0);
    std::vector<double> hs((size_t)nt, 0.0);
    rk_device_us = 0;
    if (nt > 0) {
        const int Tc = (int)cdiv(rk_C, kIntTile);
        const SelPlan plan = sel_plan(rk_row_slab, rk_cand_strip, n_ctx, Tc);
        const int64_t slab = plan.slab;
        const size_t lds = rank_count_lds_bytes(tcap);
        HIPC(hipFuncSetAttribute(eptr ? (const void*)rank_count_kernel<true>
                                      : (const void*)rank_count_kernel<false>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIPC(rk_U.alloc(sizeof(double) * (size_t)slab * rk_Rp));
        HIPC(rk_rc.alloc(sizeof(double) * (size_t)slab));
        SPFM_TRY(upload(rk_tp, tptr, (size_t)n_ctx + 1));
        SPFM_TRY(upload(rk_ti, tidx, (size_t)nt));
        if (eptr) {
            SPFM_TRY(upload(rk_ep, eptr, (size_t)n_ctx + 1));
            SPFM_TRY(upload(rk_ei, eidx, (size_t)eptr[n_ctx]));
        }
        HIPC(rk_ts.alloc(sizeof(double) * (size_t)nt));
        HIPC(rk_tr.alloc(sizeof(int32_t) * (size_t)nt));
        HIPC(hipMemsetAsync(rk_ts.p, 0, sizeof(double) * (size_t)nt, stream));
        HIPC(hipMemsetAsync(rk_tr.p, 0, sizeof(int32_t) * (size_t)nt, stream));
        std::vector<int64_t> keys;
        std::vector<int2> pairs;
        DeviceTimer timer;
        for (int64_t r0 = 0; r0 < n_ctx; r0 += slab) {
            const int64_t nrow = std::min(slab, n_ctx - r0);
            if (tptr[r0 + nrow] == tptr[r0]) continue;  // no target in the slab
            // the (row tile, candidate tile) pairs of the slab that hold a target
            keys.clear();
            for (int64_t i = 0; i < nrow; ++i)
                for (int64_t ii = tptr[r0 + i]; ii < tptr[r0 + i + 1]; ++ii)
                    keys.push_back((i / kIntTile) * Tc + tidx[ii] / kIntTile);
            std::sort(keys.begin(), keys.end());
            keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
            pairs.resize(keys.size());
            for (size_t q = 0; q < keys.size(); ++q)
                pairs[q] = make_int2((int)(keys[q] / Tc), (int)(keys[q] % Tc));
            SPFM_TRY(upload(rk_pairs, pairs.data(), pairs.size()));
            timer.begin(stream);
            SPFM_TRY(rank_towers(r0, nrow, RANK_CTX, rk_U.as<double>(), rk_rc.as<double>()));
            RankEvalArgs e;
            memset(&e, 0, sizeof e);
            e.r = rank_args(this, r0, nrow, plan.strip_tiles);
            e.tptr = rk_tp.as<int64_t>();
            e.tidx = rk_ti.as<int32_t>();
            e.pairs = rk_pairs.as<int2>();
            e.tscore = rk_ts.as<double>();
            e.trank = rk_tr.as<int32_t>();
            e.tcap = tcap;
            hipLaunchKernelGGL(rank_tscore_kernel, dim3((unsigned)pairs.size()), dim3(kBlock), 0,
                               stream, e);
            const dim3 grid((unsigned)e.r.n_strips, (unsigned)(e.r.rows_pad / kIntTile));
            if (eptr)
                hipLaunchKernelGGL(rank_count_kernel<true>, grid, dim3(kBlock), lds, stream, e);
            else
                hipLaunchKernelGGL(rank_count_kernel<false>, grid, dim3(kBlock), lds, stream, e);
            HIPC(hipGetLastError());
            timer.end(stream);
            SPFM_TRY(sync());  // `pairs` and the context towers are rewritten by the next slab
            timer.collect();
        }
        SPFM_TRY(download(hs.data(), rk_ts.p, (size_t)nt));
        SPFM_TRY(download(hr.data(), rk_tr.p, (size_t)nt));
        SPFM_TRY(sync());
        rk_device_us = (int)std::min(timer.ms * 1e3, 2e9);
        for (int64_t ii = 0; ii < nt; ++ii)
            if (!std::isfinite(hs[(size_t)ii])) hr[(size_t)ii] = -1;
    }
    // the caller's arrays are written only once nothing can fail
    if (rank_out) std::copy(hr.begin(), hr.end(), rank_out);
    if (score_out) std::copy(hs.begin(), hs.end(), score_out);
    if (n_eff_out)
        for (int64_t i = 0; i < n_ctx; ++i)
            n_eff_out[i] = (int32_t)(rk_C - (eptr ? eptr[i + 1] - eptr[i] : 0));
    return SPFM_OK;
}

extern "C" {

int spfm_rank_set_candidates(spfm_handle h, int degree, int fit_linear, int add_lower_deg2,
                             int64_t n_cand, const int64_t* indptr, const int32_t* indices,
                             const double* data) {
    SPFM_GUARD(h);
    return h->rank_set_candidates(degree, fit_linear, add_lower_deg2, n_cand, indptr, indices,
                                  data);
}

int spfm_rank_scores(spfm_handle h, int64_t n_ctx, const int64_t* indptr, const int32_t* indices,
                     const double* data, double* out) {
    SPFM_GUARD(h);
    return h->rank_scores(n_ctx, indptr, indices, data, out);
}

int spfm_rank_topk(spfm_handle h, int64_t n_ctx, const int64_t* indptr, const int32_t* indices,
                   const double* data, int64_t K, int32_t* idx_out, double* val_out,
                   int64_t* k_out) {
    SPFM_GUARD(h);
    return h->rank_topk(n_ctx, indptr, indices, data, nullptr, nullptr, K, idx_out, val_out,
                        k_out);
}

int spfm_rank_topk_excl(spfm_handle h, int64_t n_ctx, const int64_t* indptr,
                        const int32_t* indices, const double* data, const int64_t* eptr,
                        const int32_t* eidx, int64_t K, int32_t* idx_out, double* val_out,
                        int64_t* k_out) {
    SPFM_GUARD(h);
    return h->rank_topk(n_ctx, indptr, indices, data, eptr, eidx, K, idx_out, val_out, k_out);
}

int spfm_rank_eval(spfm_handle h, int64_t n_ctx, const int64_t* indptr, const int32_t* indices,
                   const double* data, const int64_t* tptr, const int32_t* tidx,
                   const int64_t* eptr, const int32_t* eidx, int32_t* rank_out, double* score_out,
                   int32_t* n_eff_out) {
    SPFM_GUARD(h);
    return h->rank_eval(n_ctx, indptr, indices, data, tptr, tidx, eptr, eidx, rank_out, score_out,
                        n_eff_out);
}

int spfm_rank_set_partition(spfm_handle h, int64_t row_slab, int64_t cand_strip) {
    if (!h) return SPFM_ERR_INVALID;
    if (row_slab < 0 || row_slab > (1 << 20) || cand_strip < 0 || cand_strip > kSelMaxStrip) {
        h->err = "rank_set_partition: row_slab must be in [0, 2^20], cand_strip in [0, 65536]";
        return SPFM_ERR_INVALID;
    }
    h->rk_row_slab = (int)row_slab;
    h->rk_cand_strip = (int)cand_strip;
    return SPFM_OK;
}

int spfm_rank_info(spfm_handle h, int64_t* out4) {
    if (!h || !out4) return SPFM_ERR_INVALID;
    out4[0] = (int64_t)h->rank_scratch_bytes();
    out4[1] = h->rk_device_us;
    out4[2] = h->rk_row_slab;
    out4[3] = h->rk_cand_strip;
    return SPFM_OK;
}

int spfm_rank_release(spfm_handle h) {
    SPFM_GUARD(h);
    h->rank_release();
    return SPFM_OK;
}

}  // extern "C"
