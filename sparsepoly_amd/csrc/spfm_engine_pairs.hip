// spfm_engine_pairs.hip -- spfm_explain_pairs_csr / _pairs_topk_csr / _pairs_grouped_csr
// (include/spfm.h): which pairs of a row's features produced its score.  Per stored pair the
// Shapley-Taylor interaction index of order 2 against a zero baseline, or the mixed second
// derivative; per stored entry its main effect; per row the K largest pairs and the
// group x group table (spfm_pairs.hip.h).  Everything the explain unit has is used as it is: the
// slab image of the CSR rows, the coefficient upload, the checks, the timing, the partition and
// spfm_explain_info.  See DESIGN.md section 16a.
#include "spfm_engine.hip.h"
#include "spfm_pairs.hip.h"

#include <algorithm>

static_assert(kPairsMaxK == SPFM_PAIRS_MAX_K && kPairsMaxGroups == SPFM_PAIRS_MAX_GROUPS,
              "header and device agree on the caps");
static_assert(PAIRS_INTERACTION == SPFM_PAIRS_INTERACTION && PAIRS_HESSIAN == SPFM_PAIRS_HESSIAN,
              "header and device agree on the modes");

namespace {
// rows of a slab: 24 bytes per row (entry offset, pair offset, slack), 16 K of lists,
// 8 (G (G + 1) / 2 + G) of tables, within 64 MiB
constexpr int64_t kPairsRowBudget = 64ll << 20;
inline int64_t row_pairs(const int64_t* indptr, int64_t i) {
    const int64_t m = indptr[i + 1] - indptr[i];
    return m * (m - 1) / 2;
}
}  // namespace

// every check of the three entries, before any device work and before any output is written
int spfm_engine::pairs_check(const char* what, const PairsCall& c) {
    const std::string w(what);
    char buf[128];
    SPFM_TRY(explain_check_model(what, c.m));
    if (c.pmode != SPFM_PAIRS_INTERACTION && c.pmode != SPFM_PAIRS_HESSIAN)
        FAIL(SPFM_ERR_INVALID, w + ": mode must be SPFM_PAIRS_INTERACTION or _HESSIAN");
    if (c.kind == PAIRS_TOPK) {
        if (c.m.K < 1) FAIL(SPFM_ERR_INVALID, w + ": K must be >= 1");
        if (c.m.K > SPFM_PAIRS_MAX_K) {
            snprintf(buf, sizeof buf, "%s: K must be <= SPFM_PAIRS_MAX_K = %d", what,
                     (int)SPFM_PAIRS_MAX_K);
            FAIL(SPFM_ERR_UNSUPPORTED, buf);
        }
    }
    if (c.kind == PAIRS_GROUPED) {
        if (c.G < 1) FAIL(SPFM_ERR_INVALID, w + ": G must be >= 1");
        if (c.G > SPFM_PAIRS_MAX_GROUPS) {
            snprintf(buf, sizeof buf, "%s: G must be <= SPFM_PAIRS_MAX_GROUPS = %d", what,
                     (int)SPFM_PAIRS_MAX_GROUPS);
            FAIL(SPFM_ERR_UNSUPPORTED, buf);
        }
        if (!c.group) FAIL(SPFM_ERR_INVALID, w + ": group is NULL");
        for (int64_t j = 0; j < d; ++j)
            if (c.group[j] < 0 || c.group[j] >= c.G)
                FAIL(SPFM_ERR_INVALID, w + ": group id out of range");
    }
    SPFM_TRY(explain_check_rows(what, c.m));
    int64_t total = 0;
    for (int64_t i = 0; i < c.m.n; ++i) {
        if (c.m.indptr[i + 1] - c.m.indptr[i] > kPairsMaxRow)
            FAIL(SPFM_ERR_UNSUPPORTED, w + ": a row with more than 65536 stored entries");
        total += row_pairs(c.m.indptr, i);
    }
    if (c.kind == PAIRS_LIST) {
        if (total > SPFM_PAIRS_MAX_BYTES / (int64_t)sizeof(double)) {
            snprintf(buf, sizeof buf, "%s: %lld pairs to list, more than SPFM_PAIRS_MAX_BYTES",
                     what, (long long)total);
            FAIL(SPFM_ERR_UNSUPPORTED, buf);
        }
        if (total > 0 && !c.out_pairs) FAIL(SPFM_ERR_INVALID, w + ": out_pairs is NULL");
        if (c.out_main && c.pmode != SPFM_PAIRS_INTERACTION)
            FAIL(SPFM_ERR_INVALID, w + ": out_main belongs to SPFM_PAIRS_INTERACTION");
    }
    if (c.m.n > 0 && c.kind == PAIRS_TOPK && (!c.m.idx || !c.col_b || !c.m.val))
        FAIL(SPFM_ERR_INVALID, w + ": NULL output");
    if (c.m.n > 0 && c.kind == PAIRS_GROUPED && (!c.out_pairs || !c.out_main))
        FAIL(SPFM_ERR_INVALID, w + ": NULL output");
    return SPFM_OK;
}

template <typename T, int M>
void spfm_engine::pairs_launch_block(int64_t rows, int64_t e0, const double* Pt_o,
                                     const double* coef_o, int mode) {
    hipLaunchKernelGGL((pairs_block_kernel<T, M>), dim3(cdiv(rows, kBlock / kWave)), dim3(kBlock),
                       0, stream, rows, k, e0, ex_rp.as<int64_t>(), ex_ri.as<int32_t>(),
                       ex_rv.as<T>(), ex_pp.as<int64_t>(), Pt_o, lams.as<double>(), coef_o, mode,
                       ex_pv.as<double>());
}

// rows [r0, r1), pp the pair offsets of the call's rows: stage, main, the blocks in the caller's
// order, top-K or tables, copy back
template <typename T>
int spfm_engine::pairs_slab(const PairsCall& c, const int64_t* pp, int64_t r0, int64_t r1) {
    const ExplainCall& m = c.m;
    const int64_t rows = r1 - r0, e0 = m.indptr[r0], ne = m.indptr[r1] - e0;
    const int64_t q0 = pp[r0], nq = pp[r1] - q0;
    const bool want_main = c.kind == PAIRS_GROUPED || c.out_main != nullptr;
    const int cells = c.G * (c.G + 1) / 2;
    std::vector<int64_t> hp((size_t)rows + 1);  // the slab's pair offsets, from 0: staging as `hv`
    for (int64_t i = 0; i <= rows; ++i) hp[(size_t)i] = pp[r0 + i] - q0;
    HIPC(ex_pv.alloc(sizeof(double) * (size_t)nq));
    HIPC(ex_pp.alloc(sizeof(int64_t) * ((size_t)rows + 1)));
    if (want_main) HIPC(ex_out.alloc(sizeof(double) * (size_t)ne));
    if (c.kind == PAIRS_TOPK) {
        HIPC(ex_ti.alloc(sizeof(int32_t) * (size_t)rows * m.K * 2));
        HIPC(ex_tv.alloc(sizeof(double) * (size_t)rows * m.K));
    }
    if (c.kind == PAIRS_GROUPED) {
        HIPC(ex_gp.alloc(sizeof(double) * (size_t)rows * cells));
        HIPC(ex_gm.alloc(sizeof(double) * (size_t)rows * c.G));
    }
    std::vector<T> hv;
    DeviceTimer timer;
    const auto enqueue = [&]() -> int {
        SPFM_TRY(stage_csr_rows<T>(ex_rp, ex_ri, ex_rv, hv, m.indptr, m.indices, m.data, r0, r1));
        SPFM_TRY(upload_to(ex_pp.p, hp.data(), hp.size()));
        timer.begin(stream);
        if (nq > 0) HIPC(hipMemsetAsync(ex_pv.p, 0, sizeof(double) * (size_t)nq, stream));
        if (want_main && ne > 0)
            hipLaunchKernelGGL((explain_init_kernel<T>), dim3(cdiv(ne, kBlock)), dim3(kBlock), 0,
                               stream, ne, ex_ri.as<int32_t>(), ex_rv.as<T>(),
                               m.fit_linear ? w.as<double>() : (const double*)nullptr,
                               (int)EXPLAIN_ATTRIBUTION, ex_out.as<double>());
        for (int q = 0; q < m.n_blocks; ++q) {
            const double* Pt_o = Pt.as<double>() + (size_t)m.order_idx[q] * k * d;
            const double* coef_o = ex_coef.as<double>() + (size_t)q * k * kExplainCoefs;
            if (want_main && ne > 0)
                hipLaunchKernelGGL((pairs_main_kernel<T>), dim3(cdiv(ne, kBlock)), dim3(kBlock), 0,
                                   stream, ne, k, ex_ri.as<int32_t>(), ex_rv.as<T>(), Pt_o,
                                   lams.as<double>(), coef_o, ex_out.as<double>());
            if (nq == 0) continue;
            (void)SPFM_DISPATCH_KIND(m.degree[q], false,  // (2..6: explain_check_model)
                                     pairs_launch_block<T, M>(rows, e0, Pt_o, coef_o, c.pmode));
        }
        const unsigned row_waves = cdiv(rows * kWave, kBlock);
        if (c.kind == PAIRS_TOPK)
            hipLaunchKernelGGL(pairs_topk_kernel, dim3(row_waves), dim3(kBlock), 0, stream, rows,
                               e0, ex_rp.as<int64_t>(), ex_ri.as<int32_t>(), ex_pp.as<int64_t>(),
                               ex_pv.as<double>(), m.K, ex_ti.as<int32_t>(),
                               ex_ti.as<int32_t>() + (size_t)rows * m.K, ex_tv.as<double>());
        if (c.kind == PAIRS_GROUPED)
            hipLaunchKernelGGL(pairs_group_kernel, dim3(row_waves), dim3(kBlock), 0, stream, rows,
                               e0, ex_rp.as<int64_t>(), ex_ri.as<int32_t>(), ex_pp.as<int64_t>(),
                               ex_pv.as<double>(), ex_out.as<double>(), c.G, ex_grp.as<int32_t>(),
                               ex_gp.as<double>(), ex_gm.as<double>());
        HIPC(hipGetLastError());
        timer.end(stream);
        if (c.kind == PAIRS_LIST) {
            SPFM_TRY(download(c.out_pairs + q0, ex_pv.p, (size_t)nq));
            if (c.out_main) SPFM_TRY(download(c.out_main + e0, ex_out.p, (size_t)ne));
        } else if (c.kind == PAIRS_TOPK) {
            const size_t cnt = (size_t)rows * m.K;
            SPFM_TRY(download(m.idx + (size_t)r0 * m.K, ex_ti.p, cnt));
            SPFM_TRY(download(c.col_b + (size_t)r0 * m.K, ex_ti.as<int32_t>() + cnt, cnt));
            SPFM_TRY(download(m.val + (size_t)r0 * m.K, ex_tv.p, cnt));
        } else {
            SPFM_TRY(download(c.out_pairs + (size_t)r0 * cells, ex_gp.p, (size_t)rows * cells));
            SPFM_TRY(download(c.out_main + (size_t)r0 * c.G, ex_gm.p, (size_t)rows * c.G));
        }
        return SPFM_OK;
    };
    return run_staged(enqueue, &timer, &ex_device_us);
}

template <typename T>
int spfm_engine::pairs_run(const char* what, const PairsCall& c) {
    SPFM_TRY(pairs_check(what, c));
    const ExplainCall& m = c.m;
    if (m.n == 0) return SPFM_OK;
    SPFM_TRY(ensure_p());
    pt_valid = false;  // P is the source of truth here, as in output_t
    SPFM_TRY(ensure_pt());
    SPFM_TRY(upload(ex_coef, m.coef, (size_t)m.n_blocks * k * kExplainCoefs));
    if (c.kind == PAIRS_GROUPED) SPFM_TRY(upload(ex_grp, c.group, (size_t)d));
    const int64_t slab_nnz = ex_slab_nnz > 0 ? ex_slab_nnz : kExplainSlabMax;
    const int64_t slab_pairs = 2 * slab_nnz;  // 2^24 at the default
    const int64_t cells = (int64_t)c.G * (c.G + 1) / 2;
    const int64_t row_cap =
        std::max<int64_t>(1, kPairsRowBudget / (24 + 16 * (int64_t)m.K + 8 * (cells + c.G)));
    std::vector<int64_t> pp((size_t)m.n + 1, 0);  // pair offsets of the call's rows
    for (int64_t i = 0; i < m.n; ++i) pp[(size_t)i + 1] = pp[(size_t)i] + row_pairs(m.indptr, i);
    ex_device_us = 0;
    ex_slabs = 0;
    for (int64_t r0 = 0; r0 < m.n;) {
        const int64_t r1 =
            slab_end(r0, m.n, row_cap, {m.indptr, slab_nnz}, {pp.data(), slab_pairs});
        SPFM_TRY(pairs_slab<T>(c, pp.data(), r0, r1));
        ++ex_slabs;
        r0 = r1;
    }
    return SPFM_OK;
}

extern "C" {

int spfm_explain_pairs_csr(spfm_handle h, int64_t n, const int64_t* indptr, const int32_t* indices,
                           const double* data, int n_blocks, const int32_t* order_idx,
                           const int32_t* degree, const double* coef, int fit_linear, int mode,
                           double* out_pairs, double* out_main) {
    SPFM_GUARD(h);
    const spfm_engine::PairsCall c = {
        {n, indptr, indices, data, n_blocks, order_idx, degree, coef, fit_linear,
         SPFM_EXPLAIN_ATTRIBUTION, nullptr, nullptr, false, 0, nullptr, nullptr},
        spfm_engine::PAIRS_LIST, mode, 0, nullptr, out_pairs, out_main, nullptr};
    return SPFM_DISPATCH(h->dtype, return h->pairs_run<T>("explain_pairs_csr", c));
}

int spfm_explain_pairs_topk_csr(spfm_handle h, int64_t n, const int64_t* indptr,
                                const int32_t* indices, const double* data, int n_blocks,
                                const int32_t* order_idx, const int32_t* degree,
                                const double* coef, int fit_linear, int mode, int K,
                                int32_t* col_a, int32_t* col_b, double* val) {
    SPFM_GUARD(h);
    const spfm_engine::PairsCall c = {
        {n, indptr, indices, data, n_blocks, order_idx, degree, coef, fit_linear,
         SPFM_EXPLAIN_ATTRIBUTION, nullptr, nullptr, true, K, col_a, val},
        spfm_engine::PAIRS_TOPK, mode, 0, nullptr, nullptr, nullptr, col_b};
    return SPFM_DISPATCH(h->dtype, return h->pairs_run<T>("explain_pairs_topk_csr", c));
}

int spfm_explain_pairs_grouped_csr(spfm_handle h, int64_t n, const int64_t* indptr,
                                   const int32_t* indices, const double* data, int n_blocks,
                                   const int32_t* order_idx, const int32_t* degree,
                                   const double* coef, int fit_linear, int G,
                                   const int32_t* group, double* out_pairs, double* out_main) {
    SPFM_GUARD(h);
    const spfm_engine::PairsCall c = {
        {n, indptr, indices, data, n_blocks, order_idx, degree, coef, fit_linear,
         SPFM_EXPLAIN_ATTRIBUTION, nullptr, nullptr, false, 0, nullptr, nullptr},
        spfm_engine::PAIRS_GROUPED, SPFM_PAIRS_INTERACTION, G, group, out_pairs, out_main, nullptr};
    return SPFM_DISPATCH(h->dtype, return h->pairs_run<T>("explain_pairs_grouped_csr", c));
}

}  // extern "C"
