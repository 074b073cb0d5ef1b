// spfm_engine_explain.hip -- spfm_explain_csr / _topk_csr / _set_partition / _info
// (include/spfm.h): why a row got its prediction.  Per stored entry the exact Shapley value
// against a zero baseline, or the input gradient; per row their sum and the K largest
// (spfm_explain.hip.h).  Read-only like predict: the (d,k) image is refreshed the way
// spfm_predict_csr does it, everything else is scratch of this unit.  Rows go through in slabs
// bounded by stored entries.  See DESIGN.md section 16.
#include "spfm_engine.hip.h"
#include "spfm_explain.hip.h"

#include <algorithm>

static_assert(kExplainMaxK == SPFM_EXPLAIN_MAX_K, "header and device agree on the cap");
static_assert(EXPLAIN_ATTRIBUTION == SPFM_EXPLAIN_ATTRIBUTION &&
                  EXPLAIN_GRADIENT == SPFM_EXPLAIN_GRADIENT,
              "header and device agree on the modes");
static_assert(kExplainCoefs == SPFM_MAX_DEGREE + 1, "one coefficient per order 0..6");

namespace {
// One slab's scratch: 4 (column) + at most 8 (value) + 8 (result) bytes per stored entry, and
// 16 + 12 K bytes per row (offset, row sum, top-K list).  Entries take at most 160 MiB of the
// 256 MiB budget, the rows of a slab are capped by what is left.
constexpr int64_t kExplainBudget = 256ll << 20;
constexpr int64_t kExplainEntryBytes = 20;
}  // namespace

void spfm_engine::explain_release() {
    for (DevBuf* b : {&ex_rp, &ex_ri, &ex_rv, &ex_out, &ex_rs, &ex_coef, &ex_ti, &ex_tv, &ex_pp,
                      &ex_pv, &ex_grp, &ex_gp, &ex_gm})
        b->release();
}

int spfm_engine::explain_check_model(const char* what, const ExplainCall& c) {
    const std::string w(what);
    if (!have_params) FAIL(SPFM_ERR_INVALID, w + ": no parameters set");
    if (c.n_blocks < 0 || (c.n_blocks > 0 && (!c.order_idx || !c.degree || !c.coef)))
        FAIL(SPFM_ERR_INVALID, w + ": bad arguments");
    for (int q = 0; q < c.n_blocks; ++q) {
        if (c.degree[q] < 2 || c.degree[q] > SPFM_MAX_DEGREE)
            FAIL(SPFM_ERR_UNSUPPORTED, w + ": degree outside 2..6");
        if (c.order_idx[q] < 0 || c.order_idx[q] >= n_orders)
            FAIL(SPFM_ERR_INVALID, w + ": order_idx outside the parameters");
    }
    return SPFM_OK;
}

int spfm_engine::explain_check_rows(const char* what, const ExplainCall& c) {
    return check_csr(what, c.n, c.indptr, c.indices, c.data, d, INT32_MAX);
}

// every check of the two entries, before any device work and before any output is written
int spfm_engine::explain_check(const char* what, const ExplainCall& c) {
    const std::string w(what);
    SPFM_TRY(explain_check_model(what, c));
    if (c.mode != SPFM_EXPLAIN_ATTRIBUTION && c.mode != SPFM_EXPLAIN_GRADIENT)
        FAIL(SPFM_ERR_INVALID, w + ": mode must be SPFM_EXPLAIN_ATTRIBUTION or _GRADIENT");
    if (c.topk) {
        if (c.K < 1) FAIL(SPFM_ERR_INVALID, w + ": K must be >= 1");
        if (c.K > SPFM_EXPLAIN_MAX_K) {
            char buf[96];
            snprintf(buf, sizeof buf, "%s: K must be <= SPFM_EXPLAIN_MAX_K = %d", what,
                     (int)SPFM_EXPLAIN_MAX_K);
            FAIL(SPFM_ERR_UNSUPPORTED, buf);
        }
    }
    SPFM_TRY(explain_check_rows(what, c));
    if (c.n > 0 && c.topk && (!c.idx || !c.val)) FAIL(SPFM_ERR_INVALID, w + ": NULL output");
    if (c.n > 0 && !c.topk && c.indptr[c.n] > 0 && !c.out_vals)
        FAIL(SPFM_ERR_INVALID, w + ": out_vals is NULL");
    return SPFM_OK;
}

template <typename T, int M>
void spfm_engine::explain_launch_block(int64_t rows, int64_t e0, const double* Pt_o,
                                       const double* coef_o, int mode) {
    hipLaunchKernelGGL((explain_block_kernel<T, M>), dim3(cdiv(rows, kBlock / kWave)),
                       dim3(kBlock), 0, stream, rows, k, e0, ex_rp.as<int64_t>(),
                       ex_ri.as<int32_t>(), ex_rv.as<T>(), Pt_o, lams.as<double>(), coef_o, mode,
                       ex_out.as<double>());
}

// rows [r0, r1): stage, linear term, the blocks in the caller's order, row sums, top-K, copy back
template <typename T>
int spfm_engine::explain_slab(const ExplainCall& c, int64_t r0, int64_t r1) {
    const int64_t rows = r1 - r0, e0 = c.indptr[r0], ne = c.indptr[r1] - e0;
    HIPC(ex_out.alloc(sizeof(double) * (size_t)ne));
    if (c.out_rowsum) HIPC(ex_rs.alloc(sizeof(double) * (size_t)rows));
    if (c.K > 0) {
        HIPC(ex_ti.alloc(sizeof(int32_t) * (size_t)rows * c.K));
        HIPC(ex_tv.alloc(sizeof(double) * (size_t)rows * c.K));
    }
    std::vector<T> hv;  // staging of the values
    DeviceTimer timer;
    const auto enqueue = [&]() -> int {
        SPFM_TRY(stage_csr_rows<T>(ex_rp, ex_ri, ex_rv, hv, c.indptr, c.indices, c.data, r0, r1));
        timer.begin(stream);
        if (ne > 0) {
            hipLaunchKernelGGL((explain_init_kernel<T>), dim3(cdiv(ne, kBlock)), dim3(kBlock), 0,
                               stream, ne, ex_ri.as<int32_t>(), ex_rv.as<T>(),
                               c.fit_linear ? w.as<double>() : (const double*)nullptr, c.mode,
                               ex_out.as<double>());
            for (int q = 0; q < c.n_blocks; ++q) {
                const double* Pt_o = Pt.as<double>() + (size_t)c.order_idx[q] * k * d;
                const double* coef_o = ex_coef.as<double>() + (size_t)q * k * kExplainCoefs;
                (void)SPFM_DISPATCH_KIND(  // (2..6: explain_check_model)
                    c.degree[q], false, explain_launch_block<T, M>(rows, e0, Pt_o, coef_o, c.mode));
            }
        }
        const unsigned row_waves = cdiv(rows * kWave, kBlock);
        if (c.out_rowsum)
            hipLaunchKernelGGL(explain_rowsum_kernel, dim3(row_waves), dim3(kBlock), 0, stream,
                               rows, e0, ex_rp.as<int64_t>(), ex_out.as<double>(),
                               ex_rs.as<double>());
        if (c.K > 0)
            hipLaunchKernelGGL(explain_topk_kernel, dim3(row_waves), dim3(kBlock), 0, stream, rows,
                               e0, ex_rp.as<int64_t>(), ex_ri.as<int32_t>(), ex_out.as<double>(),
                               c.K, ex_ti.as<int32_t>(), ex_tv.as<double>());
        HIPC(hipGetLastError());
        timer.end(stream);
        if (c.out_vals) SPFM_TRY(download(c.out_vals + e0, ex_out.p, (size_t)ne));
        if (c.out_rowsum) SPFM_TRY(download(c.out_rowsum + r0, ex_rs.p, (size_t)rows));
        if (c.K > 0) {
            SPFM_TRY(download(c.idx + (size_t)r0 * c.K, ex_ti.p, (size_t)rows * c.K));
            SPFM_TRY(download(c.val + (size_t)r0 * c.K, ex_tv.p, (size_t)rows * c.K));
        }
        return SPFM_OK;
    };
    return run_staged(enqueue, &timer, &ex_device_us);
}

template <typename T>
int spfm_engine::explain_run(const char* what, const ExplainCall& c) {
    SPFM_TRY(explain_check(what, c));
    if (c.n == 0) return SPFM_OK;
    SPFM_TRY(ensure_p());
    pt_valid = false;  // P is the source of truth here, as in output_t
    SPFM_TRY(ensure_pt());
    SPFM_TRY(upload(ex_coef, c.coef, (size_t)c.n_blocks * k * kExplainCoefs));
    const int64_t slab_nnz = ex_slab_nnz > 0 ? ex_slab_nnz : kExplainSlabMax;
    const int64_t row_cap = std::max<int64_t>(
        1, (kExplainBudget - kExplainEntryBytes * slab_nnz) / (16 + 12 * (int64_t)c.K));
    ex_device_us = 0;
    ex_slabs = 0;
    for (int64_t r0 = 0; r0 < c.n;) {
        const int64_t r1 = slab_end(r0, c.n, row_cap, {c.indptr, slab_nnz});
        SPFM_TRY(explain_slab<T>(c, r0, r1));
        ++ex_slabs;
        r0 = r1;
    }
    return SPFM_OK;
}

extern "C" {

int spfm_explain_csr(spfm_handle h, int64_t n, const int64_t* indptr, const int32_t* indices,
                     const double* data, int n_blocks, const int32_t* order_idx,
                     const int32_t* degree, const double* coef, int fit_linear, int mode,
                     double* out_vals, double* out_rowsum) {
    SPFM_GUARD(h);
    const spfm_engine::ExplainCall c = {n, indptr, indices, data, n_blocks, order_idx, degree,
                                        coef, fit_linear, mode, out_vals, out_rowsum, false, 0,
                                        nullptr, nullptr};
    return SPFM_DISPATCH(h->dtype, return h->explain_run<T>("explain_csr", c));
}

int spfm_explain_topk_csr(spfm_handle h, int64_t n, const int64_t* indptr, const int32_t* indices,
                          const double* data, int n_blocks, const int32_t* order_idx,
                          const int32_t* degree, const double* coef, int fit_linear, int K,
                          int32_t* idx, double* val) {
    SPFM_GUARD(h);
    const spfm_engine::ExplainCall c = {n, indptr, indices, data, n_blocks, order_idx, degree,
                                        coef, fit_linear, SPFM_EXPLAIN_ATTRIBUTION, nullptr,
                                        nullptr, true, K, idx, val};
    return SPFM_DISPATCH(h->dtype, return h->explain_run<T>("explain_topk_csr", c));
}

int spfm_explain_set_partition(spfm_handle h, int64_t slab_nnz) {
    if (!h) return SPFM_ERR_INVALID;
    if (slab_nnz < 0 || slab_nnz > spfm_engine::kExplainSlabMax) {
        h->err = "explain_set_partition: slab_nnz must be in [0, 2^23]";
        return SPFM_ERR_INVALID;
    }
    h->ex_slab_nnz = slab_nnz;
    return SPFM_OK;
}

int spfm_explain_info(spfm_handle h, int64_t* out4) {
    if (!h || !out4) return SPFM_ERR_INVALID;
    out4[0] = (int64_t)h->explain_scratch_bytes();
    out4[1] = h->ex_device_us;
    out4[2] = h->ex_slab_nnz;
    out4[3] = h->ex_slabs;
    return SPFM_OK;
}

}  // extern "C"
