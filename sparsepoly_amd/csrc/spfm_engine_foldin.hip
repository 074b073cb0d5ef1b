// spfm_engine_foldin.hip -- spfm_foldin_csr / _set_partition / _info (include/spfm.h): the
// parameters of single columns estimated with every other parameter fixed.  Per target column a
// small strictly convex problem (spfm_foldin.hip.h): the design rows of the rows that store the
// column, then one workgroup per column running a damped Newton iteration.  Read-only like
// explain: the (d,k) image is refreshed the way spfm_predict_csr does it, everything else is
// scratch of this unit.  Target columns go through in groups bounded by the rows of their design
// matrix.  See DESIGN.md section 18.
#include "spfm_engine.hip.h"
#include "spfm_foldin.hip.h"

#include <algorithm>

static_assert(kFoldinMaxUnknowns == SPFM_FOLDIN_MAX_UNKNOWNS, "header and device agree on the cap");
static_assert(kFoldinCoefs == SPFM_MAX_DEGREE + 1, "one coefficient per order 0..6");
static_assert(LOSS_SQUARED == SPFM_LOSS_SQUARED && LOSS_SQUARED_HINGE == SPFM_LOSS_SQUARED_HINGE &&
                  LOSS_LOGISTIC == SPFM_LOSS_LOGISTIC,
              "header and device agree on the losses");

void spfm_engine::foldin_release() {
    for (DevBuf* b : {&fi_rp, &fi_ri, &fi_rv, &fi_tp, &fi_y, &fi_Z, &fi_c, &fi_cp, &fi_coef,
                      &fi_theta, &fi_stat, &fi_it})
        b->release();
}

// every check, before any device work and before any output is written; leaves the row lists
int spfm_engine::foldin_check(const char* what, const FoldinCall& c, FoldinPlan& plan) {
    const std::string w(what);
    char buf[160];
    SPFM_TRY(explain_check_model(what, c.m));
    if (c.m.n_blocks < 1) FAIL(SPFM_ERR_INVALID, w + ": n_blocks must be >= 1");
    if (c.loss != SPFM_LOSS_SQUARED && c.loss != SPFM_LOSS_SQUARED_HINGE &&
        c.loss != SPFM_LOSS_LOGISTIC)
        FAIL(SPFM_ERR_INVALID, w + ": unknown loss");
    if (c.n_cols < 0 || (c.n_cols > 0 && !c.cols)) FAIL(SPFM_ERR_INVALID, w + ": bad cols");
    if (!(c.beta > 0.0) || !std::isfinite(c.beta)) FAIL(SPFM_ERR_INVALID, w + ": beta must be > 0");
    if (c.m.fit_linear && (!(c.alpha > 0.0) || !std::isfinite(c.alpha)))
        FAIL(SPFM_ERR_INVALID, w + ": alpha must be > 0 with a linear term");
    if (c.max_iter < 1) FAIL(SPFM_ERR_INVALID, w + ": max_iter must be >= 1");
    if (!(c.tol >= 0.0) || !std::isfinite(c.tol))
        FAIL(SPFM_ERR_INVALID, w + ": tol must be finite and >= 0");
    if (!std::isfinite(c.offset)) FAIL(SPFM_ERR_INVALID, w + ": offset must be finite");
    const int64_t R64 = (int64_t)c.m.n_blocks * k + (c.m.fit_linear ? 1 : 0);
    if (R64 > SPFM_FOLDIN_MAX_UNKNOWNS) {
        snprintf(buf, sizeof buf,
                 "%s: %lld unknowns per column, more than SPFM_FOLDIN_MAX_UNKNOWNS = %d", what,
                 (long long)R64, (int)SPFM_FOLDIN_MAX_UNKNOWNS);
        FAIL(SPFM_ERR_UNSUPPORTED, buf);
    }
    plan.R = (int)R64;
    plan.Rp = (int)round_up(R64, 4);
    SPFM_TRY(explain_check_rows(what, c.m));
    if (c.m.n > 0 && !c.y) FAIL(SPFM_ERR_INVALID, w + ": y is NULL");
    if (c.n_cols > 0 && (!c.theta || !c.n_rows || !c.n_iter || !c.converged || !c.grad_norm ||
                         !c.obj0 || !c.obj1))
        FAIL(SPFM_ERR_INVALID, w + ": NULL output");
    std::vector<int32_t> slot((size_t)d, -1);  // column -> its index in cols
    for (int64_t q = 0; q < c.n_cols; ++q) {
        const int32_t j = c.cols[q];
        if (j < 0 || j >= d) {
            snprintf(buf, sizeof buf, "%s: target column %d outside [0, %d)", what, (int)j, d);
            FAIL(SPFM_ERR_INVALID, buf);
        }
        if (slot[(size_t)j] >= 0) {
            snprintf(buf, sizeof buf, "%s: target column %d is listed twice", what, (int)j);
            FAIL(SPFM_ERR_INVALID, buf);
        }
        slot[(size_t)j] = (int32_t)q;
    }
    // the row -> target map: which column a row belongs to and where its entry stands
    std::vector<int32_t> owner((size_t)c.m.n, -1), pos((size_t)c.m.n, 0);
    plan.cptr.assign((size_t)c.n_cols + 1, 0);
    for (int64_t i = 0; i < c.m.n; ++i) {
        for (int64_t ii = c.m.indptr[i]; ii < c.m.indptr[i + 1]; ++ii) {
            const int32_t q = slot[(size_t)c.m.indices[ii]];
            if (q < 0) continue;
            if (owner[(size_t)i] >= 0) {
                snprintf(buf, sizeof buf,
                         "%s: row %lld stores two target entries (columns %d and %d): the "
                         "columns of one call must not share a row",
                         what, (long long)i, (int)c.cols[owner[(size_t)i]], (int)c.cols[q]);
                FAIL(SPFM_ERR_INVALID, buf);
            }
            owner[(size_t)i] = q;
            pos[(size_t)i] = (int32_t)(ii - c.m.indptr[i]);
        }
        if (owner[(size_t)i] >= 0) plan.cptr[(size_t)owner[(size_t)i] + 1]++;
    }
    const int64_t cap = kFoldinBudget / ((int64_t)sizeof(double) * plan.Rp);
    for (int64_t q = 0; q < c.n_cols; ++q) {
        if (plan.cptr[(size_t)q + 1] > cap) {
            snprintf(buf, sizeof buf,
                     "%s: target column %d has %lld rows, its design matrix exceeds the scratch "
                     "of %lld MiB",
                     what, (int)c.cols[q], (long long)plan.cptr[(size_t)q + 1],
                     (long long)(kFoldinBudget >> 20));
            FAIL(SPFM_ERR_UNSUPPORTED, buf);
        }
        plan.cptr[(size_t)q + 1] += plan.cptr[(size_t)q];
    }
    const int64_t np = plan.cptr[(size_t)c.n_cols];
    plan.rows.resize((size_t)np);
    plan.tpos.resize((size_t)np);
    std::vector<int64_t> fill(plan.cptr.begin(), plan.cptr.end() - 1);
    for (int64_t i = 0; i < c.m.n; ++i) {  // ascending rows: every column's list is ascending
        const int32_t q = owner[(size_t)i];
        if (q < 0) continue;
        const int64_t at = fill[(size_t)q]++;
        plan.rows[(size_t)at] = i;
        plan.tpos[(size_t)at] = pos[(size_t)i];
    }
    return SPFM_OK;
}

template <typename T, int M>
void spfm_engine::foldin_launch_design(int64_t rows, int q, const FoldinCall& c, int Rp) {
    const int lin = c.m.fit_linear ? 1 : 0;
    hipLaunchKernelGGL((foldin_design_kernel<T, M>), dim3(cdiv(rows, kBlock / kWave)),
                       dim3(kBlock), 0, stream, rows, k, c.m.n_blocks * k + lin, Rp, lin + q * k,
                       q == 0 ? 1 : 0, lin, c.offset, fi_rp.as<int64_t>(), fi_ri.as<int32_t>(),
                       fi_rv.as<T>(), fi_tp.as<int32_t>(),
                       Pt.as<double>() + (size_t)c.m.order_idx[q] * k * d, w.as<double>(),
                       lams.as<double>(), fi_coef.as<double>() + (size_t)q * k * kFoldinCoefs,
                       fi_Z.as<double>(), fi_c.as<double>());
}

// target columns [c0, c1): gather their rows, design, solve, copy back
template <typename T>
int spfm_engine::foldin_group(const FoldinCall& c, const FoldinPlan& plan, int64_t c0,
                              int64_t c1) {
    const int64_t ncg = c1 - c0, q0 = plan.cptr[(size_t)c0], rows = plan.cptr[(size_t)c1] - q0;
    const int R = plan.R, Rp = plan.Rp;
    // the group's rows as a CSR image of their own, in (column, row) order
    std::vector<int64_t> hp((size_t)rows + 1), hcp((size_t)ncg + 1);
    hp[0] = 0;
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t i = plan.rows[(size_t)(q0 + r)];
        hp[(size_t)r + 1] = hp[(size_t)r] + (c.m.indptr[i + 1] - c.m.indptr[i]);
    }
    const int64_t ne = hp[(size_t)rows];
    std::vector<int32_t> hi((size_t)ne);
    std::vector<T> hv((size_t)ne);
    std::vector<double> hy((size_t)rows);
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t i = plan.rows[(size_t)(q0 + r)], b = c.m.indptr[i];
        const int64_t len = c.m.indptr[i + 1] - b;
        std::copy(c.m.indices + b, c.m.indices + b + len, hi.begin() + hp[(size_t)r]);
        for (int64_t u = 0; u < len; ++u) hv[(size_t)(hp[(size_t)r] + u)] = (T)c.m.data[b + u];
        hy[(size_t)r] = c.y[i];
    }
    for (int64_t q = 0; q <= ncg; ++q) hcp[(size_t)q] = plan.cptr[(size_t)(c0 + q)] - q0;
    std::vector<double> hth((size_t)ncg * R), hst((size_t)ncg * 3);
    std::vector<int32_t> hit((size_t)ncg * 2);
    HIPC(fi_Z.alloc(sizeof(double) * (size_t)rows * Rp));
    HIPC(fi_c.alloc(sizeof(double) * (size_t)rows));
    HIPC(fi_theta.alloc(sizeof(double) * (size_t)ncg * R));
    HIPC(fi_stat.alloc(sizeof(double) * (size_t)ncg * 3));
    HIPC(fi_it.alloc(sizeof(int32_t) * (size_t)ncg * 2));
    const size_t lds = sizeof(double) * foldin_solve_lds(R, Rp);
    HIPC(hipFuncSetAttribute((const void*)foldin_solve_kernel,
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    DeviceTimer timer;
    const auto enqueue = [&]() -> int {
        SPFM_TRY(upload(fi_rp, hp.data(), hp.size()));
        SPFM_TRY(upload(fi_ri, hi.data(), hi.size()));
        SPFM_TRY(upload(fi_rv, hv.data(), hv.size()));
        SPFM_TRY(upload(fi_tp, plan.tpos.data() + q0, (size_t)rows));
        SPFM_TRY(upload(fi_y, hy.data(), hy.size()));
        SPFM_TRY(upload(fi_cp, hcp.data(), hcp.size()));
        timer.begin(stream);
        if (rows > 0)
            for (int q = 0; q < c.m.n_blocks; ++q)
                (void)SPFM_DISPATCH_KIND(c.m.degree[q], false,  // (2..6: explain_check_model)
                                         foldin_launch_design<T, M>(rows, q, c, Rp));
        const FoldinSolveArgs a = {R, Rp, c.m.fit_linear ? 1 : 0, c.loss, c.max_iter, c.alpha,
                                   c.beta, c.tol, fi_cp.as<int64_t>(), fi_Z.as<double>(),
                                   fi_c.as<double>(), fi_y.as<double>(), fi_theta.as<double>(),
                                   fi_stat.as<double>(), fi_it.as<int32_t>()};
        hipLaunchKernelGGL(foldin_solve_kernel, dim3((unsigned)ncg), dim3(kBlock), lds, stream, a);
        HIPC(hipGetLastError());
        timer.end(stream);
        SPFM_TRY(download(hth.data(), fi_theta.p, hth.size()));
        SPFM_TRY(download(hst.data(), fi_stat.p, hst.size()));
        SPFM_TRY(download(hit.data(), fi_it.p, hit.size()));
        return SPFM_OK;
    };
    SPFM_TRY(run_staged(enqueue, &timer, &fi_device_us));
    std::copy(hth.begin(), hth.end(), c.theta + (size_t)c0 * R);
    for (int64_t q = 0; q < ncg; ++q) {
        c.n_rows[c0 + q] = hcp[(size_t)q + 1] - hcp[(size_t)q];
        c.grad_norm[c0 + q] = hst[(size_t)q * 3];
        c.obj0[c0 + q] = hst[(size_t)q * 3 + 1];
        c.obj1[c0 + q] = hst[(size_t)q * 3 + 2];
        c.n_iter[c0 + q] = hit[(size_t)q * 2];
        c.converged[c0 + q] = hit[(size_t)q * 2 + 1];
    }
    return SPFM_OK;
}

template <typename T>
int spfm_engine::foldin_run(const char* what, const FoldinCall& c) {
    FoldinPlan plan;
    SPFM_TRY(foldin_check(what, c, plan));
    fi_device_us = 0;
    fi_groups = 0;
    const int64_t np = c.n_cols > 0 ? plan.cptr[(size_t)c.n_cols] : 0;
    fi_ignored = c.m.n - np;
    if (c.n_cols == 0) return SPFM_OK;
    if (np == 0) {  // no column has a row: theta = 0 minimises the ridge term alone
        std::fill(c.theta, c.theta + (size_t)c.n_cols * plan.R, 0.0);
        for (int64_t q = 0; q < c.n_cols; ++q) {
            c.n_rows[q] = 0;
            c.n_iter[q] = 0;
            c.converged[q] = 1;
            c.grad_norm[q] = c.obj0[q] = c.obj1[q] = 0.0;
        }
        return SPFM_OK;
    }
    SPFM_TRY(ensure_p());
    pt_valid = false;  // P is the source of truth here, as in output_t
    SPFM_TRY(ensure_pt());
    SPFM_TRY(upload(fi_coef, c.m.coef, (size_t)c.m.n_blocks * k * kFoldinCoefs));
    int64_t cap = kFoldinBudget / ((int64_t)sizeof(double) * plan.Rp);
    if (fi_max_rows > 0) cap = std::min(cap, fi_max_rows);
    for (int64_t c0 = 0; c0 < c.n_cols;) {
        // whole columns, bounded by the rows of their design matrix
        const int64_t c1 = slab_end(c0, c.n_cols, kSlabNoCap, {plan.cptr.data(), cap});
        SPFM_TRY(foldin_group<T>(c, plan, c0, c1));
        ++fi_groups;
        c0 = c1;
    }
    return SPFM_OK;
}

extern "C" {

int spfm_foldin_csr(spfm_handle h, int64_t n, const int64_t* indptr, const int32_t* indices,
                    const double* data, const double* y, int n_blocks, const int32_t* order_idx,
                    const int32_t* degree, const double* coef, int fit_linear, double offset,
                    int loss, int64_t n_cols, const int32_t* cols, double alpha, double beta,
                    int max_iter, double tol, double* theta, int64_t* n_rows, int32_t* n_iter,
                    int32_t* converged, double* grad_norm, double* obj0, double* obj1) {
    SPFM_GUARD(h);
    const spfm_engine::ExplainCall m = {n, indptr, indices, data, n_blocks, order_idx, degree,
                                        coef, fit_linear, 0, nullptr, nullptr, false, 0, nullptr,
                                        nullptr};
    const spfm_engine::FoldinCall c = {m, y, offset, loss, n_cols, cols, alpha, beta, max_iter,
                                       tol, theta, n_rows, n_iter, converged, grad_norm, obj0,
                                       obj1};
    return SPFM_DISPATCH(h->dtype, return h->foldin_run<T>("foldin_csr", c));
}

int spfm_foldin_set_partition(spfm_handle h, int64_t max_rows) {
    if (!h) return SPFM_ERR_INVALID;
    if (max_rows < 0) {
        h->err = "foldin_set_partition: max_rows must be >= 0";
        return SPFM_ERR_INVALID;
    }
    h->fi_max_rows = max_rows;
    return SPFM_OK;
}

int spfm_foldin_info(spfm_handle h, int64_t* out5) {
    if (!h || !out5) return SPFM_ERR_INVALID;
    out5[0] = (int64_t)h->foldin_scratch_bytes();
    out5[1] = h->fi_device_us;
    out5[2] = h->fi_max_rows;
    out5[3] = h->fi_groups;
    out5[4] = h->fi_ignored;
    return SPFM_OK;
}

}  // extern "C"
