// spfm_engine_objective.hip -- spfm_objective_terms, spfm_set_eval_csr, spfm_eval_loss
// (include/spfm.h): what is being minimised and what the regularizer has switched off, from the
// live device parameters, and the loss on a second, resident CSR matrix.  All three are read-only
// views: scratch buffers of their own, no change to the P / Pt validity flags, to y_pred, the
// regularizer state or the schedule.  See DESIGN.md section 13.
#include "spfm_engine.hip.h"
#include "spfm_objective.hip.h"
#include "spfm_predict.hip.h"

template <int M>
int spfm_engine::objective_launch(const double* base, int64_t ss, int64_t sj, int kk,
                                  int all_subsets, int is_w) {
    const int nblk = (int)cdiv(d, kObjTile);
    HIPC(obj_rec.alloc(sizeof(double) * (size_t)nblk * (kk + 1) * kObjRec));
    HIPC(obj_fin.alloc(sizeof(double) * (size_t)(kk + 1) * kObjRec));
    HIPC(obj_out.alloc(sizeof(double) * 8));
    hipLaunchKernelGGL((obj_block_kernel<M>), dim3(nblk), dim3(kBlock), 0, stream, base, ss, sj,
                       kk, d, obj_rec.as<double>());
    hipLaunchKernelGGL((obj_finish_kernel<M>), dim3(1), dim3(kBlock), 0, stream,
                       obj_rec.as<double>(), nblk, kk, reg, all_subsets, is_w,
                       obj_fin.as<double>(), obj_out.as<double>());
    HIPC(hipGetLastError());
    return SPFM_OK;
}

int spfm_engine::objective_terms(int order_idx, int degree, double* out8) {
    if (!out8) FAIL(SPFM_ERR_INVALID, "objective_terms: out8 is NULL");
    if (!have_params) FAIL(SPFM_ERR_INVALID, "objective_terms: no parameters set");
    if (!configured)
        FAIL(SPFM_ERR_INVALID, "objective_terms: call spfm_configure first (regularizer kind)");
    if (degree != -1 && (degree < 1 || degree > SPFM_MAX_DEGREE))
        FAIL(SPFM_ERR_UNSUPPORTED, "objective_terms: degree must be 1..6 or -1 (all-subsets)");
    if (order_idx < -1 || order_idx >= n_orders)
        FAIL(SPFM_ERR_INVALID, "objective_terms: bad order index");
    int rc;
    if (order_idx == -1) {
        rc = objective_launch<0>(w.as<double>(), 0, 1, 1, 0, 1);
    } else {
        const BlockView v = live_block(order_idx);
        const bool poly = (reg == SPFM_REG_OMEGATI || reg == SPFM_REG_OMEGACS) && degree > 0;
        const int all = degree == -1;
        switch (poly ? degree : 0) {
            case 0: rc = objective_launch<0>(v.base, v.ss, v.sj, k, all, 0); break;
            case 1: rc = objective_launch<1>(v.base, v.ss, v.sj, k, all, 0); break;
            case 2: rc = objective_launch<2>(v.base, v.ss, v.sj, k, all, 0); break;
            case 3: rc = objective_launch<3>(v.base, v.ss, v.sj, k, all, 0); break;
            case 4: rc = objective_launch<4>(v.base, v.ss, v.sj, k, all, 0); break;
            case 5: rc = objective_launch<5>(v.base, v.ss, v.sj, k, all, 0); break;
            default: rc = objective_launch<6>(v.base, v.ss, v.sj, k, all, 0); break;
        }
    }
    if (rc) return rc;
    SPFM_TRY(download(out8, obj_out.p, 8));
    return sync();
}

template <typename T>
int spfm_engine::set_eval_t(int64_t rows, const int64_t* indptr, const int32_t* indices,
                            const double* data, const double* y) {
    std::vector<T> hv;
    SPFM_TRY(stage_csr_rows(ev_rptr, ev_ridx, ev_rval, hv, indptr, indices, data, 0, rows));
    HIPC(ev_pred.alloc(sizeof(double) * (size_t)rows));
    HIPC(ev_part.alloc(sizeof(double) * 520));
    if (y) SPFM_TRY(upload(ev_y, y, (size_t)rows));
    return sync();  // hv and the caller's arrays are free again
}

int spfm_engine::set_eval_csr(int64_t rows, int32_t d_, const int64_t* indptr,
                              const int32_t* indices, const double* data, const double* y) {
    if (rows < 0 || d_ <= 0 || !indptr) FAIL(SPFM_ERR_INVALID, "set_eval: bad arguments");
    if (!have_data && !have_params)
        FAIL(SPFM_ERR_INVALID, "set_eval: set data or parameters first (n_features)");
    if (d_ != d) FAIL(SPFM_ERR_INVALID, "set_eval: n_features differs from the model's");
    if (rows >= (int64_t)1 << 31) FAIL(SPFM_ERR_UNSUPPORTED, "n_samples must be < 2^31");
    if (indptr[0] != 0) FAIL(SPFM_ERR_INVALID, "set_eval: indptr[0] != 0");
    for (int64_t i = 0; i < rows; ++i)
        if (indptr[i + 1] < indptr[i]) FAIL(SPFM_ERR_INVALID, "set_eval: indptr not monotone");
    if (indptr[rows] > 0 && (!indices || !data)) FAIL(SPFM_ERR_INVALID, "set_eval: bad arguments");
    for (int64_t i = 0; i < rows; ++i)
        for (int64_t ii = indptr[i]; ii < indptr[i + 1]; ++ii) {
            if (indices[ii] < 0 || indices[ii] >= d)
                FAIL(SPFM_ERR_INVALID, "set_eval: column index out of range");
            if (ii > indptr[i] && indices[ii] <= indices[ii - 1])
                FAIL(SPFM_ERR_INVALID,
                     "set_eval: CSR must have sorted, duplicate-free column indices");
        }
    have_eval = false;
    SPFM_TRY(SPFM_DISPATCH(dtype, return set_eval_t<T>(rows, indptr, indices, data, y)));
    ev_n = rows;
    ev_has_y = y != nullptr;
    have_eval = true;
    return SPFM_OK;
}

int spfm_engine::eval_loss(int degree, int fit_linear, int add_lower, double* loss_sum_out,
                           double* y_pred_out) {
    if (!have_params) FAIL(SPFM_ERR_INVALID, "eval_loss: no parameters set");
    if (!have_eval) FAIL(SPFM_ERR_INVALID, "eval_loss: call spfm_set_eval_csr first");
    if (degree != -1 && (degree < 1 || degree > SPFM_MAX_DEGREE))
        FAIL(SPFM_ERR_UNSUPPORTED, "eval_loss: degree must be 1..6 or -1 (all-subsets)");
    if (loss_sum_out && !ev_has_y)
        FAIL(SPFM_ERR_INVALID, "eval_loss: the held-out set has no targets");
    if (loss_sum_out && !configured)
        FAIL(SPFM_ERR_INVALID, "eval_loss: call spfm_configure first (loss kind)");
    if (loss_sum_out) *loss_sum_out = 0.0;
    if (ev_n == 0) return SPFM_OK;
    // the predict pass wants the (d,k) image: the live one, or a transpose of the live (k,d) image
    // into a buffer of this call's own (Pt and the validity flags stay as the epochs left them)
    const double* Pt_all = Pt.as<double>();
    if (!pt_valid) {
        HIPC(ev_pt.alloc(sizeof(double) * (size_t)n_orders * k * d));
        for (int o = 0; o < n_orders; ++o) {
            const size_t off = (size_t)o * k * d;
            hipLaunchKernelGGL(transpose_kernel, dim3(cdiv((int64_t)k * d, 256)), dim3(256), 0,
                               stream, P.as<double>() + off, k, d, ev_pt.as<double>() + off);
        }
        HIPC(hipGetLastError());
        Pt_all = ev_pt.as<double>();
    }
    SPFM_TRY(SPFM_DISPATCH(
        dtype, return output_pt_t<T>(ev_n, ev_rptr.as<int64_t>(), ev_ridx.as<int32_t>(),
                                     ev_rval.as<T>(), degree, fit_linear, add_lower, Pt_all,
                                     ev_pred.as<double>())));
    double total = 0.0;
    if (loss_sum_out) {
        const int nb = 512;
        hipLaunchKernelGGL(eval_loss_partial_kernel, dim3(nb), dim3(kBlock), 0, stream, ev_n,
                           ev_pred.as<double>(), ev_y.as<double>(), loss, ev_part.as<double>());
        hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(kBlock), 0, stream,
                           ev_part.as<double>(), nb, ev_part.as<double>() + 512);
        HIPC(hipGetLastError());
        SPFM_TRY(download(&total, ev_part.as<double>() + 512, 1));
    }
    if (y_pred_out) SPFM_TRY(download(y_pred_out, ev_pred.p, (size_t)ev_n));
    SPFM_TRY(sync());
    if (loss_sum_out) *loss_sum_out = total;
    return SPFM_OK;
}

extern "C" {

int spfm_objective_terms(spfm_handle h, int order_idx, int degree, double* out8) {
    SPFM_GUARD(h);
    return h->objective_terms(order_idx, degree, out8);
}

int spfm_set_eval_csr(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                      const int32_t* indices, const double* data, const double* y) {
    SPFM_GUARD(h);
    return h->set_eval_csr(n, d, indptr, indices, data, y);
}

int spfm_eval_loss(spfm_handle h, int degree, int fit_linear, int add_lower_deg2,
                   double* loss_sum, double* y_pred_out) {
    SPFM_GUARD(h);
    return h->eval_loss(degree, fit_linear, add_lower_deg2, loss_sum, y_pred_out);
}

}  // extern "C"
