// spfm_engine_psgd_ftrl.hip -- FTRL-Proximal steps of the minibatch unit:
// the handle's state, its setter and getter, and the launch of the lazy update that the batch
// driver of spfm_engine_psgd.hip calls in FTRL mode.  A unit of its own: built without packed-fp32
// instructions, and the units of the other update kernels keep their flags.
#include "spfm_engine.hip.h"
#include "spfm_predict.hip.h"  // transpose_kernel
#include "spfm_psgd_ftrl.hip.h"

using namespace spfm;

void spfm_engine::psgd_ftrl_update(int grid, int fit_linear, const PsgdBatch& b,
                                   const PsgdBatch* sched, int* idx) {
    SPFM_DISPATCH_L(k, hipLaunchKernelGGL(
        (psgd_update_ftrl_kernel<L>), dim3(grid), dim3(kBlock), 0, stream, Pt.as<double>(),
        sg_gradP.as<double>(), w.as<double>(), sg_gradw.as<double>(), ft_zP.as<double>(),
        ft_nP.as<double>(), ft_zw.as<double>(), ft_nw.as<double>(), n_orders, k, d, reg,
        fit_linear, b, sched, idx));
}

// Mode 0 only switches the rule off: nothing else is read, the state stays.  Mode 1 with all four
// arrays: the state to go on from (z_P as P is given, (n_orders, k, d)); with none: n = 0 and z
// derived from the live parameters.  A moved buffer changes the recorded kernel arguments.
int spfm_engine::psgd_set_ftrl(int mode, double g0, double eta0, double alpha, double beta,
                               double gamma, const double* z_P, const double* z_w,
                               const double* n_P, const double* n_w) {
    if (mode != 0 && mode != 1)
        FAIL(SPFM_ERR_INVALID, "set_ftrl: mode must be 0 (off) or 1 (FTRL-Proximal)");
    if (mode == 0) {
        psgd_ftrl = 0;
        return SPFM_OK;
    }
    if (!(g0 > 0.0) || !std::isfinite(g0))
        FAIL(SPFM_ERR_INVALID, "set_ftrl: G0 must be positive and finite");
    if (!(eta0 > 0.0) || !std::isfinite(eta0))
        FAIL(SPFM_ERR_INVALID, "set_ftrl: eta0 must be positive and finite");
    if (!std::isfinite(alpha) || !std::isfinite(beta) || !std::isfinite(gamma))
        FAIL(SPFM_ERR_INVALID, "set_ftrl: alpha, beta and gamma must be finite");
    if (!have_params) FAIL(SPFM_ERR_INVALID, "set_ftrl: set the parameters first");
    if (!configured || solver != SPFM_SOLVER_PSGD)
        FAIL(SPFM_ERR_INVALID, "set_ftrl: configure the handle for psgd first (the starting z "
                               "depends on the regularizer)");
    const int given = (z_P != nullptr) + (z_w != nullptr) + (n_P != nullptr) + (n_w != nullptr);
    if (given != 0 && given != 4)
        FAIL(SPFM_ERR_INVALID, "set_ftrl: give z_P, z_w, n_P and n_w together or none of them");
    const size_t nP = (size_t)n_orders * d, nw = (size_t)d, nz = nP * k;
    for (size_t i = 0; n_P && i < nP; ++i)
        if (!(n_P[i] >= 0.0) || !std::isfinite(n_P[i]))
            FAIL(SPFM_ERR_INVALID, "set_ftrl: n_P holds a negative or non-finite value");
    for (size_t i = 0; n_w && i < nw; ++i)
        if (!(n_w[i] >= 0.0) || !std::isfinite(n_w[i]))
            FAIL(SPFM_ERR_INVALID, "set_ftrl: n_w holds a negative or non-finite value");
    // from here on the buffers are rewritten: a failure below leaves the mode off and no state
    psgd_ftrl = 0;
    ftrl_d = 0;
    const void *o1 = ft_zP.p, *o2 = ft_zw.p, *o3 = ft_nP.p, *o4 = ft_nw.p;
    HIPC(ft_zP.alloc(sizeof(double) * nz));
    HIPC(ft_zw.alloc(sizeof(double) * nw));
    HIPC(ft_nP.alloc(sizeof(double) * nP));
    HIPC(ft_nw.alloc(sizeof(double) * nw));
    if (ft_zP.p != o1 || ft_zw.p != o2 || ft_nP.p != o3 || ft_nw.p != o4) clear_graphs();
    if (given) {
        HIPC(ft_stage.alloc(sizeof(double) * nz));
        SPFM_TRY(upload_to(ft_stage.p, z_P, nz));
        for (int o = 0; o < n_orders; ++o) {  // (k, d) as given -> (d, k) as the kernels read it
            const size_t off = (size_t)o * k * d;
            hipLaunchKernelGGL(transpose_kernel, dim3(cdiv((int64_t)k * d, 256)), dim3(256), 0,
                               stream, ft_stage.as<double>() + off, k, d,
                               ft_zP.as<double>() + off);
        }
        SPFM_TRY(upload_to(ft_zw.p, z_w, nw));
        SPFM_TRY(upload_to(ft_nP.p, n_P, nP));
        SPFM_TRY(upload_to(ft_nw.p, n_w, nw));
    } else {
        SPFM_TRY(ensure_pt());  // (P stays valid: nothing is written to either image)
        const int reg_ = reg;
        SPFM_DISPATCH_L(k, hipLaunchKernelGGL(
            (psgd_ftrl_init_kernel<L>),
            dim3((int)std::min<int64_t>(kPsgdNB, cdiv(d, kBlock / L))), dim3(kBlock), 0, stream,
            Pt.as<double>(), w.as<double>(), ft_zP.as<double>(), ft_nP.as<double>(),
            ft_zw.as<double>(), ft_nw.as<double>(), n_orders, k, d, reg_, g0, eta0, alpha, beta,
            gamma));
    }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(stream));  // the caller may reuse its arrays
    ft_stage.release();
    ftrl_orders = n_orders;
    ftrl_d = d;
    ftrl_k = k;
    psgd_ftrl = 1;
    ftrl_g0 = g0;
    return SPFM_OK;
}

int spfm_engine::psgd_get_ftrl(int* mode, double* g0, double* z_P, double* z_w, double* n_P,
                               double* n_w) {
    if (mode) *mode = psgd_ftrl;
    if (g0) *g0 = ftrl_g0;
    if (!z_P && !z_w && !n_P && !n_w) return SPFM_OK;
    if (ftrl_d == 0) FAIL(SPFM_ERR_INVALID, "get_ftrl: spfm_psgd_set_ftrl was not called");
    const size_t per = (size_t)ftrl_k * ftrl_d;
    if (z_P) {
        HIPC(ft_stage.alloc(sizeof(double) * per * ftrl_orders));
        for (int o = 0; o < ftrl_orders; ++o)
            hipLaunchKernelGGL(transpose_kernel, dim3(cdiv((int64_t)per, 256)), dim3(256), 0,
                               stream, ft_zP.as<double>() + per * o, ftrl_d, ftrl_k,
                               ft_stage.as<double>() + per * o);
        HIPC(hipGetLastError());
        SPFM_TRY(download(z_P, ft_stage.p, per * ftrl_orders));
    }
    if (z_w) SPFM_TRY(download(z_w, ft_zw.p, (size_t)ftrl_d));
    if (n_P) SPFM_TRY(download(n_P, ft_nP.p, (size_t)ftrl_orders * ftrl_d));
    if (n_w) SPFM_TRY(download(n_w, ft_nw.p, (size_t)ftrl_d));
    HIPC(hipStreamSynchronize(stream));
    ft_stage.release();
    return SPFM_OK;
}

extern "C" {

int spfm_psgd_set_ftrl(spfm_handle h, int mode, double G0, double eta0, double alpha, double beta,
                       double gamma, const double* z_P, const double* z_w, const double* n_P,
                       const double* n_w) {
    SPFM_GUARD(h);
    return h->psgd_set_ftrl(mode, G0, eta0, alpha, beta, gamma, z_P, z_w, n_P, n_w);
}

int spfm_psgd_get_ftrl(spfm_handle h, int* mode, double* G0, double* z_P, double* z_w,
                       double* n_P, double* n_w) {
    SPFM_GUARD(h);
    return h->psgd_get_ftrl(mode, G0, z_P, z_w, n_P, n_w);
}

}  // extern "C"
