// spfm_engine_psgd_full.hip -- full-catalogue softmax route of the ranking fit: the
// checks, the towers' buffers and the launches of one minibatch.  The minibatch driver, the update
// and the Michelot passes stay in spfm_engine_psgd.hip, which calls full_launch through
// psgd_batches_tl's gradient callable (psgd_full_run).
#include "spfm_engine.hip.h"
#include "spfm_psgd_full.hip.h"

using namespace spfm;

// Argument checks of both entries, on the host, before any launch: the state of the handle, the
// sampler's B / C / positives, and every pair against them.  (The disjoint-column rule was checked
// by set_sampler for every context with a positive against every candidate.)
int spfm_engine::psgd_full_check(const char* what, int degree, int64_t batch_size,
                                 const int32_t* pairs, int64_t m) {
    const std::string ws = std::string(what) + ": ";
    if (dist()) FAIL(SPFM_ERR_UNSUPPORTED, ws + "several ranks are not supported");
    SPFM_TRY(refuse_det(what));
    SPFM_TRY(refuse_pairs_det(what));
    SPFM_TRY(psgd_ready(what, degree));
    if (!have_sampler)
        FAIL(SPFM_ERR_INVALID, ws + "call spfm_psgd_pairs_set_sampler first: it gives the "
                                    "contexts, the candidates and the forbidden set");
    if (m < 1 || !pairs || m > INT32_MAX)
        FAIL(SPFM_ERR_INVALID, ws + "pairs must hold 1 <= m < 2^31 rows of 2");
    if (batch_size < 1) FAIL(SPFM_ERR_INVALID, ws + "batch_size must be >= 1");
    for (int64_t q = 0; q < m; ++q) {
        const int64_t b = pairs[2 * q], c = (int64_t)pairs[2 * q + 1] - sm_nctx;
        if (b < 0 || b >= sm_nctx)
            FAIL(SPFM_ERR_INVALID, ws + "pair " + std::to_string(q) + " names no context row");
        if (c < 0 || c >= sm_ncand)
            FAIL(SPFM_ERR_INVALID,
                 ws + "pair " + std::to_string(q) + " names no candidate row [B, B + C)");
        const int32_t *lo = h_sm_posidx.data() + h_sm_posptr[(size_t)b],
                      *hi = h_sm_posidx.data() + h_sm_posptr[(size_t)b + 1];
        if (!std::binary_search(lo, hi, (int32_t)c))
            FAIL(SPFM_ERR_INVALID, ws + "pair " + std::to_string(q) +
                                       " is not stored in the sampler's positives");
    }
    if (std::min(batch_size, m) > ((int64_t)1 << 20))
        FAIL(SPFM_ERR_UNSUPPORTED, ws + "more than 2^20 positives in a minibatch");
    int64_t R = 0;
    for (int o = 0; o < n_orders; ++o) R += (int64_t)k * (degree - o - 1);
    const int64_t Rp = round_up(R + 1, 4), Cpad = round_up(sm_ncand, kIntTile);
    if (sm_ncand > ((int64_t)1 << 20))
        FAIL(SPFM_ERR_UNSUPPORTED, ws + "more than 2^20 candidates");
    if (2 * Cpad * Rp * (int64_t)sizeof(double) > ((int64_t)1 << 30))
        FAIL(SPFM_ERR_UNSUPPORTED, ws + "the catalogue tower and its gradient (2 x " +
                                       std::to_string(Cpad) + " x " + std::to_string(Rp) +
                                       " doubles) exceed the cap of 1 GiB");
    return SPFM_OK;
}

// The pair list on the device, the towers and the strip counts of the three tile passes: about
// 1024 workgroups each, from the shapes alone.  Everything is sized by min(batch_size, m) and C.
int spfm_engine::full_prepare(int degree, int64_t batch_size, const int32_t* pairs, int64_t m) {
    SPFM_TRY(ensure_pt());
    int R = 0;
    for (int o = 0; o < n_orders; ++o) R += k * (degree - o - 1);
    fl_R = R;
    fl_Rp = (int)round_up(R + 1, 4);
    fl_Bpad = (int)round_up(std::min(batch_size, m), kIntTile);
    fl_Cpad = (int)round_up(sm_ncand, kIntTile);
    const int Tt = fl_Bpad / kIntTile, Tc = fl_Cpad / kIntTile, nrc = (int)cdiv(fl_Rp, kIntTile);
    auto strips = [](int walked, int others, int& tiles, int& count) {
        const int want = std::max(1, std::min(walked, 1024 / std::max(1, others)));
        tiles = (int)cdiv(walked, want);
        count = (int)cdiv(walked, tiles);
    };
    strips(Tc, Tt, fl_st_tiles, fl_st_strips);
    strips(Tc, Tt * nrc, fl_gu_tiles, fl_gu_strips);
    strips(Tt, Tc * nrc, fl_gv_tiles, fl_gv_strips);
    const size_t bimg = sizeof(double) * (size_t)fl_Bpad * fl_Rp,
                 cimg = sizeof(double) * (size_t)fl_Cpad * fl_Rp,
                 bvec = sizeof(double) * fl_Bpad, cvec = sizeof(double) * fl_Cpad;
    DevBuf* bufs[] = {&fl_pairs, &fl_loss, &fl_U,  &fl_dU, &fl_Vc,  &fl_dVc,
                      &fl_cc,    &fl_part, &fl_mx, &fl_rz, &fl_spos};
    const size_t sizes[] = {sizeof(int32_t) * 2 * (size_t)m, sizeof(double) * (size_t)m, bimg, bimg,
                            cimg, cimg, cvec, 2 * bvec * fl_st_strips, bvec, bvec, bvec};
    bool moved = fl_fptr_seen != sm_fptr.p || fl_fidx_seen != sm_fidx.p;
    for (int i = 0; i < 11; ++i) {
        const void* old = bufs[i]->p;
        HIPC(bufs[i]->alloc(sizes[i]));
        moved = moved || bufs[i]->p != old;
    }
    if (moved) clear_graphs();
    fl_fptr_seen = sm_fptr.p;
    fl_fidx_seen = sm_fidx.p;
    SPFM_TRY(upload_to(fl_pairs.p, pairs, 2 * (size_t)m));
    HIPC(hipStreamSynchronize(stream));  // caller may reuse pairs
    return SPFM_OK;
}

// the positions [pos, pos + B) (table: the batch sg_idx[0] of sg_sched); eval: no gradient
template <typename T, int L>
void spfm_engine::full_launch_tl(int64_t pos, int B, bool table, int degree, int fit_linear,
                                 bool eval) {
    const PsgdBatch* sched = table ? sg_sched.as<PsgdBatch>() : (const PsgdBatch*)nullptr;
    int* idx = table ? sg_idx.as<int>() : (int*)nullptr;
    FullArgs a{};
    a.pairs = fl_pairs.as<int32_t>();
    a.fptr = sm_fptr.as<int64_t>();
    a.fidx = sm_fidx.as<int32_t>();
    a.U = fl_U.as<double>();
    a.dU = fl_dU.as<double>();
    a.Vc = fl_Vc.as<double>();
    a.dVc = fl_dVc.as<double>();
    a.cc = fl_cc.as<double>();
    a.part = fl_part.as<double>();
    a.mx = fl_mx.as<double>();
    a.rz = fl_rz.as<double>();
    a.spos = fl_spos.as<double>();
    a.R = fl_R;
    a.Rp = fl_Rp;
    a.Bpad = fl_Bpad;
    a.Cpad = fl_Cpad;
    a.B0 = (int)sm_nctx;
    a.C = (int)sm_ncand;
    a.st_tiles = fl_st_tiles;
    a.st_strips = fl_st_strips;
    a.gu_tiles = fl_gu_tiles;
    a.gu_strips = fl_gu_strips;
    a.gv_tiles = fl_gv_tiles;
    a.gv_strips = fl_gv_strips;
    const InbArgs ctx = full_ctx_view(a);
    const int Tt = fl_Bpad / kIntTile, Tc = fl_Cpad / kIntTile, nrc = (int)cdiv(fl_Rp, kIntTile);
    const long long p0 = (long long)pos;
    hipLaunchKernelGGL((inb_tower_kernel<T>), dim3(cdiv(fl_Bpad, kBlock / kWave), 1), dim3(kBlock),
                       0, stream, ctx, p0, B, sched, idx, rptr.as<int64_t>(), ridx.as<int32_t>(),
                       rval.as<T>(), Pt.as<double>(), w.as<double>(), lams.as<double>(), n_orders,
                       k, d, degree);
    hipLaunchKernelGGL((full_tower_kernel<T>), dim3(cdiv(fl_Cpad, kBlock / kWave)), dim3(kBlock), 0,
                       stream, a, rptr.as<int64_t>(), ridx.as<int32_t>(), rval.as<T>(),
                       Pt.as<double>(), w.as<double>(), lams.as<double>(), n_orders, k, d, degree);
    hipLaunchKernelGGL(full_stats_kernel, dim3(fl_st_strips, Tt), dim3(kBlock), 0, stream, a, p0, B,
                       sched, idx);
    hipLaunchKernelGGL(full_lse_kernel, dim3(cdiv(fl_Bpad, kBlock)), dim3(kBlock), 0, stream, a, p0,
                       B, sched, idx, fl_loss.as<double>());
    if (eval) return;
    hipLaunchKernelGGL((full_grad_tile_kernel<false>), dim3(fl_gu_strips, Tt, nrc), dim3(kBlock), 0,
                       stream, a, p0, B, sched, idx);
    hipLaunchKernelGGL((full_grad_tile_kernel<true>), dim3(fl_gv_strips, Tc, nrc), dim3(kBlock), 0,
                       stream, a, p0, B, sched, idx);
    hipLaunchKernelGGL((inb_back_kernel<T, L>), dim3(cdiv(fl_Bpad, kBlock / L), 1), dim3(kBlock), 0,
                       stream, ctx, p0, B, sched, idx, rptr.as<int64_t>(), ridx.as<int32_t>(),
                       rval.as<T>(), Pt.as<double>(), lams.as<double>(), n_orders, k, d, degree,
                       fit_linear, sg_gradP.as<double>(), sg_gradw.as<double>());
    hipLaunchKernelGGL((full_back_kernel<T, L>), dim3(cdiv(sm_ncand, kBlock / L)), dim3(kBlock), 0,
                       stream, a, rptr.as<int64_t>(), ridx.as<int32_t>(), rval.as<T>(),
                       Pt.as<double>(), lams.as<double>(), n_orders, k, d, degree, fit_linear,
                       sg_gradP.as<double>(), sg_gradw.as<double>());
}

void spfm_engine::full_launch(int64_t pos, int B, bool table, int degree, int fit_linear,
                              bool eval) {
    SPFM_DISPATCH(dtype, SPFM_DISPATCH_L(k, full_launch_tl<T, L>(pos, B, table, degree,
                                                                  fit_linear, eval)));
}

int spfm_engine::psgd_full_epoch(const PsgdStep& st, const int32_t* pairs, int64_t m,
                                 double* sum_loss) {
    SPFM_TRY(psgd_full_check("psgd full", st.degree, st.batch_size < 1 ? 1 : st.batch_size, pairs,
                             m));
    if (const std::string e = st.check("psgd full"); !e.empty()) FAIL(SPFM_ERR_INVALID, e);
    SPFM_TRY(full_prepare(st.degree, st.batch_size, pairs, m));
    SPFM_TRY(psgd_full_run(st, m));
    return psgd_epoch_end(fl_loss.as<double>(), m, sum_loss);
}

// the towers, the statistics and the losses of every minibatch at the live parameters
int spfm_engine::psgd_full_eval(int degree, int64_t batch_size, const int32_t* pairs, int64_t m,
                                double* sum_loss) {
    SPFM_TRY(psgd_full_check("psgd full eval", degree, batch_size, pairs, m));
    if (sum_loss) *sum_loss = 0.0;
    SPFM_TRY(full_prepare(degree, batch_size, pairs, m));
    for (int64_t pos = 0; pos < m; pos += batch_size)
        full_launch(pos, (int)std::min<int64_t>(batch_size, m - pos), false, degree, 0, true);
    loss_sum(fl_loss.as<double>(), m, 0);
    HIPC(hipGetLastError());
    SPFM_TRY(download(h_scalar, scalar.p, 1));
    HIPC(hipStreamSynchronize(stream));
    if (sum_loss) *sum_loss = h_scalar[0];
    return SPFM_OK;
}

extern "C" {

int spfm_psgd_full_epoch(spfm_handle h, int degree, double alpha, double beta, double gamma,
                         double eta0, int learning_rate, double power_t, int64_t batch_size,
                         const int32_t* pairs, int64_t m, int fit_linear, int64_t* it,
                         double* sum_loss) {
    SPFM_GUARD(h);
    const PsgdStep st = h->psgd_step(degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                                      batch_size, fit_linear, it);
    return h->psgd_full_epoch(st, pairs, m, sum_loss);
}

int spfm_psgd_full_eval(spfm_handle h, int degree, int64_t batch_size, const int32_t* pairs,
                        int64_t m, double* sum_loss) {
    SPFM_GUARD(h);
    return h->psgd_full_eval(degree, batch_size, pairs, m, sum_loss);
}

}  // extern "C"
