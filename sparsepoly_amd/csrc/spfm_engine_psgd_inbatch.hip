// spfm_engine_psgd_inbatch.hip -- in-batch softmax route of the ranking fit: the
// checks, the per-minibatch images and the launches of its six kernels.  The minibatch driver, the
// update and the Michelot passes stay in spfm_engine_psgd.hip, which calls inbatch_launch through
// psgd_batches_tl's gradient callable (psgd_inbatch_run).
#include "spfm_engine.hip.h"
#include "spfm_psgd_inbatch.hip.h"

using namespace spfm;

// Argument checks of both entries, on the host, before any launch: the state of the handle, the
// row indices, and the disjoint-column rule of psgd_pairs_check (first_shared_column).
int spfm_engine::psgd_inbatch_check(const char* what, int degree, int64_t batch_size,
                                    const int32_t* pairs, int64_t m) {
    const std::string ws = std::string(what) + ": ";
    if (dist()) FAIL(SPFM_ERR_UNSUPPORTED, ws + "several ranks are not supported");
    SPFM_TRY(refuse_det(what));
    SPFM_TRY(refuse_pairs_det(what));
    SPFM_TRY(psgd_ready(what, degree));
    if (m < 1 || !pairs || m > INT32_MAX)
        FAIL(SPFM_ERR_INVALID, ws + "pairs must hold 1 <= m < 2^31 rows of 2");
    if (batch_size < 1) FAIL(SPFM_ERR_INVALID, ws + "batch_size must be >= 1");
    std::vector<uint8_t> side((size_t)(n > 0 ? n : 1), 0);  // 1: context, 2: candidate
    for (int64_t q = 0; q < m; ++q) {
        const int32_t b = pairs[2 * q], c = pairs[2 * q + 1];
        if (b < 0 || b >= n || c < 0 || c >= n)
            FAIL(SPFM_ERR_INVALID, ws + "pair " + std::to_string(q) + " names a row outside [0, n)");
        side[(size_t)b] |= 1;
        side[(size_t)c] |= 2;
    }
    const int32_t j = first_shared_column(side, d, h_cptr.data(), h_cidx.data());
    if (j >= 0)
        FAIL(SPFM_ERR_INVALID, ws + "column " + std::to_string(j) +
                                   " is stored in a context row and in a candidate row: the two "
                                   "column sets must be disjoint");
    if (std::min(batch_size, m) > ((int64_t)1 << 20))
        FAIL(SPFM_ERR_UNSUPPORTED, ws + "more than 2^20 positives in a minibatch");
    return SPFM_OK;
}

// The pair list on the device and the images of one minibatch (a moved buffer changes the
// recorded kernel arguments).  Everything is sized by min(batch_size, m), never by a batch.
int spfm_engine::inbatch_prepare(int degree, int64_t batch_size, const int32_t* pairs, int64_t m) {
    SPFM_TRY(ensure_pt());
    int R = 0;
    for (int o = 0; o < n_orders; ++o) R += k * (degree - o - 1);
    ib_R = R;
    ib_Rp = (int)round_up(R + 1, 4);
    ib_Bpad = (int)round_up(std::min(batch_size, m), kIntTile);
    const int T = ib_Bpad / kIntTile, nrc = (int)cdiv(ib_Rp, kIntTile);
    // about 1024 workgroups per tile pass: T row tiles x strips x column chunks of the images
    const int want = std::max(1, std::min(T, 1024 / std::max(1, T * nrc)));
    ib_strip_tiles = (int)cdiv(T, want);
    ib_nstrips = (int)cdiv(T, ib_strip_tiles);
    const size_t img = sizeof(double) * (size_t)ib_Bpad * ib_Rp, vec = sizeof(double) * ib_Bpad;
    DevBuf* bufs[] = {&ib_pairs, &ib_loss, &ib_U, &ib_V, &ib_dU, &ib_dV, &ib_cc,
                      &ib_part,  &ib_mx,   &ib_rz, &ib_diag};
    const size_t sizes[] = {sizeof(int32_t) * 2 * (size_t)m, sizeof(double) * (size_t)m, img, img,
                            img, img, vec, 2 * vec * ib_nstrips, vec, vec, vec};
    bool moved = false;
    for (int i = 0; i < 11; ++i) {
        const void* old = bufs[i]->p;
        HIPC(bufs[i]->alloc(sizes[i]));
        moved = moved || bufs[i]->p != old;
    }
    if (moved) clear_graphs();
    SPFM_TRY(upload_to(ib_pairs.p, pairs, 2 * (size_t)m));
    HIPC(hipStreamSynchronize(stream));  // caller may reuse pairs
    return SPFM_OK;
}

// the positions [pos, pos + B) (table: the batch sg_idx[0] of sg_sched); eval: no gradient
template <typename T, int L>
void spfm_engine::inbatch_launch_tl(int64_t pos, int B, bool table, int degree, int fit_linear,
                                    bool eval) {
    const PsgdBatch* sched = table ? sg_sched.as<PsgdBatch>() : (const PsgdBatch*)nullptr;
    int* idx = table ? sg_idx.as<int>() : (int*)nullptr;
    const InbArgs a{ib_pairs.as<int32_t>(), ib_U.as<double>(),    ib_V.as<double>(),
                    ib_cc.as<double>(),     ib_dU.as<double>(),   ib_dV.as<double>(),
                    ib_part.as<double>(),   ib_mx.as<double>(),   ib_rz.as<double>(),
                    ib_diag.as<double>(),   ib_R, ib_Rp, ib_Bpad, ib_strip_tiles, ib_nstrips};
    const int Tt = ib_Bpad / kIntTile, nrc = (int)cdiv(ib_Rp, kIntTile);
    const long long p0 = (long long)pos;
    hipLaunchKernelGGL((inb_tower_kernel<T>), dim3(cdiv(ib_Bpad, kBlock / kWave), 2), dim3(kBlock),
                       0, stream, a, p0, B, sched, idx, rptr.as<int64_t>(), ridx.as<int32_t>(),
                       rval.as<T>(), Pt.as<double>(), w.as<double>(), lams.as<double>(), n_orders,
                       k, d, degree);
    hipLaunchKernelGGL(inb_stats_kernel, dim3(ib_nstrips, Tt), dim3(kBlock), 0, stream, a, p0, B,
                       sched, idx);
    hipLaunchKernelGGL(inb_lse_kernel, dim3(cdiv(ib_Bpad, kBlock)), dim3(kBlock), 0, stream, a, p0,
                       B, sched, idx, ib_loss.as<double>());
    if (eval) return;
    hipLaunchKernelGGL((inb_grad_tile_kernel<false>), dim3(ib_nstrips, Tt, nrc), dim3(kBlock), 0,
                       stream, a, p0, B, sched, idx);
    hipLaunchKernelGGL((inb_grad_tile_kernel<true>), dim3(ib_nstrips, Tt, nrc), dim3(kBlock), 0,
                       stream, a, p0, B, sched, idx);
    hipLaunchKernelGGL((inb_back_kernel<T, L>), dim3(cdiv(ib_Bpad, kBlock / L), 2), dim3(kBlock), 0,
                       stream, a, p0, B, sched, idx, rptr.as<int64_t>(), ridx.as<int32_t>(),
                       rval.as<T>(), Pt.as<double>(), lams.as<double>(), n_orders, k, d, degree,
                       fit_linear, sg_gradP.as<double>(), sg_gradw.as<double>());
}

void spfm_engine::inbatch_launch(int64_t pos, int B, bool table, int degree, int fit_linear,
                                 bool eval) {
    SPFM_DISPATCH(dtype, SPFM_DISPATCH_L(k, inbatch_launch_tl<T, L>(pos, B, table, degree,
                                                                     fit_linear, eval)));
}

int spfm_engine::psgd_inbatch_epoch(const PsgdStep& st, const int32_t* pairs, int64_t m,
                                    double* sum_loss) {
    SPFM_TRY(psgd_inbatch_check("psgd inbatch", st.degree, st.batch_size < 1 ? 1 : st.batch_size,
                                pairs, m));
    if (const std::string e = st.check("psgd inbatch"); !e.empty()) FAIL(SPFM_ERR_INVALID, e);
    SPFM_TRY(inbatch_prepare(st.degree, st.batch_size, pairs, m));
    SPFM_TRY(psgd_inbatch_run(st, m));
    return psgd_epoch_end(ib_loss.as<double>(), m, sum_loss);
}

// the towers, the statistics and the losses of every minibatch at the live parameters
int spfm_engine::psgd_inbatch_eval(int degree, int64_t batch_size, const int32_t* pairs, int64_t m,
                                   double* sum_loss) {
    SPFM_TRY(psgd_inbatch_check("psgd inbatch eval", degree, batch_size, pairs, m));
    if (sum_loss) *sum_loss = 0.0;
    SPFM_TRY(inbatch_prepare(degree, batch_size, pairs, m));
    for (int64_t pos = 0; pos < m; pos += batch_size)
        inbatch_launch(pos, (int)std::min<int64_t>(batch_size, m - pos), false, degree, 0, true);
    loss_sum(ib_loss.as<double>(), m, 0);
    HIPC(hipGetLastError());
    SPFM_TRY(download(h_scalar, scalar.p, 1));
    HIPC(hipStreamSynchronize(stream));
    if (sum_loss) *sum_loss = h_scalar[0];
    return SPFM_OK;
}

extern "C" {

int spfm_psgd_inbatch_epoch(spfm_handle h, int degree, double alpha, double beta, double gamma,
                            double eta0, int learning_rate, double power_t, int64_t batch_size,
                            const int32_t* pairs, int64_t m, int fit_linear, int64_t* it,
                            double* sum_loss) {
    SPFM_GUARD(h);
    const PsgdStep st = h->psgd_step(degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                                      batch_size, fit_linear, it);
    return h->psgd_inbatch_epoch(st, pairs, m, sum_loss);
}

int spfm_psgd_inbatch_eval(spfm_handle h, int degree, int64_t batch_size, const int32_t* pairs,
                           int64_t m, double* sum_loss) {
    SPFM_GUARD(h);
    return h->psgd_inbatch_eval(degree, batch_size, pairs, m, sum_loss);
}

}  // extern "C"
