// spfm_engine_psgd_pairs_det.hip -- deterministic gradient of the pairwise fit:
// the plan over the resident triple list and the launches of its two kernels.  The minibatch
// driver, the update and the Michelot passes stay in spfm_engine_psgd.hip, which calls
// pairs_det_launch through psgd_batches_tl's gradient callable.
#include "spfm_engine.hip.h"
#include "spfm_psgd_pairs_det.hip.h"
#include "spfm_psgd_plan.hip.h"

using namespace spfm;

int spfm_engine::psgd_pairs_set_deterministic(int mode) {
    if (mode != 0 && mode != 1)
        FAIL(SPFM_ERR_INVALID, "pairs_set_deterministic: mode must be 0 (off) or 1 (on)");
    pairs_det = mode;
    return SPFM_OK;
}

// The plan of the epoch over sg_triples[0, m): the stored entries of every triple's three rows,
// enumerated by position and role, stably sorted by (minibatch, column), and the tables of the
// runs.  Nothing is uploaded.  Kept while the list and batch_size stay what they were (the list is
// compared on the device with the planned copy), so a fit that samples once plans once.
template <typename T>
int spfm_engine::pairs_det_plan_t(int64_t m, int64_t batch_size) {
    if (std::min(m, batch_size) > ((int64_t)1 << 30))
        FAIL(SPFM_ERR_UNSUPPORTED, "psgd pairs (deterministic): more than 2^30 triples in a "
                                   "minibatch");
    const int64_t nbat = cdiv(m, batch_size);
    int* h_figs = reinterpret_cast<int*>(h_scalar + 4);
    HIPC(pd_figs.alloc(sizeof(int) * 4));
    int* figs = pd_figs.as<int>();  // runs, longest run, lists differ
    if (pd_bs == batch_size && pd_m == m && pd_trip.p) {
        HIPC(hipMemsetAsync(figs + 2, 0, sizeof(int), stream));
        hipLaunchKernelGGL(det_differ_kernel, dim3(cdiv(3 * m, kBlock)), dim3(kBlock), 0, stream,
                           sg_triples.as<int32_t>(), pd_trip.as<int32_t>(), 3 * m, figs + 2);
        SPFM_TRY(download(h_figs, figs + 2, 1));
        HIPC(hipStreamSynchronize(stream));
        if (!h_figs[0]) return SPFM_OK;
    }
    pd_bs = 0;
    // the number of records: the three rows' entries summed over the list
    HIPC(pd_len.alloc(sizeof(int64_t) * (size_t)(m + 1)));
    HIPC(pd_qoff.alloc(sizeof(int64_t) * (size_t)(m + 1)));
    size_t t1 = 0;
    HIPC(rocprim::exclusive_scan(nullptr, t1, pd_len.as<int64_t>(), pd_qoff.as<int64_t>(),
                                 (int64_t)0, (size_t)(m + 1), rocprim::plus<int64_t>(), stream));
    HIPC(pd_tmp.alloc(t1));
    HIPC(hipMemsetAsync(pd_len.as<int64_t>() + m, 0, sizeof(int64_t), stream));
    hipLaunchKernelGGL(pair_det_len_kernel, dim3(cdiv(m, kBlock)), dim3(kBlock), 0, stream,
                       sg_triples.as<int32_t>(), rptr.as<int64_t>(), m, pd_len.as<int64_t>());
    t1 = pd_tmp.bytes;
    HIPC(rocprim::exclusive_scan(pd_tmp.p, t1, pd_len.as<int64_t>(), pd_qoff.as<int64_t>(),
                                 (int64_t)0, (size_t)(m + 1), rocprim::plus<int64_t>(), stream));
    int64_t N = 0;  // qoff[m]: the scan ran over m + 1 items
    SPFM_TRY(download(&N, pd_qoff.as<int64_t>() + m, 1));
    HIPC(hipStreamSynchronize(stream));
    if (N > INT32_MAX)
        FAIL(SPFM_ERR_UNSUPPORTED, "psgd pairs (deterministic): more than 2^31 - 1 plan records");
    HIPC(pd_trip.alloc(sizeof(int32_t) * 3 * (size_t)m));
    auto lengths = []() -> int { return SPFM_OK; };  // (counted above)
    auto enumerate = [&](uint64_t* key, uint32_t* val, int32_t* entq) {
        hipLaunchKernelGGL(pair_det_enum_kernel, dim3(cdiv(m, kBlock / 16)), dim3(kBlock), 0,
                           stream, sg_triples.as<int32_t>(), rptr.as<int64_t>(),
                           ridx.as<int32_t>(), pd_qoff.as<int64_t>(), m, batch_size, d, key, val,
                           entq);
    };
    auto head = [&](const uint64_t* key, const uint32_t* val, const int32_t* entq, int32_t* flag) {
        hipLaunchKernelGGL((pair_det_head_kernel<T>), dim3(cdiv(N, kBlock)), dim3(kBlock), 0,
                           stream, key, val, entq, sg_triples.as<int32_t>(), rptr.as<int64_t>(),
                           rval.as<T>(), pd_qoff.as<int64_t>(), N, batch_size,
                           pd_rec.as<uint32_t>(), pd_recx.as<T>(), flag);
    };
    SPFM_TRY(det_plan_runs({pd_keys, pd_vals, pd_entq, pd_rec, pd_recx, pd_segptr, pd_segcol,
                            pd_bseg, pd_tmp, pd_figs},
                           sizeof(uint32_t), sizeof(T), N, nbat, t1, lengths, enumerate, head,
                           pd_nseg, pd_longest));
    HIPC(hipMemcpyAsync(pd_trip.p, sg_triples.p, sizeof(int32_t) * 3 * (size_t)m,
                        hipMemcpyDeviceToDevice, stream));
    pd_bs = batch_size;
    pd_m = m;
    return SPFM_OK;
}

// the plan, then the per-minibatch dL / DP state of the two gradient kernels (a moved buffer
// changes the recorded kernel arguments) and the bytes the mode holds
int spfm_engine::pairs_det_prepare(const PsgdStep& st, int64_t m) {
    SPFM_TRY(SPFM_DISPATCH(dtype, return pairs_det_plan_t<T>(m, st.batch_size)));
    SPFM_TRY(det_grid_init());
    const int64_t bmax = std::min<int64_t>(st.batch_size, m);
    const void *o1 = pd_dl.p, *o2 = pd_state.p;
    HIPC(pd_dl.alloc(sizeof(double) * (size_t)bmax));
    HIPC(pd_state.alloc(sizeof(double) * (size_t)bmax * 2 * n_orders * (st.degree - 1) * k));
    if (pd_dl.p != o1 || pd_state.p != o2) clear_graphs();
    pd_bytes = 0;
    for (const DevBuf* b : {&pd_trip, &pd_len, &pd_qoff, &pd_keys, &pd_vals, &pd_entq, &pd_rec,
                            &pd_recx, &pd_segptr, &pd_segcol, &pd_bseg, &pd_tmp, &pd_figs, &pd_dl,
                            &pd_state})
        pd_bytes += (int64_t)b->bytes;
    return SPFM_OK;
}

template <typename T, int L, bool WT>
void spfm_engine::pairs_det_launch_tl(int64_t pos, int B, bool table, const PsgdStep& st) {
    const PsgdBatch* sched = table ? sg_sched.as<PsgdBatch>() : (const PsgdBatch*)nullptr;
    int* idx = table ? sg_idx.as<int>() : (int*)nullptr;
    const PairDetPlan pl{pd_bseg.as<int32_t>(), pd_segptr.as<int32_t>(), pd_segcol.as<int32_t>(),
                         pd_rec.as<uint32_t>()};
    hipLaunchKernelGGL((psgd_pair_rowstate_kernel<T, L, WT>), dim3(dt_grid), dim3(kBlock), 0,
                       stream, sg_triples.as<int32_t>() + 3 * pos, B, rptr.as<int64_t>(),
                       ridx.as<int32_t>(), rval.as<T>(), Pt.as<double>(), w.as<double>(),
                       lams.as<double>(), n_orders, k, d, st.degree, loss, pd_dl.as<double>(),
                       pd_state.as<double>(), sg_lossrow.as<double>() + pos, sched, idx,
                       WT ? sg_weights.as<double>() + pos : (const double*)nullptr);
    hipLaunchKernelGGL((psgd_pair_colgrad_kernel<T, L>), dim3(dt_grid), dim3(kBlock), 0, stream,
                       pl, pd_recx.as<T>(), (int)(pos / st.batch_size), Pt.as<double>(),
                       lams.as<double>(), pd_dl.as<double>(), pd_state.as<double>(), n_orders, k,
                       d, st.degree, st.fit_linear, sg_gradP.as<double>(), sg_gradw.as<double>(),
                       (const int*)idx);
}

// the gradient of the triples [pos, pos + B) (table: of the batch sg_idx[0] of sg_sched)
void spfm_engine::pairs_det_launch(int64_t pos, int B, bool table, const PsgdStep& st,
                                   bool weighted) {
    if (weighted)
        SPFM_DISPATCH(dtype,
                      SPFM_DISPATCH_L(k, pairs_det_launch_tl<T, L, true>(pos, B, table, st)));
    else
        SPFM_DISPATCH(dtype,
                      SPFM_DISPATCH_L(k, pairs_det_launch_tl<T, L, false>(pos, B, table, st)));
}

extern "C" {

int spfm_psgd_pairs_set_deterministic(spfm_handle h, int mode) {
    SPFM_GUARD(h);
    return h->psgd_pairs_set_deterministic(mode);
}

int spfm_psgd_pairs_get_deterministic(spfm_handle h, int* mode, int64_t* segments,
                                      int64_t* longest_segment, int64_t* plan_bytes) {
    SPFM_GUARD(h);
    const bool planned = h->pd_bs > 0;
    if (mode) *mode = h->pairs_det;
    if (segments) *segments = planned ? h->pd_nseg : 0;
    if (longest_segment) *longest_segment = planned ? h->pd_longest : 0;
    if (plan_bytes) *plan_bytes = planned ? h->pd_bytes : 0;
    return SPFM_OK;
}

}  // extern "C"
