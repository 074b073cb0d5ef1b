// spfm_engine_psgd.hip -- minibatch solver (psgd)
#include "spfm_engine.hip.h"
#include "spfm_psgd_pairs.hip.h"
#include "spfm_psgd_sample.hip.h"
#include "spfm_psgd_lists.hip.h"

using namespace spfm;

// ================================================================== psgd
// regularizer.init_cache_psgd exists for l1 / l21 / squaredl12 / squaredl21 only
// (reference regularizer/*.py); psgd has no all-subsets variant.
int spfm_engine::configure_psgd(int loss_, int reg_, int top_degree_) {
    if (reg_ != SPFM_REG_L1 && reg_ != SPFM_REG_L21 && reg_ != SPFM_REG_SQUAREDL12 &&
        reg_ != SPFM_REG_SQUAREDL21)
        FAIL(SPFM_ERR_INVALID, "this regularizer cannot be used with solver='psgd'");
    if (top_degree_ < 2 || top_degree_ > SPFM_MAX_DEGREE)
        FAIL(SPFM_ERR_UNSUPPORTED, "psgd: degree must be in 2..6");
    if (top_degree_ - (n_orders - 1) < 1)
        FAIL(SPFM_ERR_INVALID, "psgd: more parameter orders than degrees");
    if (k > 64 * kPsgdMaxC) FAIL(SPFM_ERR_UNSUPPORTED, "psgd: n_components > 256 not supported");
    solver = SPFM_SOLVER_PSGD;
    loss = loss_;
    reg = reg_;
    top_degree = top_degree_;
    clear_graphs();
    const size_t np = (size_t)n_orders * k * d;
    const size_t V = (size_t)n_orders * k;
    HIPC(sg_gradP.alloc(sizeof(double) * np));
    HIPC(sg_gradw.alloc(sizeof(double) * (size_t)d));
    HIPC(sg_samples.alloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1)));
    HIPC(sg_part.alloc(sizeof(double) * 2 * V * kPsgdNB));
    HIPC(sg_cond.alloc(sizeof(double) * V));
    HIPC(sg_thr.alloc(sizeof(double) * V));
    HIPC(sg_theta.alloc(sizeof(double) * V));
    HIPC(sg_done.alloc(sizeof(int) * 4));
    HIPC(sg_conv.alloc(sizeof(int) * V));
    HIPC(sg_norms.alloc(sizeof(double) * (size_t)n_orders * d));
    HIPC(hipMemsetAsync(sg_cond.p, 0, sizeof(double) * V, stream));  // first prox: G = all
    psgd_warm = false;
    HIPC(hipMemsetAsync(sg_gradP.p, 0, sizeof(double) * np, stream));
    HIPC(hipMemsetAsync(sg_gradw.p, 0, sizeof(double) * (size_t)d, stream));
    HIPC(hipMemsetAsync(sg_done.p, 0, sizeof(int) * 4, stream));
    HIPC(scalar.alloc(sizeof(double) * 8));
    if (!h_scalar) HIPC(hipHostMalloc((void**)&h_scalar, sizeof(double) * 8));
    HIPC(hipStreamSynchronize(stream));
    configured = true;
    return SPFM_OK;
}

// the state every entry of the unit but the pointwise epoch asks for, in `what`'s words
int spfm_engine::psgd_ready(const char* what, int degree) {
    const std::string w = std::string(what) + ": ";
    if (!have_data || !have_params || !configured)
        FAIL(SPFM_ERR_INVALID, w + "data, parameters and configuration are required");
    if (solver != SPFM_SOLVER_PSGD) FAIL(SPFM_ERR_INVALID, w + "engine is not configured for psgd");
    if (degree != top_degree) FAIL(SPFM_ERR_INVALID, w + "degree differs from configure()");
    return refuse_weighted(what);  // the triple and list kernels know no row weights
}

// ================================================== per-feature AdaGrad steps
// the step of an epoch entry with the handle's adaptive state beside the entry's arguments
PsgdStep spfm_engine::psgd_step(int degree, double alpha, double beta, double gamma, double eta0,
                                int lr, double power_t, int64_t batch_size, int fit_linear,
                                int64_t* it) const {
    PsgdStep st{degree, alpha, beta, gamma, eta0, lr, power_t, batch_size, fit_linear, it};
    st.adaptive = psgd_adaptive;
    st.g0 = psgd_g0;
    if (psgd_adaptive)
        st.adaptive_err = psgd_adaptive_error(
            reg == SPFM_REG_SQUAREDL12 || reg == SPFM_REG_SQUAREDL21, dist(),
            acc_orders == n_orders && acc_d == d);
    return st;
}

// NULL: the accumulator starts from zero.  A moved buffer changes the recorded kernel arguments.
int spfm_engine::psgd_set_adaptive(int mode, double g0, const double* acc_P, const double* acc_w) {
    if (mode != 0 && mode != 1)
        FAIL(SPFM_ERR_INVALID, "set_adaptive: mode must be 0 (off) or 1 (per-feature AdaGrad)");
    if (!(g0 > 0.0) || !std::isfinite(g0))
        FAIL(SPFM_ERR_INVALID, "set_adaptive: initial_accumulator must be positive and finite");
    if (!have_params) FAIL(SPFM_ERR_INVALID, "set_adaptive: set the parameters first");
    const size_t nP = (size_t)n_orders * d, nw = (size_t)d;
    for (size_t i = 0; acc_P && i < nP; ++i)
        if (!(acc_P[i] >= 0.0) || !std::isfinite(acc_P[i]))
            FAIL(SPFM_ERR_INVALID, "set_adaptive: acc_P holds a negative or non-finite value");
    for (size_t i = 0; acc_w && i < nw; ++i)
        if (!(acc_w[i] >= 0.0) || !std::isfinite(acc_w[i]))
            FAIL(SPFM_ERR_INVALID, "set_adaptive: acc_w holds a negative or non-finite value");
    const void *o1 = sg_accP.p, *o2 = sg_accw.p;
    HIPC(sg_accP.alloc(sizeof(double) * nP));
    HIPC(sg_accw.alloc(sizeof(double) * nw));
    if (sg_accP.p != o1 || sg_accw.p != o2) clear_graphs();
    if (acc_P)
        SPFM_TRY(upload_to(sg_accP.p, acc_P, nP));
    else
        HIPC(hipMemsetAsync(sg_accP.p, 0, sizeof(double) * nP, stream));
    if (acc_w)
        SPFM_TRY(upload_to(sg_accw.p, acc_w, nw));
    else
        HIPC(hipMemsetAsync(sg_accw.p, 0, sizeof(double) * nw, stream));
    HIPC(hipStreamSynchronize(stream));  // the caller may reuse its arrays
    acc_orders = n_orders;
    acc_d = d;
    psgd_adaptive = mode;
    psgd_g0 = g0;
    return SPFM_OK;
}

int spfm_engine::psgd_get_adaptive(double* acc_P, double* acc_w) {
    if (acc_d == 0) FAIL(SPFM_ERR_INVALID, "get_adaptive: spfm_psgd_set_adaptive was not called");
    if (acc_P) SPFM_TRY(download(acc_P, sg_accP.p, (size_t)acc_orders * acc_d));
    if (acc_w) SPFM_TRY(download(acc_w, sg_accw.p, (size_t)acc_d));
    HIPC(hipStreamSynchronize(stream));
    return SPFM_OK;
}

// first stage of a count: out[block] = number of set flags in the block's contiguous slice
static __global__ __launch_bounds__(kBlock) void pair_count_partial_kernel(
    const int* __restrict__ v, int64_t n, double* __restrict__ out) {
    __shared__ double red[16];
    const int64_t per = (n + gridDim.x - 1) / gridDim.x;
    const int64_t lo = per * blockIdx.x, hi = (lo + per < n) ? lo + per : n;
    double a = 0, b = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) a += (double)v[i];
    block_sum2(a, b, red);
    if (threadIdx.x == 0) out[blockIdx.x] = a;
}

// scalar[slot] = sum of src[0, n): 256 partials of the slot's own, then one block (S = int: a
// count of set flags)
template <typename S>
void spfm_engine::loss_sum(const S* src, int64_t n_items, int slot) {
    double* part = partial.as<double>() + 256 * slot;
    if constexpr (std::is_same<S, int>::value)
        hipLaunchKernelGGL(pair_count_partial_kernel, dim3(256), dim3(kBlock), 0, stream, src,
                           n_items, part);
    else
        hipLaunchKernelGGL(reduce_partial_kernel, dim3(256), dim3(kBlock), 0, stream, src, n_items,
                           part);
    hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(kBlock), 0, stream, part, 256,
                       scalar.as<double>() + slot);
}

// the end of an epoch on either route: the sum of the items' losses (over the ranks, if several)
int spfm_engine::psgd_epoch_end(const double* loss_row, int64_t n_items, double* sum_loss) {
    loss_sum(loss_row, n_items, 0);
    HIPC(hipGetLastError());
    if (dist()) SPFM_TRY(allreduce(scalar.as<double>(), 1));
    SPFM_TRY(download(h_scalar, scalar.p, 1));
    HIPC(hipStreamSynchronize(stream));
    prof_collect();
    if (sum_loss) *sum_loss = h_scalar[0];
    psgd_warm = true;
    return SPFM_OK;
}

// The minibatches of one epoch over `n_items` training items (samples of the pointwise fit,
// triples of the pairwise one) behind a gradient launch: update, Michelot passes, table-driven
// graph replay of runs of 32 with the eager redo from a snapshot.
//   grad(pos, B, grid, table)  enqueues the gradient kernel of the items [pos, pos + B) on
//                              `grid` workgroups; table: the kernel takes pos and B of batch
//                              sg_idx[0] from sg_sched instead
template <int L, typename GradFn>
int spfm_engine::psgd_batches_tl(GradFn&& grad, const char* tag, int64_t tsize_, int64_t n_items,
                                 const PsgdStep& st) {
    const bool mich = (reg == SPFM_REG_SQUAREDL12 || reg == SPFM_REG_SQUAREDL21);
    constexpr int gpb = kBlock / L;
    const int nb_dense = (int)std::min<int64_t>(kPsgdNB, cdiv(d, gpb));
    MichState ms;
    ms.part = sg_part.as<double>();
    ms.cond = sg_cond.as<double>();
    ms.thr = sg_thr.as<double>();
    ms.theta = sg_theta.as<double>();
    ms.conv = sg_conv.as<int>();
    ms.done = sg_done.as<int>();
    ms.V = (reg == SPFM_REG_SQUAREDL12) ? n_orders * k : n_orders;
    ms.NB = nb_dense;
    const int nb_fin = cdiv(ms.V, kBlock / kWave);
    int* h_done = reinterpret_cast<int*>(h_scalar + 4);
    // what follows a gradient, for both routes below: with a table (graph replay) the kernels
    // read the minibatch's scalars from sched[idx[1]] and the ones passed here are placeholders
    // (adaptive steps: the kernel of DESIGN.md section 19d takes the update's place on both routes)
    auto update = [&](const PsgdBatch& b, const PsgdBatch* sched, int* idx) {
        if (st.adaptive)
            hipLaunchKernelGGL((psgd_update_adaptive_kernel<L>), dim3(nb_dense), dim3(kBlock), 0,
                               stream, Pt.as<double>(), sg_gradP.as<double>(), w.as<double>(),
                               sg_gradw.as<double>(), sg_accP.as<double>(), sg_accw.as<double>(),
                               n_orders, k, d, reg, st.fit_linear, b, sched, idx);
        else
            hipLaunchKernelGGL((psgd_update_kernel<L>), dim3(nb_dense), dim3(kBlock), 0, stream,
                               Pt.as<double>(), sg_gradP.as<double>(), w.as<double>(),
                               sg_gradw.as<double>(), n_orders, k, d, reg, b.cp, b.denp,
                               b.strength, st.fit_linear, b.cw, b.denw, sg_norms.as<double>(), ms,
                               sched, idx);
    };
    auto mich_finish = [&](double strength, const PsgdBatch* sched, const int* idx) {
        hipLaunchKernelGGL(psgd_mich_finish_kernel, dim3(nb_fin), dim3(kBlock), 0, stream, ms,
                           strength, sched, idx);
    };
    auto mich_sweeps = [&](int count, double strength, const PsgdBatch* sched, const int* idx) {
        for (int sweep = 0; sweep < count; ++sweep) {
            hipLaunchKernelGGL((psgd_mich_reduce_kernel<L>), dim3(nb_dense), dim3(kBlock), 0,
                               stream, Pt.as<double>(), sg_norms.as<double>(), n_orders, k, d, reg,
                               ms);
            mich_finish(strength, sched, idx);
        }
    };
    auto mich_apply = [&]() {
        hipLaunchKernelGGL((psgd_mich_apply_kernel<L>), dim3(nb_dense), dim3(kBlock), 0, stream,
                           Pt.as<double>(), sg_norms.as<double>(), n_orders, k, d, reg,
                           sg_thr.as<double>());
    };
    // l1 / l21 (no host round trip inside a minibatch): tabulate the epoch and replay runs
    // of kPsgdRun minibatches from one hipGraph -- the kernels take the batch from a device
    // table, so every (gradient, update) pair has identical arguments
    // (squared-norm prox: the first epoch after configure() starts the support search cold --
    // 6-13 sweeps -- and runs eagerly; afterwards minibatches warm-start each other)
    // (several ranks: every minibatch carries a collective -- eager launches)
    if (use_graph && !prof_on && !psgd_force_eager && !dist() && (!mich || psgd_warm)) {
        constexpr int kPsgdRun = 32;
        const int kMichSweeps = psgd_graph_sweeps;  // recorded sweeps per minibatch (2 suffice
                                                    // with the warm start; a failed check
                                                    // redoes the epoch eagerly)
        tabulate_epoch(st, n_items, *st.it, h_sched);
        const int64_t nbat = (int64_t)h_sched.size();
        const void* old = sg_sched.p;
        HIPC(sg_sched.alloc(sizeof(PsgdBatch) * (size_t)nbat));
        HIPC(sg_idx.alloc(sizeof(int) * 4));
        if (sg_sched.p != old) clear_graphs();
        SPFM_TRY(upload_to(sg_sched.p, h_sched.data(), (size_t)nbat));
        HIPC(hipMemsetAsync(sg_idx.p, 0, sizeof(int) * 4, stream));  // idx[0..1], idx[2] = failed
        const size_t np = (size_t)n_orders * k * d;
        if (mich) {  // snapshot for the (rare) eager redo
            HIPC(sg_snapP.alloc(sizeof(double) * np));
            HIPC(sg_snapw.alloc(sizeof(double) * (size_t)d));
            HIPC(sg_snapc.alloc(sizeof(double) * (size_t)ms.V));
            HIPC(hipMemcpyAsync(sg_snapP.p, Pt.p, sizeof(double) * np, hipMemcpyDeviceToDevice,
                                stream));
            HIPC(hipMemcpyAsync(sg_snapw.p, w.p, sizeof(double) * (size_t)d,
                                hipMemcpyDeviceToDevice, stream));
            HIPC(hipMemcpyAsync(sg_snapc.p, sg_cond.p, sizeof(double) * (size_t)ms.V,
                                hipMemcpyDeviceToDevice, stream));
        }
        const int gridg = cdiv(std::min<int64_t>(st.batch_size, n_items), gpb);
        const PsgdBatch* sched = sg_sched.as<PsgdBatch>();
        int* idx = sg_idx.as<int>();
        PsgdBatch none{};  // placeholders: the kernels read sched[idx[1]]
        none.B = 1;
        none.denp = none.denw = 1.0;
        auto pair = [&]() {
            grad((int64_t)0, 0, gridg, true);
            update(none, sched, idx);
            if (!mich) return;
            mich_finish(0.0, sched, idx);
            mich_sweeps(kMichSweeps, 0.0, sched, idx);
            hipLaunchKernelGGL(psgd_mich_verify_kernel, dim3(1), dim3(kBlock), 0, stream, ms,
                               idx + 2);
            mich_apply();
        };
        const std::string key = fkey(tag, {}, {st.degree, loss, reg, st.fit_linear, gridg, L,
                                                  tsize_, (int64_t)mich,
                                                  (int64_t)psgd_graph_sweeps,
                                                  (int64_t)st.adaptive});
        int64_t done_b = 0;
        for (; done_b + kPsgdRun <= nbat; done_b += kPsgdRun) {
            int rc = run_cached(key, [&]() {
                for (int q = 0; q < kPsgdRun; ++q) pair();
                return (int)SPFM_OK;
            });
            if (rc) return rc;
        }
        for (; done_b < nbat; ++done_b) pair();
        HIPC(hipGetLastError());
        int failed = 0;
        if (mich)
            SPFM_TRY(download(&failed, sg_idx.as<int>() + 2, 1));
        HIPC(hipStreamSynchronize(stream));  // h_sched may be rewritten by the next epoch
        if (!failed) {
            *st.it += nbat;
            return SPFM_OK;
        }
        // some minibatch needed more sweeps than were recorded: restore and redo eagerly
        HIPC(hipMemcpyAsync(Pt.p, sg_snapP.p, sizeof(double) * np, hipMemcpyDeviceToDevice,
                            stream));
        HIPC(hipMemcpyAsync(w.p, sg_snapw.p, sizeof(double) * (size_t)d,
                            hipMemcpyDeviceToDevice, stream));
        HIPC(hipMemcpyAsync(sg_cond.p, sg_snapc.p, sizeof(double) * (size_t)ms.V,
                            hipMemcpyDeviceToDevice, stream));
        HIPC(hipMemsetAsync(sg_gradP.p, 0, sizeof(double) * np, stream));
        HIPC(hipMemsetAsync(sg_gradw.p, 0, sizeof(double) * (size_t)d, stream));
        psgd_redone += 1;
    }
    // one rank: the batches of its n samples; several ranks: the batches of the global order,
    // of which this rank holds samples [lpos, lpos + lB) of its local list (psgd_epoch)
    const bool sharded = dist();
    const int64_t nbat_e = sharded ? (int64_t)sg_gB.size() : cdiv(n_items, st.batch_size);
    for (int64_t bi = 0; bi < nbat_e; ++bi) {
        const int64_t pos = sharded ? sg_lpos[(size_t)bi] : bi * st.batch_size;
        const int lB =
            sharded ? sg_lB[(size_t)bi] : (int)std::min<int64_t>(st.batch_size, n_items - pos);
        const int B = sharded ? sg_gB[(size_t)bi] : lB;  // eta / B: the whole minibatch
        prof_begin(0, 0);
        if (lB > 0) grad(pos, lB, (int)cdiv(lB, gpb), false);
        prof_end(0);
        if (sharded) {  // sum of the ranks' gradients: identical bits on every rank
            int arc = allreduce(sg_gradP.as<double>(), (size_t)n_orders * k * d);
            if (arc) return arc;
            if (st.fit_linear) {
                arc = allreduce(sg_gradw.as<double>(), (size_t)d);
                if (arc) return arc;
            }
        }
        const PsgdBatch b = st.batch(*st.it, B);
        prof_begin(1, 0);
        update(b, nullptr, nullptr);
        prof_end(1);
        if (mich) {
            prof_begin(2, 0);
            mich_finish(b.strength, nullptr, nullptr);
            // the iteration is monotone after the first sweep, so it terminates (<= d
            // sweeps; 2-4 with the warm start); the host looks at the flag per chunk
            for (int guard = 0;; ++guard) {
                mich_sweeps(2, b.strength, nullptr, nullptr);
                hipLaunchKernelGGL(psgd_mich_check_kernel, dim3(1), dim3(kBlock), 0, stream,
                                   ms);
                SPFM_TRY(download(h_done, sg_done.p, 1));
                HIPC(hipStreamSynchronize(stream));
                if (*h_done) break;
                if (guard > d) FAIL(SPFM_ERR_RUNTIME, "psgd: prox support search did not settle");
            }
            mich_apply();
            prof_end(2);
        }
        *st.it += 1;
    }
    HIPC(hipGetLastError());
    return SPFM_OK;
}

// the pointwise gradient (one sample per group) in front of the shared minibatch driver
template <typename T, int L>
int spfm_engine::psgd_epoch_tl(const PsgdStep& st) {
    auto grad = [&](int64_t pos, int B, int grid, bool table) {
        if (weighted) {
            hipLaunchKernelGGL((psgd_grad_kernel<T, L, RowWeight>), dim3(grid), dim3(kBlock), 0,
                               stream, sg_samples.as<int32_t>() + pos, B, rptr.as<int64_t>(),
                               ridx.as<int32_t>(), rval.as<T>(), yy.as<T>(), Pt.as<double>(),
                               w.as<double>(), lams.as<double>(), n_orders, k, d, st.degree,
                               loss, st.fit_linear, sg_gradP.as<double>(),
                               sg_gradw.as<double>(), pred_tmp.as<double>() + pos,
                               table ? sg_sched.as<PsgdBatch>() : (const PsgdBatch*)nullptr,
                               table ? sg_idx.as<int>() : (int*)nullptr,
                               RowWeight{wrow.as<double>()});
            return;
        }
        hipLaunchKernelGGL((psgd_grad_kernel<T, L>), dim3(grid), dim3(kBlock), 0, stream,
                           sg_samples.as<int32_t>() + pos, B, rptr.as<int64_t>(),
                           ridx.as<int32_t>(), rval.as<T>(), yy.as<T>(), Pt.as<double>(),
                           w.as<double>(), lams.as<double>(), n_orders, k, d, st.degree, loss,
                           st.fit_linear, sg_gradP.as<double>(), sg_gradw.as<double>(),
                           pred_tmp.as<double>() + pos,
                           table ? sg_sched.as<PsgdBatch>() : (const PsgdBatch*)nullptr,
                           table ? sg_idx.as<int>() : (int*)nullptr, NoRowWeight{});
    };
    // (the graph tag says which gradient kernel was recorded)
    return psgd_batches_tl<L>(grad, weighted ? "psgd_w" : "psgd", (int64_t)sizeof(T), n, st);
}

// optimizer/psgd.py:125-199: one pass over indices_samples
int spfm_engine::psgd_epoch(const PsgdStep& st, const int32_t* indices_samples, int64_t n_samples,
                            int64_t row_lo, double* sum_loss) {
    // (this entry's three state messages share no prefix: psgd_ready cannot word them)
    if (!have_data || !have_params || !configured)
        FAIL(SPFM_ERR_INVALID, "epoch: data, parameters and configuration are required");
    if (solver != SPFM_SOLVER_PSGD) FAIL(SPFM_ERR_INVALID, "engine is not configured for psgd");
    if (st.degree != top_degree) FAIL(SPFM_ERR_INVALID, "psgd: degree differs from configure()");
    const bool sharded = dist();
    if (!indices_samples || !st.it || (!sharded && (n_samples != n || row_lo != 0)))
        FAIL(SPFM_ERR_INVALID, "psgd: indices_samples must list every sample once");
    if (sharded && (row_lo < 0 || row_lo + n > n_samples || n_samples > INT32_MAX))
        FAIL(SPFM_ERR_INVALID, "psgd: the handle's rows [row_lo, row_lo + n) lie outside the "
                               "global sample range");
    if (const std::string e = st.check("psgd"); !e.empty()) FAIL(SPFM_ERR_INVALID, e);
    if (!is_permutation(indices_samples, n_samples))
        FAIL(SPFM_ERR_INVALID, "psgd: indices_samples is not a permutation");
    if (n_samples == 0) {
        if (sum_loss) *sum_loss = 0.0;
        return SPFM_OK;
    }
    SPFM_TRY(ensure_pt());
    p_valid = false;
    std::vector<int32_t> local;  // several ranks: this rank's samples in visiting order
    if (sharded) {
        if (!shard_batches(indices_samples, n_samples, row_lo, n, st.batch_size, sg_lpos, sg_lB,
                           sg_gB, local))
            FAIL(SPFM_ERR_INVALID, "psgd: the global order does not hold this rank's rows once");
        indices_samples = local.data();
    }
    if (n > 0) {
        SPFM_TRY(upload_to(sg_samples.p, indices_samples, (size_t)n));
        HIPC(hipStreamSynchronize(stream));  // caller may reuse indices_samples
    }
    SPFM_TRY(SPFM_DISPATCH(dtype, return SPFM_DISPATCH_L(k, return psgd_epoch_tl<T, L>(st))));
    return psgd_epoch_end(pred_tmp.as<double>(), n, sum_loss);
}

// ============================================================ pairwise ranking fit
//  triples (anchor, plus, minus) of rows of the handle's data [X; Z]

// Argument checks of both pair entries, on the host, before any launch: the state of the handle,
// the row indices, plus != minus, and -- one flag per row the triples name, then one pass over
// the columns' stored rows -- no column stored in an anchor row and in a plus / minus row.
int spfm_engine::psgd_pairs_check(const char* what, int degree, const int32_t* triples, int64_t m) {
    SPFM_TRY(psgd_ready(what, degree));
    if (m < 0 || (m > 0 && !triples) || m > INT32_MAX)
        FAIL(SPFM_ERR_INVALID, std::string(what) + ": triples must hold 0 <= m < 2^31 rows of 3");
    std::vector<uint8_t> side((size_t)(n > 0 ? n : 1), 0);  // 1: anchor, 2: plus / minus
    for (int64_t q = 0; q < m; ++q) {
        const int32_t b = triples[3 * q], cp = triples[3 * q + 1], cm = triples[3 * q + 2];
        if (b < 0 || b >= n || cp < 0 || cp >= n || cm < 0 || cm >= n)
            FAIL(SPFM_ERR_INVALID, std::string(what) + ": triple " + std::to_string(q) +
                                       " names a row outside [0, n)");
        if (cp == cm)
            FAIL(SPFM_ERR_INVALID, std::string(what) + ": triple " + std::to_string(q) +
                                       " has plus == minus");
        side[(size_t)b] |= 1;
        side[(size_t)cp] |= 2;
        side[(size_t)cm] |= 2;
    }
    const int32_t j = first_shared_column(side, d, h_cptr.data(), h_cidx.data());
    if (j >= 0)
        FAIL(SPFM_ERR_INVALID, std::string(what) + ": column " + std::to_string(j) +
                                   " is stored in an anchor row and in a plus/minus row: the "
                                   "two column sets must be disjoint");
    return SPFM_OK;
}

// room for m triples and their losses (a new allocation changes the recorded kernel arguments);
// whatever list was drawn on the device is about to be overwritten
int spfm_engine::pairs_reserve(int64_t m) {
    sampled = false;
    sampled_weighted = false;
    const void *o1 = sg_triples.p, *o2 = sg_lossrow.p;
    HIPC(sg_triples.alloc(sizeof(int32_t) * 3 * (size_t)m));
    HIPC(sg_lossrow.alloc(sizeof(double) * (size_t)m));
    if (sg_triples.p != o1 || sg_lossrow.p != o2) clear_graphs();
    return SPFM_OK;
}

// room for m weights beside the triples
int spfm_engine::weights_reserve(int64_t m) {
    const void* old = sg_weights.p;
    HIPC(sg_weights.alloc(sizeof(double) * (size_t)m));
    if (sg_weights.p != old) clear_graphs();
    return SPFM_OK;
}

// WT: the weighted instance, reading sg_weights (the graph tag says which was recorded)
template <typename T, int L, bool WT>
int spfm_engine::psgd_pairs_epoch_tl(const PsgdStep& st, int64_t m) {
    auto grad = [&](int64_t pos, int B, int grid, bool table) {
        hipLaunchKernelGGL((psgd_pair_grad_kernel<T, L, false, WT>), dim3(grid), dim3(kBlock), 0,
                           stream, sg_triples.as<int32_t>() + 3 * pos, B, rptr.as<int64_t>(),
                           ridx.as<int32_t>(), rval.as<T>(), Pt.as<double>(), w.as<double>(),
                           lams.as<double>(), n_orders, k, d, st.degree, loss, st.fit_linear,
                           sg_gradP.as<double>(), sg_gradw.as<double>(),
                           sg_lossrow.as<double>() + pos, (int*)nullptr,
                           table ? sg_sched.as<PsgdBatch>() : (const PsgdBatch*)nullptr,
                           table ? sg_idx.as<int>() : (int*)nullptr,
                           WT ? sg_weights.as<double>() + pos : (const double*)nullptr);
    };
    return psgd_batches_tl<L>(grad, WT ? "psgd_pairs_w" : "psgd_pairs", (int64_t)sizeof(T), m, st);
}

int spfm_engine::psgd_pairs_epoch(const PsgdStep& st, const int32_t* triples, int64_t m,
                                  double* sum_loss) {
    if (dist()) FAIL(SPFM_ERR_UNSUPPORTED, "psgd pairs: several ranks are not supported");
    SPFM_TRY(psgd_pairs_check("psgd pairs", st.degree, triples, m));
    if (const std::string e = st.check("psgd pairs"); !e.empty()) FAIL(SPFM_ERR_INVALID, e);
    if (m == 0) {
        if (sum_loss) *sum_loss = 0.0;
        return SPFM_OK;
    }
    SPFM_TRY(ensure_pt());
    SPFM_TRY(pairs_reserve(m));
    SPFM_TRY(upload_to(sg_triples.p, triples, 3 * (size_t)m));
    HIPC(hipStreamSynchronize(stream));  // caller may reuse triples
    return psgd_pairs_run(st, m, sum_loss);
}

// uploaded triples with a weight each: sum_loss is the sum of wt * loss
int spfm_engine::psgd_pairs_epoch_weighted(const PsgdStep& st, const int32_t* triples,
                                           const double* weights, int64_t m, double* sum_loss) {
    if (dist()) FAIL(SPFM_ERR_UNSUPPORTED, "psgd pairs: several ranks are not supported");
    SPFM_TRY(psgd_pairs_check("psgd pairs", st.degree, triples, m));
    if (const std::string e = st.check("psgd pairs"); !e.empty()) FAIL(SPFM_ERR_INVALID, e);
    if (m > 0 && !weights) FAIL(SPFM_ERR_INVALID, "psgd pairs: weights must hold m values");
    for (int64_t q = 0; q < m; ++q)
        if (!(weights[q] >= 0.0) || !std::isfinite(weights[q]))
            FAIL(SPFM_ERR_INVALID, "psgd pairs: weight " + std::to_string(q) +
                                       " is negative or not finite");
    if (m == 0) {
        if (sum_loss) *sum_loss = 0.0;
        return SPFM_OK;
    }
    SPFM_TRY(ensure_pt());
    SPFM_TRY(pairs_reserve(m));
    SPFM_TRY(weights_reserve(m));
    SPFM_TRY(upload_to(sg_triples.p, triples, 3 * (size_t)m));
    SPFM_TRY(upload_to(sg_weights.p, weights, (size_t)m));
    HIPC(hipStreamSynchronize(stream));  // caller may reuse triples and weights
    return psgd_pairs_run(st, m, sum_loss, true);
}

// the batches over the resident triple list sg_triples[0, m) and the sum of the triples' losses
int spfm_engine::psgd_pairs_run(const PsgdStep& st, int64_t m, double* sum_loss, bool weighted) {
    p_valid = false;
    if (weighted)
        SPFM_TRY(SPFM_DISPATCH(dtype, return SPFM_DISPATCH_L(
                                          k, return psgd_pairs_epoch_tl<T, L, true>(st, m))));
    else
        SPFM_TRY(SPFM_DISPATCH(dtype, return SPFM_DISPATCH_L(
                                          k, return psgd_pairs_epoch_tl<T, L, false>(st, m))));
    return psgd_epoch_end(sg_lossrow.as<double>(), m, sum_loss);
}

// loss sum and number of triples with m > 0 at the live parameters; nothing is updated
int spfm_engine::psgd_pairs_eval(int degree, int fit_linear, const int32_t* triples, int64_t m,
                                 double* sum_loss, int64_t* n_ordered) {
    (void)fit_linear;  // the margin reads w as it stands (zeros when no linear term was fitted)
    if (dist()) FAIL(SPFM_ERR_UNSUPPORTED, "psgd pairs eval: several ranks are not supported");
    SPFM_TRY(psgd_pairs_check("psgd pairs eval", degree, triples, m));
    if (sum_loss) *sum_loss = 0.0;
    if (n_ordered) *n_ordered = 0;
    if (m == 0) return SPFM_OK;
    SPFM_TRY(ensure_pt());
    SPFM_TRY(pairs_reserve(m));
    HIPC(sg_ordered.alloc(sizeof(int) * (size_t)m));
    SPFM_TRY(upload_to(sg_triples.p, triples, 3 * (size_t)m));
    SPFM_DISPATCH(dtype, SPFM_DISPATCH_L(k, hipLaunchKernelGGL(
        (psgd_pair_grad_kernel<T, L, true>), dim3(cdiv(m, kBlock / L)), dim3(kBlock), 0, stream,
        sg_triples.as<int32_t>(), (int)m, rptr.as<int64_t>(), ridx.as<int32_t>(), rval.as<T>(),
        Pt.as<double>(), w.as<double>(), lams.as<double>(), n_orders, k, d, degree, loss, 0,
        (double*)nullptr, (double*)nullptr, sg_lossrow.as<double>(), sg_ordered.as<int>(),
        (const PsgdBatch*)nullptr, (int*)nullptr, (const double*)nullptr)));
    loss_sum(sg_lossrow.as<double>(), m, 0);
    loss_sum(sg_ordered.as<int>(), m, 1);
    HIPC(hipGetLastError());
    SPFM_TRY(download(h_scalar, scalar.p, 2));
    HIPC(hipStreamSynchronize(stream));
    if (sum_loss) *sum_loss = h_scalar[0];
    if (n_ordered) *n_ordered = (int64_t)h_scalar[1];
    return SPFM_OK;
}

// ============================================================ negatives drawn on the device
// 

int spfm_engine::psgd_pairs_set_sampler(int64_t n_ctx, int64_t n_cand, const int64_t* pos_ptr,
                                        const int32_t* pos_idx, const int64_t* forb_ptr,
                                        const int32_t* forb_idx) {
    have_sampler = false;
    sampled = false;
    have_proposal = have_posw = sampled_weighted = false;  // they go with the sampler
    if (!have_data) FAIL(SPFM_ERR_INVALID, "set_sampler: data is required");
    if (n_ctx < 1 || n_cand < 1 || n_ctx + n_cand != n)
        FAIL(SPFM_ERR_INVALID, "set_sampler: n_ctx + n_cand must be the handle's row count");
    if (const char* e = sampler_csr_error(n_ctx, n_cand, pos_ptr, pos_idx))
        FAIL(SPFM_ERR_INVALID, std::string("set_sampler: positives: ") + e);
    if (!forb_ptr) {
        forb_ptr = pos_ptr;
        forb_idx = pos_idx;
    } else if (const char* e = sampler_csr_error(n_ctx, n_cand, forb_ptr, forb_idx)) {
        FAIL(SPFM_ERR_INVALID, std::string("set_sampler: forbidden: ") + e);
    }
    const int64_t npos = pos_ptr[n_ctx];
    if (npos < 1 || npos > INT32_MAX)
        FAIL(SPFM_ERR_INVALID, "set_sampler: 1 <= nnz(positives) < 2^31 is required");
    int64_t bad = 0;
    if (const int kind = check_positives_in_forbidden(n_ctx, n_cand, pos_ptr, pos_idx, forb_ptr,
                                                      forb_idx, &bad))
        FAIL(SPFM_ERR_INVALID,
             "set_sampler: row " + std::to_string(bad) +
                 (kind == kForbiddenLacksPositive
                      ? " of the forbidden set lacks one of its positives"
                      : " forbids every candidate: no negative can be drawn"));
    std::vector<uint8_t> side((size_t)n, 0);  // 1: context with a positive, 2: candidate
    std::vector<int32_t> prow((size_t)npos);
    for (int64_t b = 0; b < n_ctx; ++b) {
        if (pos_ptr[b + 1] > pos_ptr[b]) side[(size_t)b] = 1;
        for (int64_t e = pos_ptr[b]; e < pos_ptr[b + 1]; ++e) prow[(size_t)e] = (int32_t)b;
    }
    for (int64_t c = n_ctx; c < n; ++c) side[(size_t)c] = 2;
    const int32_t j = first_shared_column(side, d, h_cptr.data(), h_cidx.data());
    if (j >= 0)  // the rule of psgd_pairs_check
        FAIL(SPFM_ERR_INVALID, "set_sampler: column " + std::to_string(j) +
                                   " is stored in a context row with a positive and in a "
                                   "candidate row: the two column sets must be disjoint");
    SPFM_TRY(upload(sm_posrow, prow.data(), (size_t)npos));
    SPFM_TRY(upload(sm_posidx, pos_idx, (size_t)npos));
    SPFM_TRY(upload(sm_fptr, forb_ptr, (size_t)n_ctx + 1));
    SPFM_TRY(upload(sm_fidx, forb_idx, (size_t)forb_ptr[n_ctx], 1));
    HIPC(hipStreamSynchronize(stream));  // prow dies here; the caller may reuse its arrays
    sm_nctx = n_ctx;
    sm_ncand = n_cand;
    sm_npos = npos;
    have_sampler = true;
    return SPFM_OK;
}

// The proposal distribution of every device sampler: inclusive cumulative sums of non-negative
// integer weights (non-decreasing, 1 <= cum[n_cand - 1] < 2^32); NULL: uniform again.
int spfm_engine::psgd_pairs_set_proposal(const uint32_t* cum, int64_t n_cand) {
    if (!have_sampler)
        FAIL(SPFM_ERR_INVALID, "set_proposal: call spfm_psgd_pairs_set_sampler first");
    if (!cum) {
        have_proposal = false;
        return SPFM_OK;
    }
    if (n_cand != sm_ncand)
        FAIL(SPFM_ERR_INVALID, "set_proposal: n_cand differs from the sampler's");
    for (int64_t c = 1; c < n_cand; ++c)
        if (cum[c] < cum[c - 1])
            FAIL(SPFM_ERR_INVALID, "set_proposal: cum decreases at candidate " + std::to_string(c));
    if (cum[n_cand - 1] < 1) FAIL(SPFM_ERR_INVALID, "set_proposal: every weight is zero");
    have_proposal = false;
    SPFM_TRY(upload(sm_cum, cum, (size_t)n_cand));
    HIPC(hipStreamSynchronize(stream));  // the caller may reuse cum
    sm_cumW = cum[n_cand - 1];
    have_proposal = true;
    return SPFM_OK;
}

// One weight per positive, canonical CSR order; NULL clears.  Once set, both sample entries write
// sg_weights.
int spfm_engine::psgd_pairs_set_positive_weights(const double* wq, int64_t nnz) {
    if (!have_sampler)
        FAIL(SPFM_ERR_INVALID, "set_positive_weights: call spfm_psgd_pairs_set_sampler first");
    if (!wq) {
        have_posw = false;
        return SPFM_OK;
    }
    if (nnz != sm_npos)
        FAIL(SPFM_ERR_INVALID, "set_positive_weights: nnz differs from the sampler's positives");
    for (int64_t q = 0; q < nnz; ++q)
        if (!(wq[q] >= 0.0) || !std::isfinite(wq[q]))
            FAIL(SPFM_ERR_INVALID, "set_positive_weights: weight " + std::to_string(q) +
                                       " is negative or not finite");
    have_posw = false;
    SPFM_TRY(upload(sm_posw, wq, (size_t)nnz));
    HIPC(hipStreamSynchronize(stream));  // the caller may reuse wq
    have_posw = true;
    return SPFM_OK;
}

int spfm_engine::psgd_pairs_sample_any(bool warp, int degree, int64_t n_negatives,
                                       int64_t n_candidates, int64_t max_draws, double margin,
                                       int64_t seed, int64_t epoch, const int32_t* order,
                                       int32_t* triples_out, double* scores_out,
                                       double* weights_out, int32_t* trials_out) {
    if (dist()) FAIL(SPFM_ERR_UNSUPPORTED, "psgd pairs sample: several ranks are not supported");
    SPFM_TRY(psgd_ready("psgd pairs sample", degree));
    if (!have_sampler)
        FAIL(SPFM_ERR_INVALID, "psgd pairs sample: call spfm_psgd_pairs_set_sampler first");
    if (n_negatives < 1 || n_candidates < 1 || max_draws < 1)
        FAIL(SPFM_ERR_INVALID, "psgd pairs sample: n_negatives, n_candidates and max_draws must "
                               "be >= 1");
    if (n_candidates > INT32_MAX || max_draws > INT32_MAX || n_negatives > INT32_MAX ||
        sm_npos * n_negatives > INT32_MAX)
        FAIL(SPFM_ERR_INVALID, "psgd pairs sample: the triple list is limited to 2^31 - 1 rows");
    if (seed < 0 || epoch < 0)
        FAIL(SPFM_ERR_INVALID, "psgd pairs sample: seed and epoch must be >= 0");
    if (warp && n_candidates > max_draws)
        FAIL(SPFM_ERR_INVALID, "psgd pairs sample: 1 <= max_trials <= max_draws is required");
    if (warp && !std::isfinite(margin))
        FAIL(SPFM_ERR_INVALID, "psgd pairs sample: margin must be finite");
    const int64_t m = sm_npos * n_negatives;
    if (order && !is_permutation(order, m))
        FAIL(SPFM_ERR_INVALID, "psgd pairs sample: order is not a permutation of 0..m-1");
    const bool wr = warp || have_posw;  // this call writes sg_weights
    SPFM_TRY(ensure_pt());
    SPFM_TRY(pairs_reserve(m));
    HIPC(sg_scores.alloc(sizeof(double) * (size_t)m));
    if (wr) SPFM_TRY(weights_reserve(m));
    if (warp) HIPC(sg_trials.alloc(sizeof(int32_t) * (size_t)m));
    if (order) SPFM_TRY(upload(sg_order, order, (size_t)m));
#define SPFM_SAMPLE_LAUNCH(WARP)                                                                 \
    SPFM_DISPATCH(dtype, SPFM_DISPATCH_L(k, hipLaunchKernelGGL(                                  \
        (psgd_pair_sample_kernel<T, L, WARP>), dim3(cdiv(m, kBlock / L)), dim3(kBlock), 0,       \
        stream, (int)m, (int)n_negatives, (int)n_candidates, (int)max_draws, (uint64_t)seed,     \
        (uint64_t)epoch, (int)sm_nctx, (int)sm_ncand, sm_posrow.as<int32_t>(),                   \
        sm_posidx.as<int32_t>(), sm_fptr.as<int64_t>(), sm_fidx.as<int32_t>(),                   \
        order ? sg_order.as<int32_t>() : (const int32_t*)nullptr, rptr.as<int64_t>(),            \
        ridx.as<int32_t>(), rval.as<T>(), Pt.as<double>(), w.as<double>(), lams.as<double>(),    \
        n_orders, k, d, degree, sg_triples.as<int32_t>(), sg_scores.as<double>(),                \
        have_proposal ? sm_cum.as<uint32_t>() : (const uint32_t*)nullptr, sm_cumW,               \
        have_posw ? sm_posw.as<double>() : (const double*)nullptr, margin,                       \
        wr ? sg_weights.as<double>() : (double*)nullptr,                                         \
        WARP ? sg_trials.as<int32_t>() : (int32_t*)nullptr)))
    if (warp)
        SPFM_SAMPLE_LAUNCH(true);
    else
        SPFM_SAMPLE_LAUNCH(false);
#undef SPFM_SAMPLE_LAUNCH
    HIPC(hipGetLastError());
    if (triples_out) SPFM_TRY(download(triples_out, sg_triples.p, 3 * (size_t)m));
    if (scores_out) SPFM_TRY(download(scores_out, sg_scores.p, (size_t)m));
    if (weights_out && wr) SPFM_TRY(download(weights_out, sg_weights.p, (size_t)m));
    if (trials_out && warp) SPFM_TRY(download(trials_out, sg_trials.p, (size_t)m));
    HIPC(hipStreamSynchronize(stream));  // order may be reused; the copies have landed
    sampled = true;
    sampled_weighted = wr;
    sampled_m = m;
    sampled_nneg = n_negatives;
    sampled_slots = order != nullptr;
    return SPFM_OK;
}

int spfm_engine::psgd_pairs_sample(int degree, int64_t n_negatives, int64_t n_candidates,
                                   int64_t max_draws, int64_t seed, int64_t epoch,
                                   const int32_t* order, int32_t* triples_out,
                                   double* scores_out) {
    return psgd_pairs_sample_any(false, degree, n_negatives, n_candidates, max_draws, 0.0, seed,
                                 epoch, order, triples_out, scores_out, nullptr, nullptr);
}

// the epoch of psgd_pairs_epoch over the list the sample call left on the device: nothing is
// uploaded and nothing re-checked (the list is valid by construction)
int spfm_engine::psgd_pairs_epoch_sampled(const PsgdStep& st, double* sum_loss) {
    if (dist()) FAIL(SPFM_ERR_UNSUPPORTED, "psgd pairs: several ranks are not supported");
    SPFM_TRY(psgd_ready("psgd pairs", st.degree));
    if (!sampled)
        FAIL(SPFM_ERR_INVALID, "psgd pairs: the resident triple list is not the output of "
                               "spfm_psgd_pairs_sample");
    if (const std::string e = st.check("psgd pairs"); !e.empty()) FAIL(SPFM_ERR_INVALID, e);
    SPFM_TRY(ensure_pt());
    return psgd_pairs_run(st, sampled_m, sum_loss, sampled_weighted);
}

// ============================================================ listwise ranking fit
//  a positive with its n_negatives negatives is one training item

static_assert(kListMaxNeg == SPFM_LIST_MAX_NEG && kListSoftmax == SPFM_LIST_SOFTMAX &&
                  kListPairMean == SPFM_LIST_PAIRMEAN,
              "spfm.h and spfm_psgd_lists.hip.h disagree");

// the list arguments of every list entry, in `what`'s words; empty: none failed
static std::string lists_args_error(const char* what, int64_t n_negatives, int list_loss) {
    const char* e = (n_negatives < 1 || n_negatives > SPFM_LIST_MAX_NEG)
                        ? "n_negatives must be in [1, SPFM_LIST_MAX_NEG = 63]"
                    : (list_loss != SPFM_LIST_SOFTMAX && list_loss != SPFM_LIST_PAIRMEAN)
                        ? "list_loss must be SPFM_LIST_SOFTMAX or SPFM_LIST_PAIRMEAN"
                        : nullptr;
    return e ? std::string(what) + ": " + e : std::string();
}

// Argument checks of the two list entries that take triples, on the host, before any launch:
// those of the pair entries, the list arguments, and the grouping of the rows.
int spfm_engine::psgd_lists_check(const char* what, int degree, const int32_t* triples, int64_t m,
                                  int64_t n_negatives, int list_loss) {
    SPFM_TRY(psgd_pairs_check(what, degree, triples, m));
    if (const std::string e = lists_args_error(what, n_negatives, list_loss); !e.empty())
        FAIL(SPFM_ERR_INVALID, e);
    if (m % n_negatives != 0)
        FAIL(SPFM_ERR_INVALID, std::string(what) + ": m is not a multiple of n_negatives");
    for (int64_t q = 0; q < m; ++q) {
        const int64_t q0 = q - q % n_negatives;
        if (triples[3 * q] != triples[3 * q0] || triples[3 * q + 1] != triples[3 * q0 + 1])
            FAIL(SPFM_ERR_INVALID, std::string(what) + ": triple " + std::to_string(q) +
                                       " differs from the first of its list in anchor or plus: "
                                       "the triples must be grouped by list");
    }
    return SPFM_OK;
}

template <typename T, int L>
int spfm_engine::psgd_lists_epoch_tl(const PsgdStep& st, int64_t n_lists, int M, int list_loss,
                                     bool ordered) {
    auto grad = [&](int64_t pos, int B, int grid, bool table) {
        hipLaunchKernelGGL((psgd_list_grad_kernel<T, L, false>), dim3(grid), dim3(kBlock), 0,
                           stream, sg_triples.as<int32_t>(),
                           ordered ? sg_listorder.as<int32_t>() : (const int32_t*)nullptr,
                           (long long)pos, B, M, list_loss, rptr.as<int64_t>(),
                           ridx.as<int32_t>(), rval.as<T>(), Pt.as<double>(), w.as<double>(),
                           lams.as<double>(), n_orders, k, d, st.degree, loss, st.fit_linear,
                           sg_gradP.as<double>(), sg_gradw.as<double>(), sg_lossrow.as<double>(),
                           (int*)nullptr,
                           table ? sg_sched.as<PsgdBatch>() : (const PsgdBatch*)nullptr,
                           table ? sg_idx.as<int>() : (int*)nullptr);
    };
    // the recorded kernel arguments hold M, list_loss and the order pointer: part of the graph key
    const std::string tag = "psgd_lists|" + std::to_string(M) + "|" + std::to_string(list_loss) +
                            "|" + std::to_string((int)ordered);
    return psgd_batches_tl<L>(grad, tag.c_str(), (int64_t)sizeof(T), n_lists, st);
}

// the batches over the lists of the resident grouped triples and the sum of the lists' losses
int spfm_engine::psgd_lists_run(const PsgdStep& st, int64_t n_lists, int M, int list_loss,
                                bool ordered, double* sum_loss) {
    p_valid = false;
    SPFM_TRY(SPFM_DISPATCH(dtype, return SPFM_DISPATCH_L(k, return psgd_lists_epoch_tl<T, L>(
                                                                 st, n_lists, M, list_loss,
                                                                 ordered))));
    return psgd_epoch_end(sg_lossrow.as<double>(), n_lists, sum_loss);
}

int spfm_engine::psgd_lists_epoch(const PsgdStep& st, const int32_t* triples, int64_t m,
                                  int64_t n_negatives, int list_loss, double* sum_loss) {
    if (dist()) FAIL(SPFM_ERR_UNSUPPORTED, "psgd lists: several ranks are not supported");
    SPFM_TRY(psgd_lists_check("psgd lists", st.degree, triples, m, n_negatives, list_loss));
    if (const std::string e = st.check("psgd lists"); !e.empty()) FAIL(SPFM_ERR_INVALID, e);
    if (m == 0) {
        if (sum_loss) *sum_loss = 0.0;
        return SPFM_OK;
    }
    SPFM_TRY(ensure_pt());
    SPFM_TRY(pairs_reserve(m));
    SPFM_TRY(upload_to(sg_triples.p, triples, 3 * (size_t)m));
    HIPC(hipStreamSynchronize(stream));  // caller may reuse triples
    return psgd_lists_run(st, m / n_negatives, (int)n_negatives, list_loss, false, sum_loss);
}

// the epoch of psgd_lists_epoch over the list the sample call left on the device: nothing is
// re-checked but that the sample call grouped it the way this call reads it
int spfm_engine::psgd_lists_epoch_sampled(const PsgdStep& st, int64_t n_negatives, int list_loss,
                                          const int32_t* list_order, double* sum_loss) {
    if (dist()) FAIL(SPFM_ERR_UNSUPPORTED, "psgd lists: several ranks are not supported");
    SPFM_TRY(psgd_ready("psgd lists", st.degree));
    if (!sampled)
        FAIL(SPFM_ERR_INVALID, "psgd lists: the resident triple list is not the output of "
                               "spfm_psgd_pairs_sample");
    if (const std::string e = lists_args_error("psgd lists", n_negatives, list_loss); !e.empty())
        FAIL(SPFM_ERR_INVALID, e);
    if (sampled_weighted)
        FAIL(SPFM_ERR_INVALID, "psgd lists: the sample call wrote weights (positive weights or "
                               "WARP); the list objectives take none");
    if (sampled_slots)
        FAIL(SPFM_ERR_INVALID, "psgd lists: the sample call scattered its triples by `order`; "
                               "lists need order == NULL");
    if (sampled_nneg != n_negatives)
        FAIL(SPFM_ERR_INVALID, "psgd lists: the sample call drew " + std::to_string(sampled_nneg) +
                                   " negatives per positive, not " + std::to_string(n_negatives));
    if (const std::string e = st.check("psgd lists"); !e.empty()) FAIL(SPFM_ERR_INVALID, e);
    const int64_t n_lists = sampled_m / n_negatives;
    if (list_order && !is_permutation(list_order, n_lists))
        FAIL(SPFM_ERR_INVALID, "psgd lists: list_order is not a permutation of the lists");
    SPFM_TRY(ensure_pt());
    if (list_order) {
        const void* old = sg_listorder.p;
        HIPC(sg_listorder.alloc(sizeof(int32_t) * (size_t)n_lists));
        if (sg_listorder.p != old) clear_graphs();
        SPFM_TRY(upload_to(sg_listorder.p, list_order, (size_t)n_lists));
        HIPC(hipStreamSynchronize(stream));  // caller may reuse list_order
    }
    return psgd_lists_run(st, n_lists, (int)n_negatives, list_loss, list_order != nullptr,
                          sum_loss);
}

// loss sum and number of lists whose positive scores first at the live parameters; nothing is
// updated
int spfm_engine::psgd_lists_eval(int degree, int fit_linear, const int32_t* triples, int64_t m,
                                 int64_t n_negatives, int list_loss, double* sum_loss,
                                 int64_t* n_first) {
    (void)fit_linear;  // the scores read w as it stands (zeros when no linear term was fitted)
    if (dist()) FAIL(SPFM_ERR_UNSUPPORTED, "psgd lists eval: several ranks are not supported");
    SPFM_TRY(psgd_lists_check("psgd lists eval", degree, triples, m, n_negatives, list_loss));
    if (sum_loss) *sum_loss = 0.0;
    if (n_first) *n_first = 0;
    if (m == 0) return SPFM_OK;
    const int64_t n_lists = m / n_negatives;
    SPFM_TRY(ensure_pt());
    SPFM_TRY(pairs_reserve(m));
    HIPC(sg_ordered.alloc(sizeof(int) * (size_t)n_lists));
    SPFM_TRY(upload_to(sg_triples.p, triples, 3 * (size_t)m));
    SPFM_DISPATCH(dtype, SPFM_DISPATCH_L(k, hipLaunchKernelGGL(
        (psgd_list_grad_kernel<T, L, true>), dim3(cdiv(n_lists, kBlock / L)), dim3(kBlock), 0,
        stream, sg_triples.as<int32_t>(), (const int32_t*)nullptr, 0LL, (int)n_lists,
        (int)n_negatives, list_loss, rptr.as<int64_t>(), ridx.as<int32_t>(), rval.as<T>(),
        Pt.as<double>(), w.as<double>(), lams.as<double>(), n_orders, k, d, degree, loss, 0,
        (double*)nullptr, (double*)nullptr, sg_lossrow.as<double>(), sg_ordered.as<int>(),
        (const PsgdBatch*)nullptr, (int*)nullptr)));
    loss_sum(sg_lossrow.as<double>(), n_lists, 0);
    loss_sum(sg_ordered.as<int>(), n_lists, 1);
    HIPC(hipGetLastError());
    SPFM_TRY(download(h_scalar, scalar.p, 2));
    HIPC(hipStreamSynchronize(stream));
    if (sum_loss) *sum_loss = h_scalar[0];
    if (n_first) *n_first = (int64_t)h_scalar[1];
    return SPFM_OK;
}

extern "C" {

int spfm_psgd_epoch(spfm_handle h, int degree, double alpha, double beta, double gamma,
                    double eta0, int learning_rate, double power_t, int64_t batch_size,
                    const int32_t* indices_samples, int64_t n_samples, int fit_linear,
                    int64_t* it, double* sum_loss) {
    SPFM_GUARD(h);
    if (h->dist()) {
        h->err = "psgd: several ranks share this handle's communicator -- use spfm_psgd_epoch_sharded";
        return SPFM_ERR_INVALID;
    }
    const PsgdStep st = h->psgd_step(degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                                      batch_size, fit_linear, it);
    return h->psgd_epoch(st, indices_samples, n_samples, 0, sum_loss);
}

int spfm_psgd_epoch_sharded(spfm_handle h, int degree, double alpha, double beta, double gamma,
                            double eta0, int learning_rate, double power_t, int64_t batch_size,
                            const int32_t* indices_samples, int64_t n_global, int64_t row_lo,
                            int fit_linear, int64_t* it, double* sum_loss) {
    SPFM_GUARD(h);
    SPFM_TRY(h->refuse_weighted("psgd (sharded)"));
    const PsgdStep st = h->psgd_step(degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                                      batch_size, fit_linear, it);
    return h->psgd_epoch(st, indices_samples, n_global, row_lo, sum_loss);
}

int spfm_psgd_set_adaptive(spfm_handle h, int mode, double initial_accumulator,
                           const double* acc_P, const double* acc_w) {
    SPFM_GUARD(h);
    return h->psgd_set_adaptive(mode, initial_accumulator, acc_P, acc_w);
}

int spfm_psgd_get_adaptive(spfm_handle h, double* acc_P, double* acc_w) {
    SPFM_GUARD(h);
    return h->psgd_get_adaptive(acc_P, acc_w);
}

int spfm_psgd_pairs_set_sampler(spfm_handle h, int64_t n_ctx, int64_t n_cand,
                                const int64_t* pos_ptr, const int32_t* pos_idx,
                                const int64_t* forb_ptr, const int32_t* forb_idx) {
    SPFM_GUARD(h);
    return h->psgd_pairs_set_sampler(n_ctx, n_cand, pos_ptr, pos_idx, forb_ptr, forb_idx);
}

int spfm_psgd_pairs_sample(spfm_handle h, int degree, int64_t n_negatives, int64_t n_candidates,
                           int64_t max_draws, int64_t seed, int64_t epoch, const int32_t* order,
                           int32_t* triples_out, double* scores_out) {
    SPFM_GUARD(h);
    return h->psgd_pairs_sample(degree, n_negatives, n_candidates, max_draws, seed, epoch, order,
                                triples_out, scores_out);
}

int spfm_psgd_pairs_set_proposal(spfm_handle h, const uint32_t* cum, int64_t n_cand) {
    SPFM_GUARD(h);
    return h->psgd_pairs_set_proposal(cum, n_cand);
}

int spfm_psgd_pairs_set_positive_weights(spfm_handle h, const double* wq, int64_t nnz) {
    SPFM_GUARD(h);
    return h->psgd_pairs_set_positive_weights(wq, nnz);
}

int spfm_psgd_pairs_sample_warp(spfm_handle h, int degree, int64_t n_negatives,
                                int64_t max_trials, int64_t max_draws, double margin,
                                int64_t seed, int64_t epoch, const int32_t* order,
                                int32_t* triples_out, double* scores_out, double* weights_out,
                                int32_t* trials_out) {
    SPFM_GUARD(h);
    return h->psgd_pairs_sample_any(true, degree, n_negatives, max_trials, max_draws, margin, seed,
                                    epoch, order, triples_out, scores_out, weights_out,
                                    trials_out);
}

int spfm_psgd_pairs_epoch_weighted(spfm_handle h, int degree, double alpha, double beta,
                                   double gamma, double eta0, int learning_rate, double power_t,
                                   int64_t batch_size, const int32_t* triples,
                                   const double* weights, int64_t m, int fit_linear, int64_t* it,
                                   double* sum_loss) {
    SPFM_GUARD(h);
    const PsgdStep st = h->psgd_step(degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                                      batch_size, fit_linear, it);
    return h->psgd_pairs_epoch_weighted(st, triples, weights, m, sum_loss);
}

int spfm_psgd_pairs_epoch_sampled(spfm_handle h, int degree, double alpha, double beta,
                                  double gamma, double eta0, int learning_rate, double power_t,
                                  int64_t batch_size, int fit_linear, int64_t* it,
                                  double* sum_loss) {
    SPFM_GUARD(h);
    const PsgdStep st = h->psgd_step(degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                                      batch_size, fit_linear, it);
    return h->psgd_pairs_epoch_sampled(st, sum_loss);
}

int spfm_psgd_pairs_epoch(spfm_handle h, int degree, double alpha, double beta, double gamma,
                          double eta0, int learning_rate, double power_t, int64_t batch_size,
                          const int32_t* triples, int64_t m, int fit_linear, int64_t* it,
                          double* sum_loss) {
    SPFM_GUARD(h);
    const PsgdStep st = h->psgd_step(degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                                      batch_size, fit_linear, it);
    return h->psgd_pairs_epoch(st, triples, m, sum_loss);
}

int spfm_psgd_pairs_eval(spfm_handle h, int degree, int fit_linear, const int32_t* triples,
                         int64_t m, double* sum_loss, int64_t* n_ordered) {
    SPFM_GUARD(h);
    return h->psgd_pairs_eval(degree, fit_linear, triples, m, sum_loss, n_ordered);
}

int spfm_psgd_lists_epoch(spfm_handle h, int degree, double alpha, double beta, double gamma,
                          double eta0, int learning_rate, double power_t, int64_t batch_size,
                          const int32_t* triples, int64_t m, int64_t n_negatives, int list_loss,
                          int fit_linear, int64_t* it, double* sum_loss) {
    SPFM_GUARD(h);
    const PsgdStep st = h->psgd_step(degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                                      batch_size, fit_linear, it);
    return h->psgd_lists_epoch(st, triples, m, n_negatives, list_loss, sum_loss);
}

int spfm_psgd_lists_epoch_sampled(spfm_handle h, int degree, double alpha, double beta,
                                  double gamma, double eta0, int learning_rate, double power_t,
                                  int64_t batch_size, int64_t n_negatives, int list_loss,
                                  const int32_t* list_order, int fit_linear, int64_t* it,
                                  double* sum_loss) {
    SPFM_GUARD(h);
    const PsgdStep st = h->psgd_step(degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                                      batch_size, fit_linear, it);
    return h->psgd_lists_epoch_sampled(st, n_negatives, list_loss, list_order, sum_loss);
}

int spfm_psgd_lists_eval(spfm_handle h, int degree, int fit_linear, const int32_t* triples,
                         int64_t m, int64_t n_negatives, int list_loss, double* sum_loss,
                         int64_t* n_first) {
    SPFM_GUARD(h);
    return h->psgd_lists_eval(degree, fit_linear, triples, m, n_negatives, list_loss, sum_loss,
                              n_first);
}

}  // extern "C"
