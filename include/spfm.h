/*
 * spfm.h -- C ABI of the MI355X (gfx950) sparse factorization-machine
 * proximal coordinate-descent core (libspfm_hip.so).
 *
 * This is the drop-in boundary for the hot path of neonnnnn/sparsepoly:
 * every entry point replaces one interpreter->Numba call (or one NumPy block)
 * of the reference's epoch drivers.  Citations are into the reference tree
 * (sparsepoly/...).  Plain pointers and sizes only; no C++/torch types; no
 * exception crosses the boundary.  All host buffers stay owned by the caller
 * and are copied during the call.
 *
 * Conventions
 *   return 0 = ok; <0 = error (spfm_last_error() gives the text)
 *     SPFM_ERR_INVALID      -> the reference raises ValueError for this input
 *     SPFM_ERR_RUNTIME      -> HIP/RCCL failure
 *     SPFM_ERR_UNSUPPORTED  -> valid for the reference, outside this library
 *   A handle is not thread-safe; distinct handles are independent.  Each handle
 *   owns one HIP stream; calls return after the stream has drained unless noted.
 *   Host arrays are float64 / int32 / int64 as in the reference
 *   (dataset.py:60-66, base.py:41-49); device storage precision is the handle's
 *   dtype (values, A caches, y_pred in f32 or f64; reductions, prox and
 *   parameters always f64).
 */
#ifndef SPFM_H
#define SPFM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spfm_engine* spfm_handle;

#define SPFM_OK 0
#define SPFM_ERR_INVALID (-1)
#define SPFM_ERR_RUNTIME (-2)
#define SPFM_ERR_UNSUPPORTED (-3)

/* storage precision of X values, A caches, y_pred, y on the device */
#define SPFM_F32 0
#define SPFM_F64 1

/* loss.py:74-80 registries */
#define SPFM_LOSS_SQUARED 0
#define SPFM_LOSS_SQUARED_HINGE 1
#define SPFM_LOSS_LOGISTIC 2

/* regularizer/__init__.py:8-15 */
#define SPFM_REG_L1 0
#define SPFM_REG_L21 1
#define SPFM_REG_SQUAREDL12 2
#define SPFM_REG_SQUAREDL21 3
#define SPFM_REG_OMEGATI 4
#define SPFM_REG_OMEGACS 5

#define SPFM_SOLVER_PCD 0
#define SPFM_SOLVER_PBCD 1
#define SPFM_SOLVER_PSGD 2

/* coordinate schedules (spfm_set_schedule) */
#define SPFM_SCHED_EXACT 0   /* keep the given order; batch = maximal run of row-disjoint columns */
#define SPFM_SCHED_COLORED 1 /* first-fit colouring of the column conflict graph; order is permuted */
#define SPFM_SCHED_COLORED_RLF 2 /* RLF colouring: fewer classes, longer set-up; order is permuted */

#define SPFM_MAX_DEGREE 6

/* -- lifetime ------------------------------------------------------------ */
int spfm_create(spfm_handle* out, int device_id, int dtype);
void spfm_destroy(spfm_handle h);
/* h may be NULL: returns the calling thread's last creation error */
const char* spfm_last_error(spfm_handle h);
/* library / device identification, e.g. "gfx950:sramecc+:xnack-" */
int spfm_device_name(spfm_handle h, char* out, int cap);
/* 12 hex digits: hash of the library's sources at build time (csrc/build.sh).  No handle and
 * no device needed.  Measurements kept under profiles/ record it, so a counter file is only
 * ever quoted for the code it was collected with. */
const char* spfm_build_tag(void);

/* -- data ------------------------------------------------------------------
 * Replaces get_dataset(X, order="fortran") (dataset.py:119-123, CSCDataset
 * :94-116) plus col_norm_sq = row_norms(X.T, squared=True)
 * (sparse_factorization_machines.py:406-409).  CSC of the LOCAL row shard:
 * indptr[d+1] (int64), indices[nnz] (int32 row ids in [0,n)), data[nnz], y[n].
 * The library also builds the CSR image it needs for the row-oriented passes. */
int spfm_set_data_csc(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                      const int32_t* indices, const double* data, const double* y);

/* The same from a CSR matrix (what scipy hands the estimators most of the time): indptr[n+1]
 * (int64), indices[nnz] (int32 column ids, sorted and duplicate-free inside each row), data,
 * y[n].  Replaces X.tocsc() of get_dataset as well: the CSC image is built inside, by host
 * threads (SPFM_THREADS, default min(cores, 16)). */
int spfm_set_data_csr(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                      const int32_t* indices, const double* data, const double* y);

/* Several handles on ONE training matrix: the fits of a regularisation path or a
 * parameter grid -- the use-case the reference serves with warm_start chains
 * (sparse_factorization_machines.py:380-391) -- and one-vs-rest targets (base.py:130-136).  `dst`
 * refers to the device image `src` holds (CSC, CSR, column norms) instead of uploading and
 * transposing its own copy, and the two share the entry streams of the persistent passes either
 * of them builds later.  Same device and storage type, no communicator.  `y` (n doubles): dst's
 * own targets, or NULL = src's.  The image is freed with its last holder; a later
 * spfm_set_data_* on either handle detaches that handle only. */
int spfm_share_data(spfm_handle dst, spfm_handle src, const double* y);

/* -- row weights ---------------------------------------
 * weights[n] for the rows of the handle's training data; NULL clears.  n must equal the data's.
 * Every loss term becomes w_i * loss(yhat_i, y_i): the column sums of pcd / pbcd / cd_linear
 * are g = sum_i (w_i dloss_i) dA_ij and h = sum_i (w_i dA_ij) dA_ij (cd_linear: the weighted
 * column norm sum_i w_i x_ij^2, formed here, once), psgd's row gradient and row loss are scaled
 * by w_i while the minibatch gradient is still divided by the number of rows of the minibatch,
 * and spfm_loss_sum returns sum_i w_i loss_i.  Integer weights are row replication (up to
 * summation order); a zero-weight row keeps its prediction maintained and enters no sum.
 * Weights belong to the handle, like the targets: co-tenants of one image (spfm_share_data) carry
 * their own, and spfm_set_data_* / spfm_share_data on the handle clear them.  While weights are
 * set the epochs run on the multi-kernel engine and the psgd kernels -- the persistent passes
 * are not used ("persistent_active" reads 0) -- and an installed schedule stays valid.  Memory:
 * 8 n + 8 d bytes.
 * SPFM_ERR_INVALID: no data, n differs, a negative or non-finite weight, all weights zero.
 * SPFM_ERR_UNSUPPORTED: a communicator is attached.  On a weighted handle the triple and list
 * entries (spfm_psgd_pairs_*, spfm_psgd_lists_*), spfm_psgd_epoch_sharded and the host-stepped
 * epochs (spfm_host_*) return SPFM_ERR_UNSUPPORTED; spfm_eval_loss, spfm_foldin_csr and the
 * bank entries do not read the weights. */
int spfm_set_sample_weight(spfm_handle h, const double* weights, int64_t n);
/* set_out: 0/1; sum_out: sum of the weights (n when none are set).  Either may be NULL. */
int spfm_get_sample_weight(spfm_handle h, int* set_out, double* sum_out);

/* -- parameters -------------------------------------------------------------
 * P is (n_orders, k, d) row-major as self.P_ (sparse_factorization_machines.py
 * :383-389), w (d), lams (k, each +-1: :403-404).  d must equal the data's
 * n_features when data is present; a handle without data (predict only) takes d
 * from here.  get copies the live device state back (pcd callbacks see live P_,
 * :227-228). */
int spfm_set_params(spfm_handle h, int n_orders, int k, int32_t d, const double* P,
                    const double* w, const double* lams);
int spfm_get_params(spfm_handle h, double* P, double* w);

/* -- configuration ----------------------------------------------------------
 * loss (base.py:18-25), regularizer (base.py:27-34) and the solver whose cache
 * protocol is initialised: regularizer.init_cache_pcd / init_cache_pbcd(degree,
 * d, k) (sparse_factorization_machines.py:194,282).  Errors as the reference:
 * SquaredL12 degree>2 / SquaredL21 degree!=2 -> SPFM_ERR_INVALID
 * (squaredl12.py:25-26, squaredl21.py:28-29); solver/regularizer pairs the
 * reference cannot run (README.md:28-32) -> SPFM_ERR_INVALID. */
int spfm_configure(spfm_handle h, int solver, int loss, int regularizer, int top_degree);

/* -- initial prediction ----------------------------------------------------
 * y_pred = _get_output(X) (sparse_factorization_machines.py:437-451, kernels.py
 * :71-115,140-153): ANOVA kernel of order `degree` on P[0], + X.w if fit_linear,
 * + the order-2 term on P[1] if add_lower_deg2 (fit_lower='explicit', degree 3). */
int spfm_init_pred(spfm_handle h, int degree, int fit_linear, int add_lower_deg2);
int spfm_get_y_pred(spfm_handle h, double* out);
/* sum_i loss(y_pred_i, y_i) (loss.py:20-21,34-42,61-65) of the local shard; with sample weights
 * set, sum_i w_i loss(y_pred_i, y_i) */
int spfm_loss_sum(spfm_handle h, double* out);

/* Same computation on a caller-supplied CSR matrix (predict(),
 * sparse_factorization_machines.py:453-458).  indptr[n+1] int64, indices int32
 * column ids in [0,d). */
int spfm_predict_csr(spfm_handle h, int64_t n, const int64_t* indptr, const int32_t* indices,
                     const double* data, int degree, int fit_linear, int add_lower_deg2,
                     double* out);

/* -- coordinate schedule ----------------------------------------------------
 * The reference's epoch functions take the visiting order as an argument
 * (indices_feature: pcd.py:86-87,97; pbcd.py:99,110; cd_linear.py:8,10).
 * This call fixes the order for the following epochs and partitions it into
 * batches of columns that share no row, which the device processes as one
 * dependent step (results equal the sequential sweep in `order_out`).
 *   conflict_indptr/indices: CSC structure used for the disjointness test; pass
 *     NULL to use the local data (single process).  Multi-GPU: pass the GLOBAL
 *     structure so that all ranks derive the identical schedule.
 *   order_out[d]: the order actually used (== indices_feature for EXACT).
 *   n_batches_out: number of dependent steps per sweep.
 * SPFM_SCHED_COLORED_RLF is accepted wherever SPFM_SCHED_COLORED is and yields the same product
 * under the same class caps, with fewer classes (hence fewer dependent steps per sweep) for a
 * longer set-up.  It builds one class at a time as a maximal independent set: the first member
 * maximises the sum, over its rows, of the uncoloured columns on the row; every later member
 * maximises the sum, over its rows, of the candidates that already left the class on that row (a
 * candidate leaves when it shares a row with a member); ties go to the column that comes first
 * in indices_feature.  Integer keys: the device form ("colour_device", the same size threshold
 * as the first fit; SPFM_RLF_DEVICE=1 in the environment lifts the threshold, for tests) equals
 * the host form exactly.  Opt-in: SPFM_SCHED_COLORED is unchanged. */
int spfm_set_schedule(spfm_handle h, int mode, const int32_t* indices_feature,
                      const int64_t* conflict_indptr, const int32_t* conflict_indices,
                      int64_t conflict_n_rows, int32_t* order_out, int32_t* n_batches_out);

/* Install a schedule computed earlier (spfm_schedule_build / a cached product of a
 * previous fit on the same data): order[d] and batch_ptr[n_batches+1].  The library
 * re-checks that `order` is a permutation and that every batch is row-disjoint on the
 * structure it would have used to build it (conflict_* as in spfm_set_schedule, NULL =
 * local data), because a batch that shares a row would race; SPFM_ERR_INVALID otherwise. */
int spfm_set_schedule_raw(spfm_handle h, const int32_t* order, const int32_t* batch_ptr,
                          int32_t n_batches, const int64_t* conflict_indptr,
                          const int32_t* conflict_indices, int64_t conflict_n_rows);

/* Read back the installed schedule: order_out[d], batch_ptr_out[n_batches+1] (either may
 * be NULL); n_batches_out receives the number of batches. */
int spfm_get_schedule(spfm_handle h, int32_t* order_out, int32_t* batch_ptr_out,
                      int32_t* n_batches_out);

/* Host-only form of the batch construction (no handle, no device): fills
 * order_out[d] and batch_ptr_out[<= d+1] (batch b = order_out[batch_ptr[b] ..
 * batch_ptr[b+1])) and returns the number of batches in n_batches_out.
 * max_batch <= 0 selects the library default (4096 columns per step). */
int spfm_schedule_build(int mode, int64_t n_rows, int32_t d, const int64_t* indptr,
                        const int32_t* indices, const int32_t* indices_feature, int max_batch,
                        int32_t* order_out, int32_t* batch_ptr_out, int32_t* n_batches_out);

/* -- epochs ------------------------------------------------------------------
 * One call = one reference epoch function call.  viol receives sum_viol. */

/* cd_linear._cd_linear_epoch (optimizer/cd_linear.py:8-33) */
int spfm_cd_linear_epoch(spfm_handle h, double alpha, double* viol);

/* pcd.pcd_epoch (optimizer/pcd.py:71-137) on P[order_idx] with `degree`;
 * indices_component[n_comp] as pcd.py:86,92. */
int spfm_pcd_epoch(spfm_handle h, int order_idx, int degree, double beta, double gamma,
                   double eta, const int32_t* indices_component, int n_comp, double* viol);

/* pbcd.pbcd_epoch (optimizer/pbcd.py:82-148) on P[order_idx] */
int spfm_pbcd_epoch(spfm_handle h, int order_idx, int degree, double beta, double gamma,
                    double eta, double* viol);

/* -- host-stepped epochs: user-defined regularizer objects ---------------------------------
 * The reference's regularizers are duck-typed plug-ins (regularizer/__init__.py:8-15,
 * base.py:27-34): any object with init_cache_* / compute_cache_* / prox_cd | prox_bcd /
 * update_cache_* can be registered.  The six built-ins run inside the device chains; for any
 * other object the epoch is stepped from the host.  Between spfm_host_epoch_begin and
 * spfm_host_epoch_end (one reference epoch call; the schedule's dependent steps b = 0 ..
 * n_batches-1 in order, for pcd once per component after spfm_host_pass_begin(s)):
 *   spfm_host_step_sums   the step's column sums: pcd sums_out[ncols][2] = (sum dloss dA,
 *                         sum dA^2) (pcd.py:54-59); pbcd sums_out[ncols][k+1] = grad[0..k),
 *                         sum_s inv_step_sizes[s] (pbcd.py:60-70); all-reduced over the ranks
 *   (caller)              pcd.py:61-68 / pbcd.py:68-79 with the object's prox and cache hooks,
 *                         column by column in the step's visiting order
 *   spfm_host_step_apply  p_new[ncols] (pcd) / p_new, p_old [ncols][k] (pbcd): parameters
 *                         written, rows scatter-updated (pcd.py:119-133 / pbcd.py:135-146)
 * Two host round trips per dependent step: the plug-in surface honoured, not accelerated.
 * sparsepoly_amd.engine.HipEngine.{pcd,pbcd}_epoch_host drive it; the estimators take this path
 * for any registered regularizer that is not one of the six built-in classes. */
int spfm_host_epoch_begin(spfm_handle h, int order_idx, int degree);
int spfm_host_pass_begin(spfm_handle h, int component);
int spfm_host_step_sums(spfm_handle h, int step, double* sums_out);
int spfm_host_step_apply(spfm_handle h, int step, const double* p_new, const double* p_old);
int spfm_host_epoch_end(spfm_handle h, double* viol);

/* psgd.psgd_epoch (optimizer/psgd.py:125-199): one pass over indices_samples (a
 * permutation of 0..n_samples-1; sparse_factorization_machines.py:98,124-125) in
 * minibatches of batch_size rows (the last one may be shorter, psgd.py:177).  Updates
 * every order of P (order o has degree `degree - o`, psgd.py:84-85,120-122) and w.
 *   learning_rate  0 constant | 1 optimal | 2 pegasos | 3 invscaling (psgd.py:9-22,
 *                  sparse_factorization_machines.py:17 LEARNING_RATE)
 *   it             in/out: the reference's self.it_ (starts at 1; +1 per parameter update)
 *   sum_loss       out: sum over samples of loss(y_pred_i, y_i) at visiting time
 * Requires spfm_configure(h, SPFM_SOLVER_PSGD, loss, reg, degree) with reg in {l1, l21,
 * squaredl12, squaredl21}; no schedule is needed.  The training-time y_pred vector
 * (spfm_get_y_pred / spfm_loss_sum) is not maintained by this solver.  One rank; several ranks:
 * spfm_psgd_epoch_sharded. */
int spfm_psgd_epoch(spfm_handle h, int degree, double alpha, double beta, double gamma,
                    double eta0, int learning_rate, double power_t, int64_t batch_size,
                    const int32_t* indices_samples, int64_t n_samples, int fit_linear,
                    int64_t* it, double* sum_loss);
/* The same epoch with the rows sharded over the ranks of the handle's communicator (data-parallel
 * minibatch SGD; the reference has no distributed code -- this is what its loop implies:
 * _update_grads (psgd.py:60-91) sums over the samples of a minibatch, _update_params
 * (psgd.py:94-122) is a function of those sums alone).  The handle holds the rows
 * [row_lo, row_lo + n_local) of a problem of n_global rows; indices_samples is the GLOBAL visiting
 * order (a permutation of 0..n_global-1, identical on every rank).  Every rank forms the gradient
 * of its own samples of a minibatch, the gradients are all-reduced (sum, f64: one collective of
 * n_orders*k*d + d doubles per minibatch), and every rank applies the identical update with the
 * GLOBAL batch size in eta/B -- parameters stay replicated.  sum_loss is the global sum.  Without
 * a communicator (one rank) it is spfm_psgd_epoch. */
int spfm_psgd_epoch_sharded(spfm_handle h, int degree, double alpha, double beta, double gamma,
                            double eta0, int learning_rate, double power_t, int64_t batch_size,
                            const int32_t* indices_samples, int64_t n_global, int64_t row_lo,
                            int fit_linear, int64_t* it, double* sum_loss);

/* Per-feature AdaGrad steps for every epoch entry of the minibatch unit -- spfm_psgd_epoch and the
 * spfm_psgd_pairs_* / spfm_psgd_lists_* epochs.  The mode is handle
 * state: the epoch entries keep their signatures, and their learning_rate / power_t give the BASE
 * rates eta_P, eta_w of a minibatch.  State: A_P (n_orders, d), one f64 accumulator per order and
 * column shared by the column's k components, and A_w (d).  With gbar the minibatch's summed
 * gradient over its B items, per column j of order o
 *   A_P[o,j] += sum_s gbar[o,j,s]^2              (accumulated first)
 *   e         = eta_P / sqrt(initial_accumulator + A_P[o,j])
 *   p[o,j,:]  = (p[o,j,:] - e gbar[o,j,:]) / (1 + e beta), then the l1 / l21 prox of the column
 *               with strength gamma e / (1 + e beta)
 * and, with fit_linear, w[j] likewise with A_w[j], eta_w and alpha.  Every column is shrunk and
 * proxed every minibatch as before; a column that never saw a gradient keeps the rate
 * eta / sqrt(initial_accumulator), the plain rule's for the default 1.0.  `it` advances as before.
 *   mode                 0 off (the plain rules) | 1 per-feature AdaGrad
 *   initial_accumulator  G0 > 0, finite
 *   acc_P, acc_w         n_orders*d and d values >= 0 to start from (a warm start); NULL: zeros
 * The call always (re)sets both accumulators; they survive spfm_set_params and epochs and are
 * cleared by this call or spfm_destroy alone.  SPFM_ERR_INVALID: a mode other than 0 / 1,
 * initial_accumulator <= 0 or not finite, a negative or non-finite accumulator value, a handle
 * without parameters.  In mode 1 every epoch entry returns SPFM_ERR_INVALID before anything is
 * launched (the parameters stay as they were) when the handle is configured with squaredl12 /
 * squaredl21 -- their prox couples columns that now carry different steps, which the support
 * search of the plain rule does not solve --, when it has a communicator (several ranks), or when
 * the parameters' n_orders / d changed since this call. */
int spfm_psgd_set_adaptive(spfm_handle h, int mode, double initial_accumulator,
                           const double* acc_P, const double* acc_w);
/* The accumulators as they stand (either pointer may be NULL).  SPFM_ERR_INVALID before the first
 * spfm_psgd_set_adaptive. */
int spfm_psgd_get_adaptive(spfm_handle h, double* acc_P, double* acc_w);

/* Pairwise ranking fit: one pass of minibatch psgd over triples.  The
 * handle's data is the stacked matrix [X; Z] (contexts, then candidates; the targets are not
 * read).  Row k of `triples` (m, 3) is (anchor, plus, minus), three row indices into that matrix:
 * context row `anchor` prefers candidate `plus` to candidate `minus`.  With
 *   margin = f(x_anchor + z_plus) - f(x_anchor + z_minus)
 * the loss of a triple is loss(margin, +1) with the configured loss ('logistic': BPR); the
 * penalties, the step sizes, the prox, `it` and the options "psgd_eager", "psgd_graph_sweeps",
 * "psgd_redone" are those of spfm_psgd_epoch.  The visiting order is the order of `triples` (the
 * caller shuffles); minibatch bi covers the triples [bi * batch_size, ...), the last one may be
 * shorter, and eta / B uses the triple count of the batch.  sum_loss: the sum of the per-triple
 * losses at visiting time.  The linear weights of the anchors' columns receive no gradient (their
 * term cancels in the margin); with alpha > 0 they only shrink.
 * Requires spfm_configure(h, SPFM_SOLVER_PSGD, loss, reg, degree).  SPFM_ERR_INVALID, checked on
 * the host before anything is launched (the parameters stay as they were): a row index outside
 * [0, n), plus == minus, a column stored in an anchor row and in a plus / minus row, batch_size
 * < 1, *it < 1, an unsupported learning_rate, a handle not configured for psgd.  A handle with a
 * communicator: SPFM_ERR_UNSUPPORTED. */
int spfm_psgd_pairs_epoch(spfm_handle h, int degree, double alpha, double beta, double gamma,
                          double eta0, int learning_rate, double power_t, int64_t batch_size,
                          const int32_t* triples /* (m,3): anchor, plus, minus rows */,
                          int64_t m, int fit_linear, int64_t* it, double* sum_loss);
/* The same triples at the live device parameters, nothing updated: sum_loss = sum of
 * loss(margin, +1), n_ordered = number of triples with margin > 0.  Same preconditions and
 * argument errors as spfm_psgd_pairs_epoch. */
int spfm_psgd_pairs_eval(spfm_handle h, int degree, int fit_linear, const int32_t* triples,
                         int64_t m, double* sum_loss, int64_t* n_ordered);

/* Negatives of the pairwise fit drawn on the device.  Rows [0, n_ctx) of
 * the handle's data are the contexts and the next n_cand rows the candidates (n_ctx + n_cand ==
 * n).  pos_ptr / pos_idx: the positives as a CSR over (n_ctx, n_cand); forb_ptr / forb_idx: the
 * candidates that may not be drawn for a context, a CSR of the same shape that contains the
 * positives (NULL, NULL: the positives themselves).  Both are uploaded once and stay until the next
 * spfm_set_data_* / spfm_share_data.  Checked once, on the host (SPFM_ERR_INVALID): n_ctx + n_cand
 * != n, no positive, an index outside [0, n_cand) or not strictly ascending within its row, a
 * positive the forbidden set lacks, a context with a positive whose row forbids all n_cand
 * candidates, a column stored both in a context row that has a positive and in a candidate row. */
int spfm_psgd_pairs_set_sampler(spfm_handle h, int64_t n_ctx, int64_t n_cand,
                                const int64_t* pos_ptr, const int32_t* pos_idx,
                                const int64_t* forb_ptr, const int32_t* forb_idx);
/* Fills the device-resident triple list with m = nnz(positives) * n_negatives triples (m < 2^31):
 * triple r = q * n_negatives + i is the i-th negative of positive q (canonical CSR order).  Draw t
 * of triple r is draw_u64(seed, epoch, r, t) (stateless, integer only), its
 * candidate ((u >> 32) * n_cand) >> 32; a draw is admitted when its candidate is not forbidden for
 * the context.  Among the first n_candidates admitted draws with t < max_draws (fewer: those; none:
 * the first admissible candidate upwards, cyclically, from the last drawn one) the negative is the
 * one with the largest score sum_o sum_s lams_s a_s^{degree-o}(x_b + z_c) + <w, z_c> at the live
 * parameters, ties to the earliest draw; n_candidates == 1 scores nothing (uniform negatives, the
 * scores are 0).  Triple r goes to slot order[r] (order: NULL or a permutation of 0..m-1, checked
 * on the host) as (b, n_ctx + c+, n_ctx + c-).  triples_out (m, 3) / scores_out (m): optional host
 * copies, by slot.  Nothing is updated.  SPFM_ERR_INVALID: no sampler set, not configured for psgd,
 * degree differs from spfm_configure, n_negatives / n_candidates / max_draws < 1, m >= 2^31, seed
 * or epoch < 0.  A handle with a communicator: SPFM_ERR_UNSUPPORTED. */
int spfm_psgd_pairs_sample(spfm_handle h, int degree, int64_t n_negatives, int64_t n_candidates,
                           int64_t max_draws, int64_t seed, int64_t epoch, const int32_t* order,
                           int32_t* triples_out, double* scores_out);
/* spfm_psgd_pairs_epoch over the list the last spfm_psgd_pairs_sample left on the device: no
 * upload, no per-epoch host check.  SPFM_ERR_INVALID when the resident list is not the output of a
 * sample call (a later spfm_psgd_pairs_epoch / _eval upload, or new data, invalidates it), and for
 * batch_size < 1, *it < 1, an unsupported learning_rate. */
int spfm_psgd_pairs_epoch_sampled(spfm_handle h, int degree, double alpha, double beta,
                                  double gamma, double eta0, int learning_rate, double power_t,
                                  int64_t batch_size, int fit_linear, int64_t* it,
                                  double* sum_loss);

/* Weighted triples, proposal distributions and the WARP sampler.
 *
 * spfm_psgd_pairs_epoch with one weight per triple: weights[q] >= 0 multiplies the loss and the
 * gradient of triple q (a triple of weight 0 is skipped); sum_loss is the sum of wt * loss; eta / B
 * still counts triples, not weight.  SPFM_ERR_INVALID, on the host before any launch (the
 * parameters stay as they were): a weight that is negative or not finite, and everything
 * spfm_psgd_pairs_epoch rejects.  A handle with a communicator: SPFM_ERR_UNSUPPORTED. */
int spfm_psgd_pairs_epoch_weighted(spfm_handle h, int degree, double alpha, double beta,
                                   double gamma, double eta0, int learning_rate, double power_t,
                                   int64_t batch_size, const int32_t* triples,
                                   const double* weights /* (m) */, int64_t m, int fit_linear,
                                   int64_t* it, double* sum_loss);
/* The proposal distribution of BOTH sample entries.  cum (n_cand): the inclusive cumulative sums of
 * non-negative integer weights -- non-decreasing, W = cum[n_cand - 1] in [1, 2^32).  With a table
 * the candidate of draw u is the smallest c with cum[c] > ((u >> 32) * W) >> 32 (integer only: a
 * binary search over cum); admission and the fallback walk are unchanged, so the walk may end on a
 * candidate of weight 0.  NULL restores the uniform draw.  Uploaded once, dropped with the sampler
 * (spfm_psgd_pairs_set_sampler, new data).  SPFM_ERR_INVALID: no sampler set, n_cand differs from
 * the sampler's, cum decreases, W == 0. */
int spfm_psgd_pairs_set_proposal(spfm_handle h, const uint32_t* cum, int64_t n_cand);
/* One weight per positive, in the canonical CSR order of the sampler's positives; NULL clears;
 * dropped with the sampler.  Once set, both sample entries write a weight per triple beside the
 * list (spfm_psgd_pairs_sample: the positive's weight; _sample_warp: times its rank weight) and
 * spfm_psgd_pairs_epoch_sampled reads it.  SPFM_ERR_INVALID: no sampler set, nnz differs from the
 * sampler's positives, a weight negative or not finite. */
int spfm_psgd_pairs_set_positive_weights(spfm_handle h, const double* wq, int64_t nnz);
/* WARP: the layout, draws, admission, score, `order` and resident-list bookkeeping of
 * spfm_psgd_pairs_sample.  For triple r of positive q = (b, c+): s+ = score(b, c+); the admitted
 * draws with t < max_draws are tried in the order of t, at most max_trials of them; the first
 * a_N with score(b, a_N) > s+ - margin (the violator) is the negative, trials = N and
 *   weight = posw_q * log(max(1, floor(A_b / N))),   A_b = n_cand - |forbidden(b)|
 * (posw_q = 1 without positive weights; under a proposal table A_b / N estimates the rank under
 * that proposal).  No violator among those tried: the highest-scored of them (ties to the earliest),
 * trials = 0, weight = 0.  No draw admitted: the fallback walk's candidate, trials = 0, weight = 0.
 * scores holds the negative's score.  weights_out (m) / trials_out (m): optional host copies, by
 * slot, like triples_out / scores_out.  The weights stay on the device for
 * spfm_psgd_pairs_epoch_sampled; spfm_psgd_lists_epoch_sampled after a sample call that wrote
 * weights is SPFM_ERR_INVALID.  SPFM_ERR_INVALID: max_trials < 1 or > max_draws, a margin that is
 * not finite, and everything spfm_psgd_pairs_sample rejects. */
int spfm_psgd_pairs_sample_warp(spfm_handle h, int degree, int64_t n_negatives,
                                int64_t max_trials, int64_t max_draws, double margin,
                                int64_t seed, int64_t epoch, const int32_t* order,
                                int32_t* triples_out, double* scores_out, double* weights_out,
                                int32_t* trials_out);

/* Listwise ranking fit: the training item is a LIST, a positive
 * (anchor, plus) with its n_negatives = M negatives.  `triples` (m, 3) is GROUPED: rows
 * q M .. q M + M - 1 share anchor and plus and hold the M negatives of list q -- the layout
 * spfm_psgd_pairs_sample writes with order == NULL.  With the scores
 *   s_i = sum_o sum_s lams_s a_s^{degree-o}(x_anchor + z_{c_i}) + <w, z_{c_i}>,  c_0 = plus,
 * (the anchor's linear term is the same for all of them and is left out) the loss of a list is
 *   SPFM_LIST_SOFTMAX   -s_0 + log sum_{i=0..M} exp(s_i)        (sampled softmax; a candidate
 *                                                                 that appears twice counts twice)
 *   SPFM_LIST_PAIRMEAN  (1/M) sum_{i>=1} loss(s_0 - s_i, +1)     (the configured loss; an epoch
 *       over B lists per batch is arithmetically spfm_psgd_pairs_epoch over the same triples
 *       with batch_size B M)
 * The context's share of the gradient is formed once per list whatever M is (one DP, one
 * gradient pass, one atomic per context column).  batch_size, eta / B and sum_loss count lists;
 * penalties, step sizes, prox, `it` and the psgd options are those of spfm_psgd_epoch.
 * SPFM_ERR_INVALID, checked on the host before anything is launched (the parameters stay as they
 * were): everything spfm_psgd_pairs_epoch rejects, m % n_negatives != 0, n_negatives outside
 * [1, SPFM_LIST_MAX_NEG], a group whose rows differ in anchor or plus, an unknown list_loss.  A
 * handle with a communicator: SPFM_ERR_UNSUPPORTED. */
#define SPFM_LIST_SOFTMAX 0
#define SPFM_LIST_PAIRMEAN 1
#define SPFM_LIST_MAX_NEG 63
int spfm_psgd_lists_epoch(spfm_handle h, int degree, double alpha, double beta, double gamma,
                          double eta0, int learning_rate, double power_t, int64_t batch_size,
                          const int32_t* triples /* (m,3), grouped by list */, int64_t m,
                          int64_t n_negatives, int list_loss, int fit_linear, int64_t* it,
                          double* sum_loss);
/* The same epoch over the list the last spfm_psgd_pairs_sample left on the device.  list_order:
 * NULL, or the visiting order of the Q = m / n_negatives lists (a permutation of 0..Q-1, checked
 * on the host, 4 Q bytes uploaded).  SPFM_ERR_INVALID: no resident sampled list, a sample call
 * that used a slot `order` or another n_negatives, list_order not a permutation, and the step
 * argument errors of spfm_psgd_lists_epoch. */
int spfm_psgd_lists_epoch_sampled(spfm_handle h, int degree, double alpha, double beta,
                                  double gamma, double eta0, int learning_rate, double power_t,
                                  int64_t batch_size, int64_t n_negatives, int list_loss,
                                  const int32_t* list_order /* Q or NULL */, int fit_linear,
                                  int64_t* it, double* sum_loss);
/* The same lists at the live device parameters, nothing updated: sum_loss = sum of the lists'
 * losses, n_first = number of lists with s_0 > max_{i>=1} s_i.  Same preconditions and argument
 * errors as spfm_psgd_lists_epoch. */
int spfm_psgd_lists_eval(spfm_handle h, int degree, int fit_linear, const int32_t* triples,
                         int64_t m, int64_t n_negatives, int list_loss, double* sum_loss,
                         int64_t* n_first);

/* -- multi-GPU (one process per GPU, RCCL over xGMI) ---------------------------
 * Rows are sharded; the column partial sums of every step are all-reduced
 * (sum, f64) so that every rank applies the identical prox.  id is an opaque
 * 128-byte RCCL unique id created on rank 0 and shipped by the caller. */
int spfm_comm_unique_id(char* id128);
int spfm_comm_init(spfm_handle h, const char* id128, int n_ranks, int rank);
/* The same sharded protocol with the all-reduce carried through a POSIX shared-memory
 * segment on the host (name as for shm_open, e.g. "/spfm_test_123"; created zero-filled by
 * whichever rank arrives first, the caller unlinks it).  For ranks that share ONE GPU, where
 * RCCL refuses to form a communicator: lets the multi-GPU code path (row shards, per-step
 * all-reduce, replicated chain) be run and checked on a single-GPU machine.  A test and
 * bring-up facility, orders of magnitude slower than RCCL over xGMI. */
int spfm_comm_init_shm(spfm_handle h, const char* shm_name, int n_ranks, int rank);

/* In-kernel cross-GPU exchange for the persistent passes (replaces the per-step collective;
 * SURVEY.md section 5 "one-hop direct-write exchange").  Every rank allocates one exchange
 * slab (spfm_peer_alloc returns its 64-byte hipIpc handle), the caller ships the handles to all
 * ranks (any channel: torch.distributed, MPI, a file) and every rank maps its peers' slabs
 * (spfm_peer_connect; handles = n_ranks x 64 bytes in rank order, n_ranks <= 8).  Requires a
 * communicator with the same ranks (spfm_comm_init / _shm): it carries the one-off set-up
 * reductions and the barrier between launches.  After connecting, set the schedule (again):
 * the persistent passes cap a step at 64 columns.  Works across the GPUs of one node (xGMI)
 * and -- for tests -- between processes that share one GPU. */
int spfm_peer_alloc(spfm_handle h, char* handle64);
/* Maps the peers' slabs and runs a handshake kernel: every rank stores one word into every
 * slab and polls its own until all ranks' words arrived (10 s bound) -- what the persistent
 * passes rely on (a system-scope store into a peer-mapped slab reaches a kernel that is already
 * polling).  All ranks call it together.  The slab is fine-grained device memory; when that
 * cannot be allocated, or the handshake fails, the call returns SPFM_ERR_RUNTIME and the caller
 * keeps the per-step collective (sparsepoly_amd.distributed.connect_peers does, on all ranks). */
int spfm_peer_connect(spfm_handle h, int n_ranks, int rank, const char* handles);

/* -- instrumentation ----------------------------------------------------------
 * Device time (ms, HIP events on the handle's stream) and launch count of the
 * dominant kernel family since the last reset: which = 0 pcd gather (persistent
 * engine: the whole-pass kernel pcd_prb_kernel; multi-kernel engine: pcd_grad_kernel),
 * 1 pcd chain+scatter (multi-kernel engine), 2 pbcd gradient, 3 pbcd sync,
 * 4 cd_linear (lin_prb_kernel or the per-step kernels).  nnz = column entries the
 * timed launches processed.  Timing is only collected when enabled (one event pair
 * per launch; the multi-kernel engine then launches eagerly instead of replaying). */
int spfm_profile_enable(spfm_handle h, int on);
int spfm_profile_get(spfm_handle h, int which, double* ms, int64_t* launches, int64_t* nnz);
int spfm_profile_reset(spfm_handle h);
/* use hipGraph replay for the per-pass launch sequences (default on) */
int spfm_set_use_graph(spfm_handle h, int on);

/* -- options ------------------------------------------------------------------
 * String-keyed integer options of a handle.  spfm_set_option returns SPFM_ERR_INVALID for an
 * unknown key, a read-out or a value outside the key's range; spfm_get_option reads every key
 * of the table except the action "interaction_release" (every settable key reads back the value
 * last set, or its default).  No option changes the coordinate order of a sweep, and none
 * changes an order the caller passed as 'exact'.
 *
 * Columns: key | values (default) | affects | when to set.  "affects" is one of
 *   nothing    nothing numerical: the same arithmetic in the same order
 *   sum order  how a sweep is cut into launches and the order in which partial sums are added
 *   schedule   also the coloured schedule built next (spfm_set_schedule(SPFM_SCHED_COLORED))
 *
 * Tuning
 *   "use_graph"               | 0/1 (1)        | nothing   | any time; hipGraph replay of the per-pass launch sequences
 *   "fuse_chain"              | 0/1 (1)        | sum order | any time; fused chain+sync kernel for steps of <= 64 columns
 *   "max_batch"               | >= 1 (4096)    | schedule  | before the schedule; columns per dependent step
 *   "persistent"              | 0/1 (1)        | sum order | before the schedule; one persistent launch per pcd component pass, caps steps at 64 columns
 *   "prb_groups"              | >= 1 (64)      | sum order | any time; workgroups of the 64-column persistent pass
 *   "prb_long"                | >= 16 (48)     | sum order | any time; entries of one column in one row block above which the whole workgroup, not 4 lanes, processes it
 *   "prb_lds"                 | 0/1 (1)        | sum order | any time; keep each workgroup's row block (A and the residual / prediction) in LDS for the whole pass when it fits: f32 storage, one cache value per row, squared loss or +-1 targets
 *   "prb_pack"                | 0/1 (1)        | sum order | any time; degree-3 passes with their rows in global memory work on packed 16-byte row records
 *   "relax"                   | 0/1 (1)        | sum order | any time; a schedule of tiny steps (the reference order, fewer than 12 columns per step on average) runs as merged steps of ~20 consecutive columns whose shared rows the chains replay in order: same result as the sequential sweep
 *   "pbcd_persistent"         | 0/1 (1)        | sum order | any time; the persistent pbcd pass
 *   "pbprb_groups"            | >= 1 (256)     | sum order | any time; workgroups of the persistent pbcd pass
 *   "pbprb_balance"           | 0/1 (1)        | sum order | any time; balanced slot groups of the persistent pbcd pass (0: slot q -> group q % groups)
 *   "pbprb_owners"            | 0 (0)          | nothing   | never; dedicated owner workgroups no longer exist, any other value returns SPFM_ERR_UNSUPPORTED
 *   "pbcd_fuse"               | 0/1 (1)        | sum order | any time; multi-kernel pbcd engine: prep and chain in one launch
 *   "wide"                    | 0/1 (1)        | schedule  | before the schedule; the wide passes for degree-2 pcd / cd_linear, steps of up to 512 columns
 *   "wide_min_cols"           | any int (110)  | schedule  | before the schedule; mean colour-class width below which the schedule is coloured again with 64 columns per class and the 64-column passes run; 0 = always wide
 *   "pcdw_groups"             | >= 1 (0 = auto) | sum order | any time; workgroups of the wide passes; auto = about 160 entries per workgroup and step, at most one per CU; reads back the count in use once the wide stream exists
 *   "wide_lds_rows"           | any int (-1 = auto) | sum order | any time; wide pass whose row block is too large for LDS: rows of it kept there
 *   "wide_ep"                 | 0/1 (1)        | sum order | any time; wide pass with rows in global memory: entry-parallel form
 *   "wide_rec8"               | 0/1 (1)        | sum order | any time; ... with 8-byte (A, residual) row records where they apply (squared loss, f32)
 *   "ingest_device"           | 0/1 (1)        | nothing   | before spfm_set_data_csr; transpose on the device (one stable radix sort of the entries by column id); 0, or no room for the sort's scratch: host threads
 *   "colour_device"           | 0/1 (1)        | nothing   | before the schedule; first-fit colouring on the device when the conflict structure is the handle's own matrix: the same order and batch boundaries as the host form
 *   "stream_device"           | 0/1 (1)        | nothing   | any time; entry streams of the persistent passes built on the device, entry for entry the host builder's
 *   "co_tenants"              | 1..64 (1)      | sum order | before the schedule; handles of this process whose persistent passes run at the same time on this device (see below)
 *   "peer_exchange"           | 0 (reads "peer_ready") | sum order | after spfm_peer_connect, then set the schedule again; gives the in-kernel cross-GPU exchange up for the per-step collective
 *   "persistent_failed"       | 0/1 (0)        | sum order | any time; 0 = try the persistent passes again after a recorded fall-back
 *   "psgd_eager"              | 0/1 (0)        | nothing   | any time; launch every psgd minibatch eagerly instead of replaying runs of 32 from a hipGraph
 *   "psgd_graph_sweeps"       | 0..64 (4)      | nothing   | any time; support-search sweeps recorded per minibatch for the squared-norm prox; an epoch in which that was not enough is redone eagerly from a snapshot ("psgd_redone")
 *   "interaction_tile_budget" | >= 0 (0 = default) | nothing | any time; tiles per launch of an interaction pass
 *   "interaction_features"    | >= 0 (0 = all) | nothing   | any time; the interaction passes see only features below this
 *   "interaction_release"     | action, value ignored, not readable | nothing | any time; frees the interaction passes' scratch
 *
 * Diagnostics (nothing numerical; set before the epochs they observe)
 *   "prb_stamps"              | 0/1 (0)        | nothing   | phase timers of the 64-column pass (spfm_debug_prb_stamps)
 *   "pcdw_stamps"             | 0/1 (0)        | nothing   | phase timers of the wide pass
 *   "pbprb_stamps"            | 0/1 (0)        | nothing   | phase timers of the persistent pbcd pass
 *   "pbprb_dbg"               | bit mask (0)   | nothing   | diagnostic counters of the persistent pbcd pass (bit 8: spfm_debug_prb_stamps returns them)
 *   "probe_xcd"               | any int (0)    | nothing   | spfm_debug_exchange_cost on one XCD
 *   "probe_lds"               | any int (61440) | nothing  | LDS bytes per workgroup of spfm_debug_exchange_cost
 *
 * Test hooks (not for production use)
 *   "debug_spin_max"          | >= 64 (2^21)   | nothing   | polls of one in-kernel wait before a persistent pass gives up
 *   "debug_drop_group"        | any int (0)    | nothing   | the next N persistent launches lack their last workgroup, i.e. time out
 *   "debug_keep_last_error"   | 0/1 (0)        | nothing   | spfm_comm_init does not clear the thread's stale HIP error before calling RCCL
 *   "debug_setup_any_size"    | 0/1 (0)        | nothing   | before the schedule; "colour_device" and "stream_device" apply whatever the problem's size (the thresholds of 2^20 entries and 4096 columns are skipped, every other guard stays), and the entry streams keep what spfm_debug_stream_tables reads
 *
 * Read-outs (spfm_get_option only)
 *   "persistent_active"       | 0/1            | -         | the next pcd epoch will use a persistent pass: option on, steps of <= 64 columns or the wide pass
 *   "wide_active"             | 0/1            | -         | the next pcd epoch will use the wide pass
 *   "pbprb_active"            | 0/1            | -         | what the last pbcd epoch used
 *   "prb_lds_active"          | 0/1/2          | -         | what the last pcd pass used: 0 global rows, 1 LDS residual form, 2 LDS prediction + label sign
 *   "prb_pack_active"         | 0/1            | -         | the last pcd pass used packed row records
 *   "wide_lds_active"         | 0/1/2          | -         | what the last wide pass used: 0 global rows, 1 all rows in LDS, 2 the first rows of a block in LDS
 *   "wide_ep_active"          | 0/1            | -         | the last wide pass used the entry-parallel form
 *   "relax_steps"             | >= 0           | -         | merged steps per sweep, 0 = strict steps
 *   "pb_relax_active"         | 0/1            | -         | the last pbcd epoch ran relaxed runs
 *   "persistent_fallbacks"    | >= 0           | -         | epochs redone on the multi-kernel engine (failure semantics below)
 *   "psgd_redone"             | >= 0           | -         | psgd epochs that fell back from graph replay to eager launches
 *   "n_ranks"                 | >= 1           | -         | ranks of the attached communicator
 *   "peer_ready"              | 0/1            | -         | in-kernel cross-GPU exchange connected and verified
 *   "ingest_device_used"      | 0/1            | -         | the last spfm_set_data_csr transposed on the device
 *   "colour_device_used"      | 0/1            | -         | the last coloured schedule was coloured on the device
 *   "stream_device_used"      | 0/1/2          | -         | 64-column entry stream: 0 host threads, 1 device, 2 taken from a co-tenant
 *   "pb_stream_device_used"   | 0/1            | -         | the pbcd entry stream was built on the device
 *   "wide_stream_device_used" | 0/1            | -         | the wide entry stream was built on the device
 *   "interaction_launches"    | >= 0           | -         | tile launches of the last interaction pass
 *   "interaction_scratch_kib" | >= 0           | -         | scratch the interaction passes hold, KiB
 *   "free_mem_mib"            | >= 0           | -         | free memory of the handle's device (hipMemGetInfo; SPFM_ERR_RUNTIME if that fails)
 *
 * co_tenants: independent fits, one handle and one host thread each; the handle then sizes its
 * passes to 1/co_tenants of the CUs (prb_groups and pbprb_groups are capped at once, the wide
 * pass caps itself) and its residency check to the shared device.  Handles are independent
 * objects: calls on DIFFERENT handles may be made from different threads at the same time, calls
 * on one handle must not overlap. */
int spfm_set_option(spfm_handle h, const char* key, int value);
int spfm_get_option(spfm_handle h, const char* key, int* value);

/* -- streams, hardware queues and failure semantics -----------------------------
 * The library never issues work on the null stream (every handle owns a non-blocking stream):
 * concurrent handles do not serialise on each other or on the host program's default stream.
 * The HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4); a host program
 * that wants more than three concurrent handles next to its own streams should raise it (the
 * Python package defaults it to 8).
 *
 * Failure semantics of the persistent passes (all-or-nothing epochs, as the reference's epoch
 * functions): if a pass cannot run to its end -- its workgroups are not all resident, a peer GPU
 * does not answer -- the epoch's parameters and regularizer state are restored from a snapshot
 * taken before the launches, y_pred is recomputed from them (arguments of the last
 * spfm_init_pred), the epoch is redone on the multi-kernel engine and the handle keeps using that
 * engine; with several ranks the decision is agreed on through the communicator.  The call
 * still returns SPFM_OK; spfm_get_option("persistent_fallbacks") counts the events. */

/* diagnostic ("prb_stamps" option): accumulated shader cycles per phase of the last
 * persistent pass, 16 values per workgroup (8 control-wave, 8 worker-wave phases);
 * returns the number of values written. */
int spfm_debug_prb_stamps(spfm_handle h, long long* out, int cap);
/* diagnostic: latency of one hand-off "agent-scope store by one workgroup becomes visible to
 * an agent-scope load of another" (the primitive of the persistent pass's exchange), measured
 * by ping-pong between workgroup 0 and workgroup `partner` of one launch (workgroups are
 * dealt round-robin to the 8 XCDs: partner 1 = other XCD, partner 8 = same XCD).
 * xcc_ids[2] receives the XCC_ID register of the two players. */
int spfm_debug_hop_latency(spfm_handle h, int partner, int rounds, double* ns_per_hop,
                           int* xcc_ids);
/* diagnostic: cost of the bare per-step exchange of the persistent pass -- `groups`
 * workgroups publish 64 granule pairs each and sweep all the others', `rounds` times, with
 * no other work (readers_mod > 1: only every readers_mod-th workgroup sweeps and passes its
 * totals on to the rest).  ncols = slots actually read. */
int spfm_debug_exchange_cost(spfm_handle h, int groups, int ncols, int readers_mod, int rounds,
                             double* ns_per_round);
/* diagnostic: the sums of one step's sweep, with an exact answer.  vals[groups][64][nv] (nv = 1:
 * lin_prb_kernel's granules, 2: pcd_prb_kernel's pairs) are uploaded as the tagged granules of step
 * `step` into a slab of the production layout; ONE workgroup then runs the persistent passes' own
 * sweep -- every wave its part, wave 0 the sum of the eight part sums -- and out[64][nv] receives
 * the totals (slots >= ncols: 0).  Nothing is published or waited for.  The contract it pins: a
 * value loses its two lowest mantissa bits, a part's workgroups are added in ascending order from
 * 0.0, then the parts in ascending order.  groups <= 256, ncols in [1, 64]. */
int spfm_debug_sweep_sums(spfm_handle h, int groups, int ncols, int nv, int step,
                          const double* vals, double* out);

/* Diagnostic for the counter calibration (profiles/r03_fetch_calibration.txt): one launch that
 * reads the persistent pass's entry stream (slot bounds, rows, values of every step, with the
 * pass's own access pattern) and nothing else; bytes_out receives the bytes it requested.  Run
 * under `rocprofv3 --pmc FETCH_SIZE` to see what the counter reports for that known quantity. */
int spfm_debug_stream_probe(spfm_handle h, int64_t* bytes_out);
/* Diagnostic (tools/write_calibration.py): one launch that stores ONE record of
 * bytes_per_record (4, 8 or 16) bytes per matrix entry at the entry's row -- the scatter pattern of
 * the persistent passes that keep their rows in global memory -- and writes nothing else;
 * *bytes_out = the bytes requested (nnz * bytes_per_record).  Calibrates WRITE_SIZE. */
int spfm_debug_write_probe(spfm_handle h, int bytes_per_record, int64_t* bytes_out);
/* diagnostic: how often the device chains took the reference's "numerical error" branches
 * since the last reset -- out[0] omegati.py:97-98 (clip), out[1] omegacs.py:90-96, out[2]
 * omegacs.py:75-76, out[3] squaredl21.py:48-49 (out[4..7] reserved).  reset != 0 clears the
 * counters after reading.  Counters are per process (all handles of the device). */
int spfm_debug_branch_counts(spfm_handle h, unsigned* out8, int reset);

/* -- the set-up tables: the entry streams of the persistent passes ------------------
 * What the passes run on is built once per schedule, by device kernels ("stream_device") or by
 * host threads; the two forms produce the same tables, entry for entry.  The two calls below
 * make the tables themselves comparable (tests/test_setup_tables_host.py,
 * tests/test_hip_setup_tables.py).  With G row blocks of rows_per = max(1, ceil(n_rows / G))
 * rows, nb steps and nnz entries:
 *   SPFM_STREAM_ROWBLOCK (the 64-column passes), _ROWBLOCK_RELAXED (their relaxed runs: the same
 *     form over the merged steps, without the entries that `skip` marks).  Entries sorted by
 *     (row block g, step b, slot q, row): sp[(g*nb + b)*65 + q] = first entry of slot q, src[e] =
 *     position of entry e in the CSC arrays, lmask[(g*nb + b)*2 + (q >> 5)] bit (q & 31) = the
 *     slot holds more than long_thresh entries.  sp: G*nb*65 + 1, lmask: G*nb*2.
 *   SPFM_STREAM_PBCD (the persistent pbcd pass).  Every (g, b) deals its slots to NG groups of at
 *     most 64 / NG: tab[(g*nb + b)*64 + grp*(64/NG) + t] = the slot group grp handles as its
 *     t-th, 0xFF = none.  balance = 0: slot q -> (q % NG, q / NG).  balance = 1: slots in
 *     descending order of their entries in the block, ties by slot, each to the group with the
 *     fewest entries so far that still has room, ties by group.  Slots exist below min(64,
 *     max(ncols(b), ncols(b+2))).  Entries sorted by (g, b, grp, t, row): sp[(g*nb + b)*(NG+1) +
 *     grp] = first entry of the group, flags[e] = t | 0x80 if step b-1 touched the entry's row (a
 *     skipped entry still marks its row as touched).  sp: G*nb*(NG+1) + 1, tab: G*max(nb,1)*64.
 *   SPFM_STREAM_WIDE (the wide passes).  Entries sorted by (g, b, q, row); wbase[b] = sum over the
 *     earlier steps of (ncols + 1), tot = d + nb: sp[g*tot + wbase[b] + q] = first entry of slot
 *     q, flags[e] = 1 if step b-1 touched the entry's row.  sp: G*tot + 1.
 * src and flags take nnz elements; the entry count (nnz less the skipped entries) is returned. */
#define SPFM_STREAM_ROWBLOCK 0
#define SPFM_STREAM_ROWBLOCK_RELAXED 1
#define SPFM_STREAM_PBCD 2
#define SPFM_STREAM_WIDE 3
/* Host-only form of the stream builders (no handle, no device), on a caller-given canonical CSC
 * structure (indptr[d+1], indices: ascending rows in [0, n_rows) inside each column), visiting
 * order and step boundaries batch_ptr[n_batches+1].  groups = G; long_thresh: row-block kinds;
 * NG (8, 16, 32 or 64) and balance: SPFM_STREAM_PBCD; skip[nnz] or NULL: not for
 * SPFM_STREAM_WIDE.  Steps of at most 64 columns except for SPFM_STREAM_WIDE.  Outputs are
 * caller-allocated with the sizes above; lmask / tab may be NULL for the kinds without them. */
int spfm_stream_build(int kind, int64_t n_rows, int32_t d, const int64_t* indptr,
                      const int32_t* indices, const int32_t* order, const int32_t* batch_ptr,
                      int32_t n_batches, int groups, int long_thresh, int NG, int balance,
                      const uint8_t* skip, int32_t* sp, int32_t* src, uint8_t* flags,
                      uint32_t* lmask, uint8_t* tab, int64_t* n_entries);
/* diagnostic: the shape of the stream of `kind` that the handle holds -- streams are built by the
 * first epoch that needs them -- info8 = {G, n_batches, NG, long_thresh, balance, entries, any
 * long slot, built on the device}; SPFM_ERR_INVALID if that stream has not been built. */
int spfm_debug_stream_info(spfm_handle h, int kind, int64_t* info8);
/* ... and its tables, copied out of device memory into caller-allocated arrays of the sizes
 * above (any pointer may be NULL).  skip[nnz] and batch_ptr_out[n_batches+1]: the entries left
 * out and the merged step boundaries of SPFM_STREAM_ROWBLOCK_RELAXED (batch_ptr_out: the
 * schedule's boundaries for the other kinds).  src, the wide stream's flags and skip are kept
 * only by a handle with "debug_setup_any_size" = 1: SPFM_ERR_INVALID otherwise. */
int spfm_debug_stream_tables(spfm_handle h, int kind, int32_t* sp, int32_t* src, uint8_t* flags,
                             uint32_t* lmask, uint8_t* tab, uint8_t* skip,
                             int32_t* batch_ptr_out);

/* -- Gram matrices (sparsepoly/kernels.py) -------------------------------------
 * The Gram matrices of kernels.py:51-137 and poly_predict (:140-153) on the device, for
 * sparsepoly_amd.kernels.  Any handle: no data, parameters or configuration are needed (only
 * its device and stream are used).
 *   kind SPFM_GRAM_ANOVA        anova_kernel (:71-115), K[i][j] = sum over i1 < ... < i_degree
 *                               of prod x_i p_i.  degree <= 1 gives X P^T (the else-branch with
 *                               an empty recursion, :98-115); degree > SPFM_GRAM_MAX_DEGREE ->
 *                               SPFM_ERR_UNSUPPORTED.
 *        SPFM_GRAM_POLY         homogeneous_kernel (:51-68) = polynomial_kernel(gamma=1,
 *                               coef0=0): (X P^T) ** degree, degree >= 0 (else UNSUPPORTED)
 *        SPFM_GRAM_ALL_SUBSETS  all_subsets_kernel (:117-137): prod_c (1 + x_c p_c); degree unused
 *   X is CSR: indptr[n1+1] (int64, indptr[0] = 0), indices (int32 column ids in [0,d), sorted and
 *   duplicate-free inside each row), data (double).
 *   lams   NULL: out receives K (n1 x n2, row-major).  Otherwise lams[n2] and out[n1] = K @ lams
 *          (poly_predict): reduced on the device in the pass that evaluates K, which is never
 *          stored whole.
 *   max_block_bytes  device memory of one block of the work (0 = library default, 4 GiB or half
 *          the free memory): X is processed in row blocks and the second operand in tiles of
 *          64-column chunks, each block of the result copied into `out` as it completes (at least
 *          one row and one 64-column tile per block, whatever the budget).  The result is
 *          bit-identical for every budget: one lane per output element, products in feature
 *          order, the K * lams sum of each 64-column chunk by a fixed tree, chunks in order.
 * Errors: bad shapes, index out of range, unsorted or duplicate indices -> SPFM_ERR_INVALID. */
#define SPFM_GRAM_ANOVA 0
#define SPFM_GRAM_POLY 1
#define SPFM_GRAM_ALL_SUBSETS 2
#define SPFM_GRAM_MAX_DEGREE 64

/* CSR X (n1 x d) against a dense B (n2 x d, row-major).  transpose_out = 1 writes K^T
 * (n2 x n1, row-major) instead: the dense-first call K(B, X) evaluated as K(X, B)^T in place
 * (not with lams: SPFM_ERR_INVALID). */
int spfm_gram_csr_dense(spfm_handle h, int kind, int degree, int64_t n1, int32_t d,
                        const int64_t* indptr, const int32_t* indices, const double* data,
                        int64_t n2, const double* B, const double* lams, int transpose_out,
                        int64_t max_block_bytes, double* out);
/* CSR X (n1 x d) against CSR P (n2 x d), both as above: every output element is a merge of two
 * sorted index lists (the rows of P staged in LDS per 64-row chunk when they fit). */
int spfm_gram_csr_csr(spfm_handle h, int kind, int degree, int64_t n1, int32_t d,
                      const int64_t* indptr1, const int32_t* indices1, const double* data1,
                      int64_t n2, const int64_t* indptr2, const int32_t* indices2,
                      const double* data2, const double* lams, int64_t max_block_bytes,
                      double* out);

/* -- objective, sparsity and held-out loss of the live parameters ----------------------------
 * What the reference's solvers minimise (sparse_factorization_machines.py:16-60 docstring):
 *   sum_i loss(y_pred_i, y_i) + alpha/2 |w|^2 + sum_o (beta/2 |P_o|^2 + gamma Omega(P_o)).
 * spfm_loss_sum gives the first term; spfm_objective_terms gives the ingredients of the others
 * from the LIVE device parameters -- the image spfm_get_params would return at that moment,
 * whichever engine ran last (persistent, wide, relaxed, multi-kernel, pbcd, psgd, after a
 * rolled-back persistent pass) -- without copying P to the host.
 *   order_idx >= 0: the block P[order_idx] (k x d);  order_idx == -1: w
 *   out8[0]  0.5 * sum p^2                        (w: 0.5 * sum w^2)
 *   out8[1]  Omega(P_o; degree) of the configured regularizer   (w: 0)
 *   out8[2]  number of non-zero entries           (w: non-zeros of w)
 *   out8[3]  active features: columns j with any P[o, s, j] != 0  (w: 0)
 *   out8[4]  active components: rows s with any non-zero          (w: 0)
 *   out8[5..7] reserved, written as 0
 * Omega is the quantity the device prox chains maintain, i.e. the reference's regularizer cache
 * after compute_cache_pcd / compute_cache_pbcd:
 *   l1 sum |p| (l1.py:17-18); l21 sum_j |P[:, j]|_2 (l21.py:19-21); squaredl12
 *   sum_s (sum_j |p_sj|)^2 (squaredl12.py:20-22, transpose=True); squaredl21 (sum_j |P[:, j]|_2)^2
 *   (squaredl21.py:23-25); omegati sum_s e_m(|P[s, :]|), m = degree in 1..6, degree = -1:
 *   sum_s prod_j (1 + |p_sj|) (omegati.py:19-47); omegacs e_m(n), n_j = |P[:, j]|_2, degree = -1:
 *   prod_j (1 + n_j) (omegacs.py:52-60, compute_cache_pbcd).
 * For five of the six this is the reference's eval().  DEVIATION, omegacs: the reference's
 * OmegaCS.eval (omegacs.py:22-39) RESHAPES its input to (k, d) instead of transposing it, so for a
 * non-square block it is not the function its own prox minimises; the value here follows the prox
 * cache (compute_cache_pbcd, then _cache[degree]).
 * Needs parameters and spfm_configure (the regularizer kind) -- and so, because spfm_configure
 * wants data, a data set; the data itself is not read.  Read-only: no
 * parameter, cache, y_pred, schedule or regularizer state changes, and a later epoch chooses
 * the same engine.  Deterministic: fixed-order f64 reductions (a tree over lanes, waves,
 * workgroups that depends on k and d only), the same bits on every call, for either parameter
 * layout and for every value of the *_groups / co_tenants options.  Several ranks: parameters are
 * replicated, the terms are local, nothing is communicated.
 * Errors: no parameters / no configuration / bad order_idx -> SPFM_ERR_INVALID; degree outside
 * 1..SPFM_MAX_DEGREE and -1 -> SPFM_ERR_UNSUPPORTED. */
int spfm_objective_terms(spfm_handle h, int order_idx, int degree, double* out8);

/* A second, held-out CSR matrix kept on the device next to the training data (what a callback
 * that scores validation data hands predict() every time, sparse_factorization_machines.py
 * :453-458): indptr[n+1] (int64, indptr[0] = 0), indices (int32 column ids in [0,d), sorted and
 * duplicate-free inside each row), data, stored in the handle's storage precision; y[n] or NULL.
 * d must equal the handle's n_features (data or parameters must be present).  Empty rows and
 * n = 0 are accepted.  Replaced by the next call, freed with the handle.
 * Errors: wrong d, index out of range, unsorted indices, nothing to take d from ->
 * SPFM_ERR_INVALID. */
int spfm_set_eval_csr(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                      const int32_t* indices, const double* data, const double* y);
/* _get_output (spfm_init_pred: same kernels, same arguments; degree = -1: all-subsets) on the
 * held-out matrix with the LIVE parameters, and *loss_sum = sum_i loss(y_pred_i, y_i) with the
 * configured loss (f64, fixed order).  Either output may be NULL; y_pred_out[n].  The matrix stays
 * resident and no parameter crosses the bus.  Read-only and deterministic as
 * spfm_objective_terms; with several ranks every rank evaluates the whole held-out set.
 * Errors: no parameters / no held-out set / loss_sum without targets or configuration ->
 * SPFM_ERR_INVALID; degree outside 1..SPFM_MAX_DEGREE and -1, or a degree the predict pass does not
 * have (1) -> SPFM_ERR_UNSUPPORTED. */
int spfm_eval_loss(spfm_handle h, int degree, int fit_linear, int add_lower_deg2,
                   double* loss_sum, double* y_pred_out);

/* -- selected feature interactions of the live parameters ------------------------------------
 * What the reference's example notebook inspects with np.dot(P.T, lams * P) != 0: which feature
 * pairs the fitted model kept.  For the block P_o = P[order_idx] (k x d),
 *   W = P_o^T diag(lams) P_o,   only j < j' counts (the diagonal is no part of the model);
 * W[j, j'] is the coefficient of x_j x_j' when P_o is the degree-2 block of a factorization
 * machine or the block of an all-subsets model.  W has d^2 entries and is NEVER formed: the
 * features with any non-zero entry (d_a of them) are compacted, the upper-triangular 64 x 64 tiles
 * of the d_a x d_a product are formed in registers (f64 matrix instructions) and consumed there.
 * Device scratch is O(d_a k + tiles / 4096 + K) -- it stays allocated between calls and is freed
 * by spfm_set_params, spfm_destroy or the option "interaction_release"; the cost is d_a^2 k flops
 * per pass.
 * All five entries need parameters only (no data, no spfm_configure), read the LIVE image --
 * whichever of the (k,d) / (d,k) layouts the last epoch left -- and are read-only as
 * spfm_objective_terms.  Arithmetic is f64 for either storage precision.  Feature ids are ids of
 * the block as stored.  Several ranks: parameters are replicated, every rank answers locally.
 *
 * Deterministic: every value of W is the same chain of operations in every entry, on every call
 * and for every tile budget; sums are reduced in a fixed tile order without float atomics.
 *
 * Options (spfm_set_option): "interaction_tile_budget" = tiles per launch (0 = default, 2^22; a
 * small value forces many launches and changes no result bit, like max_block_bytes above);
 * "interaction_features" = n > 0 restricts the stats / topk / list entries to the features
 * [0, n) (an augmented dummy column is left out this way); 0 = all.  "interaction_release" (any
 * value) frees the scratch.  spfm_get_option also gives
 * "interaction_launches" (tile launches of the last pass), "interaction_scratch_kib" (scratch the
 * entries hold) and "free_mem_mib" (hipMemGetInfo).
 *
 * spfm_interaction_stats: counts2 = {pairs with |W| > tol, active features d_a},
 *   sums3 = {sum W^2, sum |W|, max |W|} over j < j'.  tol >= 0; tol = 0 counts W != 0.
 * spfm_interaction_topk: the K pairs of largest |W| among W != 0, ordered by |W| descending, then
 *   j, then j' ascending; rows[K], cols[K] (j < j'), vals[K] (signed); *n_out = pairs written
 *   (< K when fewer exist).  Exact: a radix select over the f64 patterns of |W| (one product pass
 *   per 12 bits examined, usually two), then one pass that emits the candidates.  More than
 *   max(2^20, 2K) pairs tied with the K-th magnitude -> SPFM_ERR_UNSUPPORTED.
 * spfm_interaction_list: every pair with |W| > tol as (rows, cols, vals), sorted by (row, col);
 *   *n_out = their number.  If it exceeds `capacity` the call fails (SPFM_ERR_INVALID, the count
 *   is in *n_out and in the message) and writes nothing to rows / cols / vals.
 * spfm_interaction_values: vals[q] = W[rows[q], cols[q]] for L given pairs, in any order of the
 *   two ids; rows[q] == cols[q] gives 0.  Components are summed in order s = 0..k-1.
 * spfm_interaction_block: out (nJ x nJ2, row-major) = W[J, J2] for two id lists (repeats allowed),
 *   0 where J[a] == J2[b].  This one does store its result: above
 *   SPFM_INTERACTION_BLOCK_MAX_BYTES it is refused (SPFM_ERR_INVALID).
 * Errors: no parameters, bad order_idx, id out of range, negative tol / K / capacity ->
 * SPFM_ERR_INVALID. */
#define SPFM_INTERACTION_BLOCK_MAX_BYTES (1LL << 30)
int spfm_interaction_stats(spfm_handle h, int order_idx, double tol, int64_t* counts2,
                           double* sums3);
int spfm_interaction_topk(spfm_handle h, int order_idx, int64_t K, int32_t* rows, int32_t* cols,
                          double* vals, int64_t* n_out);
int spfm_interaction_list(spfm_handle h, int order_idx, double tol, int64_t capacity,
                          int32_t* rows, int32_t* cols, double* vals, int64_t* n_out);
int spfm_interaction_values(spfm_handle h, int order_idx, int64_t L, const int32_t* rows,
                            const int32_t* cols, double* vals);
int spfm_interaction_block(spfm_handle h, int order_idx, int64_t nJ, const int32_t* J,
                           int64_t nJ2, const int32_t* J2, double* out);

/* -- per-feature views of the pairwise weights -----------------------------------------------
 * For one feature, or for every feature: whom does it interact with, and how strongly?  Both
 * entries walk the FULL square of W (both triangles, 2 d_a^2 k flops) on the pair entries'
 * compaction and packed images: 64-row tiles of query features against strips of candidate
 * partners, W formed in registers and consumed there, nothing of size d_a^2 stored.  The scratch
 * is part of the pair entries' scratch (counted by "interaction_scratch_kib", freed by the same
 * three things): O(slab * d_a / 64) row records for the degrees, O(slab * (k + strips * K)) for
 * the partners.  "interaction_launches" reports the tile launches of the last pass.
 * Semantics are those of the pair entries word for word: parameters only (no data, no
 * spfm_configure), the LIVE image in either layout, read-only, f64 arithmetic for either storage
 * precision, ids of the block as stored, every rank answers locally.  The view is theirs too:
 * with "interaction_features" = n > 0 the features >= n are neither queries nor partners.
 *
 * Bits: every value of W seen or returned here is the tile chain's value, the bits that
 * spfm_interaction_topk / _list give; W[j, j'] and W[j', j] are the same bits (lams is +-1).
 *
 * spfm_interaction_degrees: for every feature j of the block, over all j' != j in view:
 *   degree[j] = number of j' with |W[j, j']| > tol (tol = 0 counts W != 0), sum_abs[j] =
 *   sum |W[j, j']|, max_abs[j] = the largest |W[j, j']|, strongest[j] = the smallest j' attaining
 *   it, -1 when max_abs[j] == 0.  Each array is [d]; any may be NULL.  A feature that is inactive
 *   or out of view gets 0, 0.0, 0.0, -1.  sum_abs is reduced without float atomics in an order
 *   that depends on d_a alone (per row: inside a 64-column tile, then the tiles); it is the same
 *   bits on every call and for every cand_strip (columns a workgroup walks; 0 = default, else a
 *   multiple of 64).
 * spfm_interaction_partners: for query q, feature J[q] (J == NULL: all features of the view in id
 *   order, nJ ignored; repeats allowed), the K partners j' in [cand_lo, cand_hi) and in view,
 *   j' != J[q], admissible under `by`, ordered by key descending, then j' ascending -- exact.
 *   cand_hi <= 0 = the end of the view.  ids / vals are [nJ][K] row-major, vals the SIGNED W;
 *   n_out[q] partners are written, the rest of the row is -1 / 0.0.  An inactive query gets
 *   n_out = 0.  row_slab = queries per slab, cand_strip = candidate columns per strip (0 =
 *   default, as in spfm_rank_set_partition; cand_strip a multiple of 64, at most 65536); no result
 *   bit depends on either.
 * Errors: no parameters, bad order_idx, id out of range, tol < 0, K < 1, an empty
 * [cand_lo, cand_hi), a bad `by`, cand_strip not a multiple of 64 -> SPFM_ERR_INVALID;
 * K > SPFM_INTERACTION_MAX_K -> SPFM_ERR_UNSUPPORTED (never an approximate answer).  With fewer
 * than 2 active features in view both succeed with the empty answers above. */
#define SPFM_PARTNERS_ABS 0   /* key |W|, among W != 0 */
#define SPFM_PARTNERS_POS 1   /* key  W,  among W > 0  */
#define SPFM_PARTNERS_NEG 2   /* key -W,  among W < 0  */
#define SPFM_INTERACTION_MAX_K 128
int spfm_interaction_degrees(spfm_handle h, int order_idx, double tol, int64_t cand_strip,
                             int64_t* degree, double* sum_abs, double* max_abs,
                             int32_t* strongest);
int spfm_interaction_partners(spfm_handle h, int order_idx, int64_t nJ, const int32_t* J,
                              int64_t K, int32_t cand_lo, int32_t cand_hi, int by,
                              int64_t row_slab, int64_t cand_strip, int32_t* ids, double* vals,
                              int32_t* n_out);

/* -- third-order interaction weights of the live parameters ----------------------------------
 * Which feature TRIPLES the fitted model kept.  For the block P_o = P[order_idx] (k x d),
 *   T[a, j, l] = sum_s lams_s p_sa p_sj p_sl,   only a < j < l counts;
 * T[a, j, l] is the coefficient of x_a x_j x_l when P_o is the degree-3 block of a factorization
 * machine or the block of an all-subsets model.  T has d^3 / 6 entries and is NEVER formed: the
 * pair entries' compaction and packed images are reused, and for every smallest member a (the
 * "pivot") the 64 x 64 tiles of T[a, :, :] -- the pair product with the second operand scaled by
 * p_.a -- are formed in registers (f64 matrix instructions) and consumed there.  A work unit is
 * (pair tile, block of 64 pivots).  Device scratch is that of the pair entries (the same
 * buffers, freed by the same three things): O(d_a k + min(units, 2^18) + units / 4096 + K), and
 * units / 4096 stays below the pair-tile count under the work guard below.  The cost is
 * d_a^3 k / 3 flops per pass.
 * Semantics are those of the pair entries word for word: parameters only (no data, no
 * spfm_configure), the LIVE image in either layout, read-only, f64 arithmetic for either storage
 * precision, ids of the block as stored, every rank answers locally.
 *
 * Deterministic: in every entry, on every call and for every launch partition and tile budget
 *   T[a, j, l] = sum_s A[j][s] * (B[l][s] * A[a][s]),  A = the packed block, B = diag(lams) A,
 * with the smallest id as the pivot, the product in brackets rounded on its own and the sum the
 * same chain of matrix-instruction steps over s = 0, 4, 8, ...; sums over triples are reduced in
 * a fixed unit order without float atomics.
 *
 * Options: the pair entries' keys, none of its own.  "interaction_tile_budget" counts units per
 * launch here (0 = default, 2^18), "interaction_launches" the unit launches of the last pass,
 * "interaction_features" restricts stats / topk / list to the features [0, n),
 * "interaction_scratch_kib" and "interaction_release" cover the shared scratch.
 *
 * Work guard: with more than SPFM_INTERACTION3_MAX_ACTIVE active features in view, stats / topk /
 * list return SPFM_ERR_UNSUPPORTED before any product pass; the message names d_a and points to
 * "interaction_features".  At the cap and k = 30 a pass is about 3.5e14 flops; at the 28 TFLOP/s
 * the PAIR pass measured that would be roughly 12 s.  That figure is an extrapolation: nobody
 * has measured a triple pass at the cap.
 *
 * spfm_interaction3_stats: counts2 = {triples with |T| > tol, active features d_a},
 *   sums3 = {sum T^2, sum |T|, max |T|} over a < j < l.  tol >= 0; tol = 0 counts T != 0.
 * spfm_interaction3_topk: the K triples of largest |T| among T != 0, ordered by |T| descending,
 *   then i, j, l ascending; i[K] < j[K] < l[K], vals[K] (signed); *n_out = triples written (< K
 *   when fewer exist).  Exact: the pair entries' radix select on the f64 patterns of |T|, then one
 *   pass that emits the candidates.  More than max(2^20, 2K) triples tied with the K-th magnitude
 *   -> SPFM_ERR_UNSUPPORTED.
 * spfm_interaction3_list: every triple with |T| > tol as (i, j, l, vals), sorted by (i, j, l);
 *   *n_out = their number.  If it exceeds `capacity` the call fails (SPFM_ERR_INVALID, the count
 *   is in *n_out and in the message) and writes nothing to i / j / l / vals.
 * spfm_interaction3_values: vals[q] = T[i[q], j[q], l[q]] for L given triples, the three ids in
 *   any order (sorted on the device; the smallest is the pivot); any two equal ids give 0.
 *   Components are summed in order s = 0..k-1.
 * Errors: no parameters, bad order_idx, id out of range, negative tol / K / capacity ->
 * SPFM_ERR_INVALID. */
#define SPFM_INTERACTION3_MAX_ACTIVE (1 << 15)
int spfm_interaction3_stats(spfm_handle h, int order_idx, double tol, int64_t* counts2,
                            double* sums3);
int spfm_interaction3_topk(spfm_handle h, int order_idx, int64_t K, int32_t* i, int32_t* j,
                           int32_t* l, double* vals, int64_t* n_out);
int spfm_interaction3_list(spfm_handle h, int order_idx, double tol, int64_t capacity, int32_t* i,
                           int32_t* j, int32_t* l, double* vals, int64_t* n_out);
int spfm_interaction3_values(spfm_handle h, int order_idx, int64_t L, const int32_t* i,
                             const int32_t* j, const int32_t* l, double* vals);

/* -- candidate ranking ------------------------------------------------------------------------
 * Given context rows X (n_ctx x d) and candidate rows Z (n_cand x d), both CSR over the handle's d
 * features: score[b, c] = _get_output(x_b + z_c), the value spfm_predict_csr gives for the summed
 * row with the same (degree, fit_linear, add_lower_deg2), and the K best candidates of every
 * context.  The columns with a stored entry in X and those with a stored entry in Z must be
 * DISJOINT (the field structure of a recommender: user / context fields against item fields).
 * Then the ANOVA kernel splits, a^m(x + z) = sum_t a^t(x) a^(m-t)(z), and so does the all-subsets
 * product:
 *   score[b, c] = rowconst[b] + colconst[c] + sum_r U[b, r] V[c, r],
 * R = k (degree - 1) columns (+ k with add_lower_deg2; k for degree = -1), rowconst / colconst the
 * model's output on x_b / z_c alone (0 for degree = -1).  Both towers cost one pass over their
 * own non-zeros; the product is formed in 64 x 64 tiles in registers (f64 matrix instructions)
 * and consumed there.  Nothing of size n_ctx * n_cand exists on the device: contexts go through in
 * slabs of rows, candidates in strips of tiles (spfm_rank_set_partition), and only
 * spfm_rank_scores stores its result (one slab at a time, at most 256 MiB).
 * Parameters only (spfm_set_params; no data, no spfm_configure), read-only as the interaction
 * entries, f64 arithmetic for either storage precision.  The candidate towers describe the
 * parameters at the time of spfm_rank_set_candidates; they and the scratch stay allocated until
 * spfm_set_params, spfm_destroy or spfm_rank_release (spfm_rank_info reads the size).
 *
 * Deterministic: a score is the same chain of matrix-instruction steps over r = 0, 4, 8, ...,
 * then + (rowconst + colconst), in both entries, on every call and for every slab height and
 * strip width; the selection uses integer counters only.
 *
 * spfm_rank_set_candidates: builds V and colconst from Z (n_cand >= 1; indptr[n_cand+1] int64
 *   starting at 0, indices int32 in [0,d), data).  degree 2..SPFM_MAX_DEGREE or -1 (all-subsets;
 *   fit_linear is ignored then); add_lower_deg2 needs P[1].
 * spfm_rank_scores: out (n_ctx x n_cand, row-major).  Above SPFM_RANK_SCORES_MAX_BYTES of output
 *   it is refused (SPFM_ERR_INVALID).  Every check precedes the first write to out.
 * spfm_rank_topk: per context row the *k_out = min(K, n_cand) largest scores, ordered by score
 *   descending, then candidate index ascending: idx_out / val_out (n_ctx x *k_out, row-major).
 *   Exact.  1 <= K <= SPFM_RANK_MAX_K, a larger K -> SPFM_ERR_UNSUPPORTED (never an approximate
 *   answer).  Scores are taken to be finite: a NaN or infinite score never ranks, and a slot that
 *   no finite score fills holds index -1 and NaN.  idx_out / val_out are written only once
 *   nothing can fail any more.
 * spfm_rank_set_partition: context rows per slab and candidates per strip of the following
 *   calls, each rounded up to 64; 0 = the library's default (4096 rows; a strip width chosen from
 *   the shape).  row_slab in [0, 2^20], cand_strip in [0, 65536].  No result bit depends on either:
 *   they exist so that a small problem can be made to run as many slabs and strips.
 * spfm_rank_info: out4 = {device scratch held in bytes (candidate towers included), device time
 *   in microseconds (HIP events) of the kernels of the last spfm_rank_scores / spfm_rank_topk call
 *   without its copies, row_slab, cand_strip as set}.
 * spfm_rank_release: frees the scratch and forgets the candidates.
 * These three are entries of their own, not keys of spfm_set_option.
 * Errors: no parameters / no candidates, indptr not starting at 0 or decreasing, column id out of
 * range, a column stored on both sides (checked with a d-byte flag pass; the message names the
 * column), K < 1 -> SPFM_ERR_INVALID. */
#define SPFM_RANK_MAX_K 128
#define SPFM_RANK_SCORES_MAX_BYTES (1LL << 30)
int spfm_rank_set_candidates(spfm_handle h, int degree, int fit_linear, int add_lower_deg2,
                             int64_t n_cand, const int64_t* indptr, const int32_t* indices,
                             const double* data);
int spfm_rank_scores(spfm_handle h, int64_t n_ctx, const int64_t* indptr, const int32_t* indices,
                     const double* data, double* out);
int spfm_rank_topk(spfm_handle h, int64_t n_ctx, const int64_t* indptr, const int32_t* indices,
                   const double* data, int64_t K, int32_t* idx_out, double* val_out,
                   int64_t* k_out);
int spfm_rank_set_partition(spfm_handle h, int64_t row_slab, int64_t cand_strip);
int spfm_rank_info(spfm_handle h, int64_t* out4);
int spfm_rank_release(spfm_handle h);

/* -- candidate ranking: lists left out, exact ranks of held-out candidates ------------------
 * Both entries take per-row lists of candidates as CSR patterns over the resident candidates:
 * ptr[n_ctx+1] int64 starting at 0 and not decreasing, ids int32 in [0, n_cand), strictly ascending
 * within a row (sorted, no duplicate).  E_b (eptr, eidx) are the candidates LEFT OUT for context
 * row b -- what the user already has --; eptr == NULL: nothing is left out.  T_b (tptr, tidx) are
 * the TARGETS of row b, the held-out candidates whose rank is asked for; a row may have none, at
 * most SPFM_RANK_MAX_TARGETS.  T_b and E_b must be disjoint.  score[b, c] below is the value
 * spfm_rank_scores writes for the pair, bit for bit, and beats((v, c), (s, t)) = v > s ||
 * (v == s && c < t) is the order of spfm_rank_topk.
 *
 * spfm_rank_topk_excl: spfm_rank_topk over the candidates outside E_b.  *k_out = min(K, n_cand) as
 *   before; a row with fewer admissible candidates ends in slots of index -1 and NaN.  With
 *   eptr == NULL it is spfm_rank_topk, bit for bit.
 * spfm_rank_eval: for every target, in the order of tidx,
 *     rank_out  = #{ c not in E_b, c != t : beats((score[b, c], c), (score[b, t], t)) }   (0-based;
 *                 the row's other targets count like any other candidate)
 *     score_out = score[b, t]
 *   and per row n_eff_out[b] = n_cand - |E_b|.  Any of the three may be NULL.  A candidate whose
 *   score is not finite never beats anything; a target whose own score is not finite gets rank -1.
 *   Exact: the target's score comes from the same chain of matrix-instruction steps as every other
 *   score, the counts are integers, and no result depends on the slab height or the strip width.
 *   Nothing of size n_ctx * n_cand is stored.
 * Slabs, strips, spfm_rank_info (device time of the last call's kernels; the scratch includes the
 * lists, scores and counts of the last call) and spfm_rank_release work as above.
 * Errors, all found before the first write to an output: a row with more than
 * SPFM_RANK_MAX_TARGETS targets -> SPFM_ERR_UNSUPPORTED (the message names the cap; a row is never
 * truncated); pointers not starting at 0 or decreasing, an id out of range, an unsorted list or a
 * duplicate, a target that is also left out, no candidates set, and the errors of spfm_rank_topk
 * -> SPFM_ERR_INVALID. */
#define SPFM_RANK_MAX_TARGETS 64
int spfm_rank_topk_excl(spfm_handle h, int64_t n_ctx, const int64_t* indptr, const int32_t* indices,
                        const double* data, const int64_t* eptr, const int32_t* eidx, int64_t K,
                        int32_t* idx_out, double* val_out, int64_t* k_out);
int spfm_rank_eval(spfm_handle h, int64_t n_ctx, const int64_t* indptr, const int32_t* indices,
                   const double* data, const int64_t* tptr, const int32_t* tidx,
                   const int64_t* eptr, const int32_t* eidx,
                   int32_t* rank_out, double* score_out, int32_t* n_eff_out);

/* -- per-row feature attributions -------------------------------------------------------------
 * Why a row got its prediction.  The model is a sum of blocks, block q being
 *   sum_s lams_s sum_{t=0..6} coef[q][s][t] A^t(p_s, x),   p_s = P[order_idx[q]][s],
 * A^t the ANOVA kernel of order t, plus w.x when fit_linear.  A plain block of degree M has
 * coef[s][M] = 1 and zeros elsewhere; the table lets a caller fold columns that are constant in
 * every row (the dummy columns of fit_lower='augment') into lower orders instead of storing
 * them.  Only t = 1..degree[q] is read: column 0 is a constant of the model and belongs to the
 * caller's base value.
 * Every monomial of A^t is a product over t entries of the row.  Against the baseline x = 0 its
 * Shapley value splits it equally among those entries, so for the stored entry (i, j)
 *   phi_ij   = w_j x_ij + x_ij sum_q sum_s lams_s p_sj sum_t (coef[q][s][t] / t) g_{t-1}
 *   df/dx_ij = w_j      +      sum_q sum_s lams_s p_sj sum_t  coef[q][s][t]      g_{t-1}
 * with g_0 = 1, g_t = A^t(p_s, x_i) - p_sj x_ij g_{t-1}, which is A^t of the row without entry j.
 * Exact, not sampled; sum_j phi_ij = f(x_i) - f(0).  The gradient is that of a stored entry with
 * the sparsity pattern held fixed.  The input is CSR over the handle's d features (indptr[n+1]
 * int64 starting at 0, indices int32 in [0,d), data); a column stored twice in a row is treated
 * as two features with the same parameters, so canonical input is the caller's business.
 * Parameters only (spfm_set_params; no data, no spfm_configure), read-only as spfm_predict_csr,
 * values read in the handle's precision, all arithmetic in f64.  Rows go through in slabs bounded
 * by a count of stored entries; the scratch holds one slab (at most 256 MiB unless a single row
 * is larger) and stays allocated until spfm_set_params or spfm_destroy.
 *
 * Deterministic: an entry's value is the linear term, then the blocks in the caller's order,
 * each a sum over the components in index order formed by one lane; a row sum adds lane l's
 * entries l, l + 64, ... in order and then the lanes by a fixed butterfly; the selection compares
 * integers.  No result bit depends on the slab size or the launch shape.
 *
 * spfm_explain_csr: mode SPFM_EXPLAIN_ATTRIBUTION or SPFM_EXPLAIN_GRADIENT; out_vals (nnz, in
 *   the order of data; slab by slab, so after an error its contents are unspecified) and
 *   out_rowsum (n; NULL: not computed), out_rowsum[i] = sum_j out_vals[i, j].
 * spfm_explain_topk_csr: the attributions of every row largest by magnitude: per row its
 *   min(K, n_i) entries ordered by |phi| descending, then column ascending (then position), in
 *   idx / val (n x K, row-major; val holds phi with its sign); the remaining slots hold column -1
 *   and value 0.  Exact.  1 <= K <= SPFM_EXPLAIN_MAX_K, a larger K -> SPFM_ERR_UNSUPPORTED (never
 *   an approximate answer).  The values stay on the device; only n x K come back.
 * spfm_explain_set_partition: stored entries per slab of the following calls, in [0, 2^23];
 *   0 = the default, 2^23.  A slab always holds at least one whole row.  No result bit depends
 *   on it: it exists so that a small problem can be made to run as many slabs.
 * spfm_explain_info: out4 = {device scratch held in bytes, device time in microseconds (HIP
 *   events) of the kernels of the last spfm_explain_* call without its copies, slab_nnz as set,
 *   slabs of the last call}.
 * The last two are entries of their own, not keys of spfm_set_option.
 * Errors: no parameters, order_idx outside the parameters, indptr not starting at 0 or
 * decreasing, column id out of range, K < 1 -> SPFM_ERR_INVALID; degree outside
 * 2..SPFM_MAX_DEGREE, K above the cap -> SPFM_ERR_UNSUPPORTED.  Every check precedes the first
 * write to an output; n = 0 is valid and writes nothing. */
#define SPFM_EXPLAIN_MAX_K 64
#define SPFM_EXPLAIN_ATTRIBUTION 0
#define SPFM_EXPLAIN_GRADIENT 1
int spfm_explain_csr(spfm_handle h, int64_t n, const int64_t* indptr, const int32_t* indices,
                     const double* data, int n_blocks, const int32_t* order_idx,
                     const int32_t* degree, const double* coef /* n_blocks x k x 7 */,
                     int fit_linear, int mode, double* out_vals, double* out_rowsum);
int spfm_explain_topk_csr(spfm_handle h, int64_t n, const int64_t* indptr, const int32_t* indices,
                          const double* data, int n_blocks, const int32_t* order_idx,
                          const int32_t* degree, const double* coef /* n_blocks x k x 7 */,
                          int fit_linear, int K, int32_t* idx, double* val);
int spfm_explain_set_partition(spfm_handle h, int64_t slab_nnz);
int spfm_explain_info(spfm_handle h, int64_t* out4);

/* -- per-row pair attributions ----------------------------------------------------------------
 * Which pairs of a row's features produced its score.  The model, the blocks, the coefficient
 * table and the CSR input are those of the block above.  Against the baseline x = 0 a monomial of
 * one entry stays with that entry (its main effect), a monomial of t >= 2 entries is split
 * equally among its t (t - 1) / 2 pairs: the Shapley-Taylor interaction index of order 2.  With
 * z_sj = p_sj x_ij, the stored entries a < b (positions in the row) of row i get
 *   main_ia = w_a x_ia + sum_q sum_s lams_s coef[q][s][1] z_sa
 *   phi_iab = sum_q sum_s lams_s z_sa z_sb sum_{t=2..M} coef[q][s][t] 2 / (t (t - 1)) h_{t-2}
 * with g_0 = h_0 = 1, g_t = A^t(p_s, x_i) - z_sa g_{t-1}, h_t = g_t - z_sb h_{t-1}: h_t is A^t of
 * the row without the entries a and b.  Exact, not sampled:
 *   sum_a main_ia + sum_{a<b} phi_iab = f(x_i) - f(0),
 *   phi_ia of spfm_explain_csr = main_ia + 1/2 sum_{b != a} phi_iab,
 * and for a plain block of degree 2 phi_iab = x_ia x_ib W[a][b].  Mode SPFM_PAIRS_HESSIAN gives
 *   d2f / dx_ia dx_ib = sum_q sum_s lams_s p_sa p_sb sum_{t=2..M} coef[q][s][t] h_{t-2}
 * on the stored pairs, the pattern held fixed.
 * The pairs of a row of n_i entries are numbered by (first position, second position): the pair
 * of positions a < b is pair a n_i - a (a + 1) / 2 + b - a - 1 of its n_i (n_i - 1) / 2, and the
 * rows follow one another.  Read-only and sliced like the block above: a slab holds at most
 * slab_nnz stored entries (spfm_explain_set_partition) and at most 2 slab_nnz pairs (2^24 at the
 * default), always at least one whole row; the pair values of one slab are device scratch, held
 * and freed with the explain scratch.  spfm_explain_info reports these calls like the others.
 *
 * Deterministic: a pair's value is the sum over the blocks in the caller's order, each a sum over
 * the components in index order formed by one lane; a table cell adds its pairs in ascending pair
 * index in one lane; the selection compares integers.  No result bit depends on the slab size or
 * the launch shape.
 *
 * spfm_explain_pairs_csr: mode SPFM_PAIRS_INTERACTION or SPFM_PAIRS_HESSIAN; out_pairs
 *   (sum_i n_i (n_i - 1) / 2, in the order above; slab by slab, so after an error its contents
 *   are unspecified) and out_main (nnz, in the order of data; NULL: not computed; interaction
 *   mode only).  More than SPFM_PAIRS_MAX_BYTES of pair values -> SPFM_ERR_UNSUPPORTED.
 * spfm_explain_pairs_topk_csr: per row its min(K, pairs) pairs ordered by |value| descending,
 *   then pair index ascending, in col_a / col_b / val (n x K, row-major; the two members' columns,
 *   col_a the one stored first; val with its sign); the remaining slots hold -1, -1 and 0.
 *   Exact.  1 <= K <= SPFM_PAIRS_MAX_K.  The pair values stay on the device.
 * spfm_explain_pairs_grouped_csr: group (d ids in [0, G)) puts every column into a group.
 *   out_pairs (n x G (G + 1) / 2, row-major): per row the upper triangle of a G x G table, cell
 *   (g, h), g <= h, at g G - g (g - 1) / 2 + h - g, the sum of phi over the pairs with one member
 *   in g and the other in h (the diagonal: both in g); out_main (n x G): main summed per group.
 *   Interaction mode.  1 <= G <= SPFM_PAIRS_MAX_GROUPS.
 * Errors: those of the block above; a mode other than the two, a group id outside [0, G), K < 1,
 * G < 1, out_main with SPFM_PAIRS_HESSIAN -> SPFM_ERR_INVALID; K or G above its cap, a listing
 * above SPFM_PAIRS_MAX_BYTES, a row of more than 65536 stored entries (its pair index would not
 * fit the selection key) -> SPFM_ERR_UNSUPPORTED, never an approximate answer.  Every check
 * precedes the first write to an output; n = 0 is valid and writes nothing. */
#define SPFM_PAIRS_MAX_K 64
#define SPFM_PAIRS_MAX_GROUPS 32
#define SPFM_PAIRS_MAX_BYTES (1ll << 30) /* of listed pair values per call */
#define SPFM_PAIRS_INTERACTION 0
#define SPFM_PAIRS_HESSIAN 1
int spfm_explain_pairs_csr(spfm_handle h, int64_t n, const int64_t* indptr, const int32_t* indices,
                           const double* data, int n_blocks, const int32_t* order_idx,
                           const int32_t* degree, const double* coef /* n_blocks x k x 7 */,
                           int fit_linear, int mode, double* out_pairs, double* out_main);
int spfm_explain_pairs_topk_csr(spfm_handle h, int64_t n, const int64_t* indptr,
                                const int32_t* indices, const double* data, int n_blocks,
                                const int32_t* order_idx, const int32_t* degree,
                                const double* coef /* n_blocks x k x 7 */, int fit_linear,
                                int mode, int K, int32_t* col_a, int32_t* col_b, double* val);
int spfm_explain_pairs_grouped_csr(spfm_handle h, int64_t n, const int64_t* indptr,
                                   const int32_t* indices, const double* data, int n_blocks,
                                   const int32_t* order_idx, const int32_t* degree,
                                   const double* coef /* n_blocks x k x 7 */, int fit_linear,
                                   int G, const int32_t* group, double* out_pairs,
                                   double* out_main);

/* ---- model banks: F fitted models scored in one pass over the rows of X.
 * A bank is F models of one kind -- all of degree 2..SPFM_MAX_DEGREE or all all-subsets (-1),
 * the same blocks, the same use of a linear term, the same d columns -- that may differ in their
 * component counts k_f.  Their parameters are stacked along the component axis, feature-major:
 *   koff (F + 1): 0 = koff[0] < koff[1] < ... ; model f owns the stacked components
 *                 koff[f] .. koff[f+1] - 1, S = koff[F]
 *   Pt_bank (n_blocks x d x S): block q's P of every model, transposed and side by side
 *   lams_bank (S), w_bank (d x F; NULL = the models have no linear term)
 *   degree (n_blocks): the blocks in _get_output's order: {M} or {3, 2}; {-1} = all-subsets
 * spfm_bank_set copies the image to the device, where it stays until spfm_bank_release, the next
 * spfm_bank_set or spfm_destroy; it needs neither data nor spfm_set_params and changes neither.
 * The four passes take a CSR matrix over the bank's d columns (indptr[n+1] int64 starting at 0,
 * indices int32 in [0,d), data; values read in the handle's precision, all arithmetic in f64; a
 * column stored twice in a row is two features, canonical input is the caller's business) and
 * run it through in slabs bounded by a count of stored entries:
 * spfm_bank_scores: out (n x F) row-major, out[i][f] = what spfm_predict_csr gives for model f.
 * spfm_bank_argmax: per row the index of the largest score (ties: the lowest index), that score
 *   and the second largest (-inf when F = 1): idx, best, runner (n each).  No score leaves the device.
 * spfm_bank_losses: out[f] = sum_i loss(score_if, y_i) (per_model = 0, y (n)) or
 *   sum_i loss(score_if, y[i][f]) (per_model = 1, y (n x F) row-major); loss one of SPFM_LOSS_*.
 *   F doubles leave the device.
 * spfm_bank_mean: out[i] = sum_f weights[f] score_if, added in model order; weights NULL = 1/F.
 * Deterministic: model f's score is (B_0 + lin) + B_1, every B_q the sum of f's own component
 * terms one after the other in f's component order, lin the sum over the row's entries in stored
 * order.  No bit of it depends on the other members, on f's position, on the slab size or the
 * launch shape.  A loss sum adds the 256 rows of a block by a fixed tree and the blocks in a
 * fixed order: the same from run to run for one slab size.
 * spfm_bank_set_partition: stored entries per slab of the following calls, in [0, 2^23]; 0 = the
 *   default, 2^23.  A slab always holds at least one whole row.
 * spfm_bank_info: out4 = {slabs of the last pass, launches of bank_predict_kernel in it, bytes of
 *   the resident image, S}.
 * Errors: NULL arrays (with n > 0 for the outputs), F < 1, koff not starting at 0 or not
 * increasing, n_blocks outside 1..2, d < 1, a matrix whose d differs from the bank's, indptr not
 * starting at 0 or decreasing, column id out of range, an unknown loss, no bank set
 * -> SPFM_ERR_INVALID; F above SPFM_BANK_MAX_MODELS, S above SPFM_BANK_MAX_COMPONENTS (the
 * message names the cap; never answered approximately, never split), a degree outside
 * 2..SPFM_MAX_DEGREE and -1 -> SPFM_ERR_UNSUPPORTED.  Every check precedes the first write to an
 * output; n = 0 is valid (the loss sums are 0). */
#define SPFM_BANK_MAX_MODELS 64
#define SPFM_BANK_MAX_COMPONENTS 4096
int spfm_bank_set(spfm_handle h, int32_t d, int F, const int32_t* koff, int n_blocks,
                  const int32_t* degree, const double* Pt_bank, const double* lams_bank,
                  const double* w_bank);
int spfm_bank_scores(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                     const int32_t* indices, const double* data, double* out);
int spfm_bank_argmax(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                     const int32_t* indices, const double* data, int32_t* idx, double* best,
                     double* runner);
int spfm_bank_losses(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                     const int32_t* indices, const double* data, int loss, const double* y,
                     int per_model, double* out);
int spfm_bank_mean(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                   const int32_t* indices, const double* data, const double* weights,
                   double* out);
/* spfm_bank_group_sums: grouped, weighted per-member sums behind the same scoring pass (DESIGN.md
 * section 21) -- what cross-validation needs from F fitted clones: every member's metric on the
 * rows of every fold, in one pass over X.
 *   out[q][f][g] = sum over rows i with group[i] == g of weight[i] * metric_q(score_if, y_if)
 * out is (Q x F x G) row-major; y_if = y[i] (per_model = 0) or y[i * F + f] (per_model = 1);
 * weight (n) or NULL = 1.0; group (n) ids in [0, G) or NULL = all 0; metrics (Q) distinct ids: one
 * of SPFM_LOSS_* (that loss of (score, y)), SPFM_METRIC_ABS_ERROR (|score - y|) or
 * SPFM_METRIC_SIGN_ERROR (1.0 where (score > 0) != (y > 0), else 0.0: a score of 0 is the negative
 * class).  The term is weight[i] * value in this bracketing, so a weight of 1.0 changes no bit of
 * it and weight = NULL equals a vector of ones.  A group without rows gives exact zeros; n = 0 is
 * valid and gives all zeros.
 * Deterministic, no float atomics: the rows go in blocks of 256 (a slab starts a new block), wave
 * w of a block adds its 64 rows' terms one after the other in row order, the four waves are added
 * in wave order, the blocks of the call in block order.  Column f depends neither on the other
 * members nor on f's position nor on F; the sums are the same from run to run for one slab size
 * (spfm_bank_set_partition).  spfm_bank_losses keeps its own kernels and its own order.
 * Errors, each before the first write to out: NULL y (with n > 0), out or metrics, G < 1, Q < 1,
 * an unknown metric id or the same id twice, a group id outside [0, G), a negative or non-finite
 * weight and everything the other passes refuse -> SPFM_ERR_INVALID; G above SPFM_BANK_MAX_GROUPS
 * or Q above SPFM_BANK_MAX_METRICS -> SPFM_ERR_UNSUPPORTED (the message names the cap; the request
 * is never split or truncated).  The caps bound the LDS table of a workgroup, 4 waves x G x F
 * doubles with the metrics taken one after the other: 64 KB at G = 32, F = 64. */
#define SPFM_BANK_MAX_GROUPS 32
#define SPFM_BANK_MAX_METRICS 4
#define SPFM_METRIC_ABS_ERROR 16
#define SPFM_METRIC_SIGN_ERROR 17
int spfm_bank_group_sums(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                         const int32_t* indices, const double* data, const double* y,
                         int per_model, const double* weight /* n, or NULL = 1.0 */,
                         const int32_t* group /* n ids in [0, G), or NULL = all 0 */, int G, int Q,
                         const int32_t* metrics, double* out /* Q x F x G, row-major */);
/* spfm_bank_group_auc: the exact ROC-AUC of every member on sets of rows, behind the same scoring
 * pass.  Row i belongs to set u of member f when bit group[i] of
 * sets[f * U + u] is set (group NULL: every row is in group 0); sets NULL: U = G and set u = {u}
 * for every member.  A row is positive for member f when y_if > 0 (y as for spfm_bank_group_sums).
 * Over the rows of a set, P its positives, N its negatives, s the member's scores:
 *   weight == NULL (integers only): pairs[f][u] = {U2, n_pos, n_neg} with
 *     U2 = 2 #{(p, q): s_q < s_p} + #{(p, q): s_q == s_p},
 *     out[f][u] = {(double)U2 / (2.0 * (double)n_pos * (double)n_neg), n_pos, n_neg};
 *   weighted: out[f][u] = {sum_p w_p (sum_{q: s_q < s_p} w_q + 1/2 sum_{q: s_q == s_p} w_q)
 *     / (W_pos W_neg), W_pos, W_neg}; pairs is not written.
 * -0.0 and +0.0 are equal scores; the scores are taken to be finite.  A set that lacks a class
 * (the product of the two counts or weights is 0) has auc = NaN, the counts and weights are
 * reported all the same; an empty set gives NaN and zeros; n = 0 is valid.
 * The scores of a slab become order-preserving 64-bit keys in a member-major image that lives
 * until the call returns; after the last slab every member's keys are sorted (stable radix sort,
 * the row number as payload: equal scores sit in row order) and walked in blocks of
 * SPFM_BANK_RANK_BLOCK sorted positions (spfm_bank_rank.hip.h: no atomics, every addend
 * non-negative, the order of the additions a function of the sorted position alone).  The integers
 * depend on nothing but the scores; the weighted values have the same bits from run to run, for
 * every slab size (spfm_bank_set_partition), every F and every position of the member.
 * Errors, each before the first write to out and before any device work: everything
 * spfm_bank_group_sums refuses for y, weight, group, G and the matrix; U < 1, NULL out, a set bit
 * at or above G -> SPFM_ERR_INVALID; G above SPFM_BANK_MAX_GROUPS, U above SPFM_BANK_MAX_SETS, or
 * a scratch (8 n F bytes of keys, n F of class and group, 4 n of row numbers, 8 n of weights where
 * given, and with Fb = min(F, max(1, 128 MiB / 12 n)) the members of a sort batch and nb = ceil(n /
 * SPFM_BANK_RANK_BLOCK): 12 n Fb of sorted pairs, 40 nb U Fb of the walk's block records, and the
 * sort's own storage) above SPFM_BANK_AUC_MAX_BYTES -> SPFM_ERR_UNSUPPORTED (the message names the
 * cap or the bytes; the request is never split or truncated).  The scratch is freed before the
 * call returns, whatever it returns.  Test hook: the environment variable SPFM_BANK_AUC_BATCH = m
 * >= 1, read at every call, makes Fb = min(Fb, m); no result bit depends on it. */
#define SPFM_BANK_MAX_SETS 32
#define SPFM_BANK_RANK_BLOCK 256
#define SPFM_BANK_AUC_MAX_BYTES (1ll << 30)
int spfm_bank_group_auc(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                        const int32_t* indices, const double* data, const double* y,
                        int per_model, const double* weight /* n, or NULL: integer path */,
                        const int32_t* group /* n ids in [0, G), or NULL = all 0 */, int G,
                        const uint32_t* sets /* F x U bitmasks over groups, or NULL */, int U,
                        double* out /* F x U x 3: auc, pos_weight, neg_weight */,
                        int64_t* pairs /* F x U x 3 or NULL; only when weight == NULL */);
/* spfm_bank_group_curve: average precision, the best F1 and the KS distance of every member on sets
 * of rows, with the thresholds of the two maxima, behind the scoring pass, the key images and the
 * sorts of spfm_bank_group_auc.  Rows, sets, groups, positives (y_if > 0),
 * weights and -0.0 == +0.0 are exactly as there.  For one member and one set, w_p the weight of a
 * row of the set (1 unweighted) and 0 of any other row, go through the member's tie runs from the
 * highest score down; for run r
 *   Prun(r), Nrun(r) = the positive / negative weight of the run,
 *   TP(r), FP(r)     = the positive / negative weight of all runs down to and including r,
 * and r is a candidate when Prun(r) + Nrun(r) > 0 (it holds a row of the set of non-zero weight: a
 * row of weight 0 is the same as an absent row).  Then
 *   average_precision = (1 / W_pos) sum over the candidates of Prun(r) * (TP(r) / (TP(r) + FP(r))),
 *   best_f1           = max over the candidates of 2 TP(r) / ((TP(r) + FP(r)) + W_pos),
 *   ks                = max over the candidates of |TP(r) / W_pos - FP(r) / W_neg|.
 * Of several candidates that reach a maximum the one with the highest score wins.  Each maximum
 * reports its threshold -- the run's score, the zero run as +0.0: predict positive where
 * decision_function >= threshold -- and its TP and FP.
 *   out[f][u]    = {ap, f1, f1_thr, f1_tp, f1_fp, ks, ks_thr, ks_tp, ks_fp, W_pos, W_neg};
 *   counts[f][u] = {n_pos, n_neg, f1_tp, f1_fp, ks_tp, ks_fp}, written only for weight == NULL.
 * weight == NULL (integers only): the two maxima are chosen by exact integer comparison (F1 by
 * cross-multiplication in unsigned 64 bit, KS by |TP n_neg - FP n_pos|), then
 *   f1 = (double)(2 TP) / (double)(TP + FP + n_pos),
 *   ks = (double)|TP n_neg - FP n_pos| / ((double)n_pos * (double)n_neg):
 * counts, thresholds, f1 and ks depend on nothing but the scores and labels.  Weighted, the doubles
 * above are compared as written; the winning ks is then reported in the integer form,
 * |TP W_neg - FP W_pos| / (W_pos W_neg) in doubles, so that integer weights give the bits that
 * replicated rows give.  The terms of ap, Prun * (TP / (TP + FP)) in double, are added in
 * blocks of SPFM_BANK_RANK_BLOCK sorted positions from the top, the blocks in order
 * (spfm_bank_curve.hip.h: no atomics, every addend non-negative): every value has the same bits
 * from run to run, for every slab size, every F, every position of the member and every batch.
 * ap and f1 need W_pos > 0 (with W_neg == 0 they are 1.0 by the formulas), ks needs both class
 * weights; what is undefined is NaN, its threshold NaN and its TP / FP 0; the weights are reported
 * all the same.  An empty set gives NaN and zeros; n = 0 is valid.
 * auc_out (F x U x 3) and auc_pairs (F x U x 3, weight == NULL only), where given, receive what
 * spfm_bank_group_auc gives for the same arguments, bit for bit, from the same sorted copies: one
 * scoring pass and one sort per member for both tables.
 * Errors: those of spfm_bank_group_auc, each before the first write to an output and before any
 * device work; NULL out -> SPFM_ERR_INVALID.  The scratch is that call's plus 96 nb U Fb bytes of
 * this walk's block records, inside the same SPFM_BANK_AUC_MAX_BYTES; SPFM_BANK_AUC_BATCH applies
 * unchanged. */
#define SPFM_BANK_CURVE_VALUES 11  /* ap, f1, f1_thr, f1_tp, f1_fp, ks, ks_thr, ks_tp, ks_fp, W_pos, W_neg */
#define SPFM_BANK_CURVE_COUNTS 6   /* n_pos, n_neg, f1_tp, f1_fp, ks_tp, ks_fp */
int spfm_bank_group_curve(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                          const int32_t* indices, const double* data, const double* y,
                          int per_model, const double* weight /* n, or NULL: integer path */,
                          const int32_t* group /* n ids in [0, G), or NULL = all 0 */, int G,
                          const uint32_t* sets /* F x U bitmasks over groups, or NULL */, int U,
                          double* out /* F x U x 11 */,
                          int64_t* counts /* F x U x 6, written only for weight == NULL; may be NULL */,
                          double* auc_out /* F x U x 3 as spfm_bank_group_auc's out, or NULL */,
                          int64_t* auc_pairs /* as spfm_bank_group_auc's pairs, or NULL */);
int spfm_bank_set_partition(spfm_handle h, int64_t slab_nnz);
int spfm_bank_info(spfm_handle h, int64_t* out4);
int spfm_bank_release(spfm_handle h);

/* -- fold-in of new columns -------------------------------------------------------------------
 * Estimate the parameters of single columns (a new user, a new item, a column that collected new
 * rows) with every other parameter fixed.  The model, the blocks and the coefficient table are
 * those of spfm_explain_csr; here coef[q][s][0] is read too.  The ANOVA kernel is multilinear, so
 * for a row i that stores the target column j, with x_i\j the row without that one entry,
 *   f(x_i)  = c_i + z_i . theta_j
 *   c_i     = offset + [w . x_i\j] + sum_q sum_s lams_s sum_{t=0..M_q} coef[q][s][t] A^t(p_s, x_i\j)
 *   theta_j = ( w_j if fit_linear ; P[order_idx[q]][s][j], q = 0..n_blocks-1, s = 0..k-1 )
 *   z_i     = x_ij ( 1 if fit_linear ; lams_s sum_{t=1..M_q} coef[q][s][t] A^{t-1}(p_s, x_i\j) )
 * with R = n_blocks k (+ 1) unknowns, and the fold-in of column j is the unique minimiser of
 *   F_j(theta) = sum_{i: x_ij stored} loss(c_i + z_i . theta, y_i)
 *                + alpha/2 theta_w^2 + beta/2 |theta_P|^2,
 * loss one of SPFM_LOSS_* exactly as the training engines evaluate it (the logistic loss with its
 * branches at |y f| = 18).  alpha and beta stand against the SUM of the loss over the column's
 * rows.  offset is a constant of the model that the caller owns (the linear weights of columns
 * that are 1 in every row).  The A^t(x_i\j) are formed by a pass over the row that skips the
 * target entry -- no downdate, hence no cancellation -- so no result bit depends on the values
 * that column j holds in the handle's parameters.  Several target columns are independent when
 * no row stores two of them; that is required, never worked around by alternating.
 * The solver is a damped Newton iteration from theta = 0: g = Z^T l' + Lambda theta,
 * H = Z^T diag(l'') Z + Lambda (l'' the derivative of the active branch of l': 1; 2 [1 - y f > 0];
 * the three logistic branches), a Cholesky factorisation of H, an Armijo backtracking line search
 * (sufficient decrease 1e-4, halving, at most 40 halvings).  It stops when
 * max|grad F_j(theta)| <= tol max|grad F_j(0)| (converged = 1), at max_iter, or when the line
 * search stalls (converged = 0 unless the criterion holds).  Squared loss ends after one step.
 * Parameters only (spfm_set_params; no data, no spfm_configure), read-only as spfm_explain_csr:
 * the handle's parameters are not changed, writing theta back is the caller's business.  Values
 * are read in the handle's precision, all arithmetic is f64.  The target columns go through in
 * groups of whole columns, in the caller's order, whose design matrix (rows x R padded to 4, f64)
 * fits 256 MiB; the scratch stays allocated until spfm_set_params or spfm_destroy.
 *
 * Deterministic: a design entry is formed by one lane walking its row in stored order; c_i adds
 * the linear term, then the blocks in the caller's order, each a fixed butterfly over 64
 * components and the chunks of 64 in order; every sum over a column's rows (g, H, F) is formed by
 * one thread per entry that walks the rows in ascending row order, and the factorisation is a
 * fixed sequence.  A column's bits depend on its own rows alone: not on the other target columns,
 * the group size or the launch shape.
 *
 * spfm_foldin_csr: cols (n_cols distinct columns in [0, d)); theta (n_cols x R, row-major),
 *   n_rows, n_iter, converged, grad_norm (max|grad F_j| at the returned theta), obj0 = F_j(0),
 *   obj1 = F_j(theta) (n_cols each).  Rows that store no target column are ignored (and counted,
 *   spfm_foldin_info); a target column without rows gets theta = 0, n_iter = 0, converged = 1.
 *   Results are written group by group, so after a runtime error their contents are unspecified.
 * spfm_foldin_set_partition: rows per group of the following calls (0 = what fits the scratch).
 *   A group always holds at least one whole column.  No result bit depends on it: it exists so
 *   that a small problem can be made to run as many groups.
 * spfm_foldin_info: out5 = {device scratch held in bytes, device time in microseconds (HIP events)
 *   of the kernels of the last spfm_foldin_csr call without its copies, max_rows as set, groups of
 *   the last call, rows it ignored}.
 * Errors: those of spfm_explain_csr for the model and the rows; n_blocks < 1, NULL y / cols /
 * outputs, a row that stores two target columns (the message names the row), a duplicate or
 * out-of-range target column, beta <= 0, alpha <= 0 with fit_linear, max_iter < 1, tol negative
 * or not finite, an unknown loss, max_rows < 0 -> SPFM_ERR_INVALID; R above
 * SPFM_FOLDIN_MAX_UNKNOWNS, a single column whose design matrix exceeds the scratch
 * -> SPFM_ERR_UNSUPPORTED, never an approximate answer.  Every check precedes the first write to
 * an output; n = 0 is valid and writes the zero-row results. */
#define SPFM_FOLDIN_MAX_UNKNOWNS 128
int spfm_foldin_csr(spfm_handle h, int64_t n, const int64_t* indptr, const int32_t* indices,
                    const double* data, const double* y, int n_blocks, const int32_t* order_idx,
                    const int32_t* degree, const double* coef /* n_blocks x k x 7 */,
                    int fit_linear, double offset, int loss, int64_t n_cols, const int32_t* cols,
                    double alpha, double beta, int max_iter, double tol, double* theta,
                    int64_t* n_rows, int32_t* n_iter, int32_t* converged, double* grad_norm,
                    double* obj0, double* obj1);
int spfm_foldin_set_partition(spfm_handle h, int64_t max_rows);
int spfm_foldin_info(spfm_handle h, int64_t* out5);

#ifdef __cplusplus
}
#endif
#endif /* SPFM_H */
