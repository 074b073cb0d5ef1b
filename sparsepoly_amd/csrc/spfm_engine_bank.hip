// spfm_engine_bank.hip -- spfm_bank_set / _scores / _argmax / _losses / _mean / _group_sums /
// _group_auc / _group_curve / _set_partition / _info / _release (include/spfm.h): F fitted models, stacked along the component
// axis and resident on the handle, scored in one pass over the rows of a CSR matrix; the argmax,
// the loss sums, the weighted mean and the grouped weighted sums are formed
// on the device behind that pass (spfm_bank.hip.h); the rank statistic of spfm_bank_group_auc hangs
// its own steps on the same slabs (spfm_engine_bank_auc.hip), and so do the
// curve statistics of spfm_bank_group_curve (section 23).
// Read-only like predict and independent of spfm_set_params: the bank brings its own parameters.
// Rows go through in slabs bounded by stored entries.  See DESIGN.md section 17.
#include "spfm_engine.hip.h"
#include "spfm_bank.hip.h"

#include <algorithm>

static_assert(kBankMaxModels == SPFM_BANK_MAX_MODELS &&
                  kBankMaxComponents == SPFM_BANK_MAX_COMPONENTS,
              "header and device agree on the caps");
static_assert(kBankMaxModels <= kWave, "one model per lane of the wave that owns a row");
static_assert(LOSS_SQUARED == SPFM_LOSS_SQUARED && LOSS_SQUARED_HINGE == SPFM_LOSS_SQUARED_HINGE &&
                  LOSS_LOGISTIC == SPFM_LOSS_LOGISTIC,
              "header and device agree on the losses");
static_assert(kBankMaxGroups == SPFM_BANK_MAX_GROUPS && kBankMaxMetrics == SPFM_BANK_MAX_METRICS &&
                  METRIC_ABS_ERROR == SPFM_METRIC_ABS_ERROR &&
                  METRIC_SIGN_ERROR == SPFM_METRIC_SIGN_ERROR && kBankMaxMetrics == 4,
              "header and device agree on the group sums (the metric ids travel in an int4)");
static_assert(sizeof(double) * (kBlock / kWave) * kBankMaxGroups * kBankMaxModels <= (64u << 10),
              "the group table of a workgroup stays within 64 KB of LDS at the caps");

namespace {
// One slab's scratch: 4 (column) + at most 8 (value) bytes per stored entry and 8 F (scores) + up
// to 8 F (per-model targets) + 28 (offset, three per-row results) bytes per row.  The entries take
// at most 96 MiB, the rows of a slab are capped so that scores and targets stay within 128 MiB.
constexpr int64_t kBankRowBudget = 128ll << 20;
constexpr int64_t kBankSlabMax = 1ll << 23;  // stored entries per slab: default and largest
enum { BANK_GROUPS = 4, BANK_AUC = 5, BANK_CURVE = 6 };  // beside BANK_SCORES ... BANK_MEAN
// the two calls that keep the keys of every slab and sort them (spfm_engine_bank_auc.hip)
inline bool bank_sorts(int what) { return what == BANK_AUC || what == BANK_CURVE; }
}  // namespace

void spfm_engine::bank_release() {
    for (DevBuf* b : {&bk_pt, &bk_lams, &bk_w, &bk_koff, &bk_rp, &bk_ri, &bk_rv, &bk_sc, &bk_y,
                      &bk_wt, &bk_part, &bk_fin, &bk_oi, &bk_o0, &bk_o1, &bk_gw, &bk_gg, &bk_gpart,
                      &bk_gacc, &bk_akey, &bk_ameta, &bk_arow, &bk_aw, &bk_askey, &bk_asrow,
                      &bk_atmp, &bk_asets, &bk_ablk, &bk_aout, &bk_cblk, &bk_cout})
        b->release();
    bk_have = false;
    bk_F = bk_S = bk_d = bk_blocks = 0;
}

int spfm_engine::bank_set(int32_t d_, int F, const int32_t* koff, int n_blocks,
                          const int32_t* degree, const double* Pt_bank, const double* lams_bank,
                          const double* w_bank) {
    char buf[128];
    if (!koff || !degree || !Pt_bank || !lams_bank) FAIL(SPFM_ERR_INVALID, "bank_set: NULL array");
    if (F < 1) FAIL(SPFM_ERR_INVALID, "bank_set: a bank holds at least one model");
    if (d_ < 1) FAIL(SPFM_ERR_INVALID, "bank_set: d must be >= 1");
    if (n_blocks < 1 || n_blocks > 2) FAIL(SPFM_ERR_INVALID, "bank_set: n_blocks must be 1 or 2");
    if (F > SPFM_BANK_MAX_MODELS) {
        snprintf(buf, sizeof buf, "bank_set: %d models exceed SPFM_BANK_MAX_MODELS = %d", F,
                 (int)SPFM_BANK_MAX_MODELS);
        FAIL(SPFM_ERR_UNSUPPORTED, buf);
    }
    if (koff[0] != 0) FAIL(SPFM_ERR_INVALID, "bank_set: koff[0] must be 0");
    for (int f = 0; f < F; ++f)
        if (koff[f + 1] <= koff[f])
            FAIL(SPFM_ERR_INVALID, "bank_set: koff must increase (every model has a component)");
    const int S = koff[F];
    if (S > SPFM_BANK_MAX_COMPONENTS) {
        snprintf(buf, sizeof buf,
                 "bank_set: %d stacked components exceed SPFM_BANK_MAX_COMPONENTS = %d", S,
                 (int)SPFM_BANK_MAX_COMPONENTS);
        FAIL(SPFM_ERR_UNSUPPORTED, buf);
    }
    for (int q = 0; q < n_blocks; ++q) {
        const bool all_subsets = degree[q] == -1 && n_blocks == 1;
        if (!all_subsets && (degree[q] < 2 || degree[q] > SPFM_MAX_DEGREE))
            FAIL(SPFM_ERR_UNSUPPORTED, "bank_set: degree outside 2..6 and -1 (one block)");
    }
    bank_release();
    HIPC(bk_pt.alloc(sizeof(double) * (size_t)n_blocks * d_ * S));
    HIPC(bk_lams.alloc(sizeof(double) * (size_t)S));
    HIPC(bk_koff.alloc(sizeof(int32_t) * (size_t)(F + 1)));
    if (w_bank) HIPC(bk_w.alloc(sizeof(double) * (size_t)d_ * F));
    const int rc = run_staged([&]() -> int {
        SPFM_TRY(upload_to(bk_pt.p, Pt_bank, (size_t)n_blocks * d_ * S));
        SPFM_TRY(upload_to(bk_lams.p, lams_bank, (size_t)S));
        SPFM_TRY(upload_to(bk_koff.p, koff, (size_t)(F + 1)));
        return w_bank ? upload_to(bk_w.p, w_bank, (size_t)d_ * F) : SPFM_OK;
    });
    if (rc) {
        bank_release();
        return rc;
    }
    bk_have = true;
    bk_lin = w_bank != nullptr;
    bk_F = F;
    bk_S = S;
    bk_d = d_;
    bk_blocks = n_blocks;
    for (int q = 0; q < n_blocks; ++q) bk_degree[q] = degree[q];
    bk_slabs = bk_launches = 0;
    return SPFM_OK;
}

// every check of the five passes, before any device work and before any output is written
int spfm_engine::bank_check(const char* what, const BankCall& c) {
    const std::string w(what);
    if (!bk_have) FAIL(SPFM_ERR_INVALID, w + ": no bank set (spfm_bank_set)");
    if (c.n < 0 || !c.indptr) FAIL(SPFM_ERR_INVALID, w + ": bad arguments");  // (ahead of d)
    if (c.d != bk_d) {
        char buf[128];
        snprintf(buf, sizeof buf, "%s: the matrix has d = %d, the bank has d = %d", what, (int)c.d,
                 bk_d);
        FAIL(SPFM_ERR_INVALID, buf);
    }
    SPFM_TRY(check_csr(what, c.n, c.indptr, c.indices, c.data, bk_d, INT32_MAX));
    if (c.what == BANK_LOSSES) {
        if (c.loss != SPFM_LOSS_SQUARED && c.loss != SPFM_LOSS_SQUARED_HINGE &&
            c.loss != SPFM_LOSS_LOGISTIC)
            FAIL(SPFM_ERR_INVALID, w + ": unknown loss");
        if (!c.out || (c.n > 0 && !c.y)) FAIL(SPFM_ERR_INVALID, w + ": NULL array");
    } else if (c.what == BANK_GROUPS || bank_sorts(c.what)) {  // (auc: Q = 1, a metric of its own)
        char buf[160];
        const double* out = c.what == BANK_CURVE ? c.curve : c.out;  // (the curve's c.out may be NULL)
        if (!out || !c.metrics || (c.n > 0 && !c.y)) FAIL(SPFM_ERR_INVALID, w + ": NULL array");
        if (c.G < 1 || c.Q < 1) FAIL(SPFM_ERR_INVALID, w + ": G and Q must be >= 1");
        if (c.G > SPFM_BANK_MAX_GROUPS) {
            snprintf(buf, sizeof buf, "%s: %d groups exceed SPFM_BANK_MAX_GROUPS = %d", what, c.G,
                     (int)SPFM_BANK_MAX_GROUPS);
            FAIL(SPFM_ERR_UNSUPPORTED, buf);
        }
        if (c.Q > SPFM_BANK_MAX_METRICS) {
            snprintf(buf, sizeof buf, "%s: %d metrics exceed SPFM_BANK_MAX_METRICS = %d", what, c.Q,
                     (int)SPFM_BANK_MAX_METRICS);
            FAIL(SPFM_ERR_UNSUPPORTED, buf);
        }
        for (int q = 0; q < c.Q; ++q) {
            const int m = c.metrics[q];
            if (m != SPFM_LOSS_SQUARED && m != SPFM_LOSS_SQUARED_HINGE && m != SPFM_LOSS_LOGISTIC &&
                m != SPFM_METRIC_ABS_ERROR && m != SPFM_METRIC_SIGN_ERROR)
                FAIL(SPFM_ERR_INVALID, w + ": unknown metric");
            for (int p = 0; p < q; ++p)
                if (c.metrics[p] == m) FAIL(SPFM_ERR_INVALID, w + ": the same metric twice");
        }
        if (c.group)
            for (int64_t i = 0; i < c.n; ++i)
                if (c.group[i] < 0 || c.group[i] >= c.G) {
                    snprintf(buf, sizeof buf, "%s: group id %d of row %lld outside [0, %d)", what,
                             (int)c.group[i], (long long)i, c.G);
                    FAIL(SPFM_ERR_INVALID, buf);
                }
        if (c.weight)
            for (int64_t i = 0; i < c.n; ++i)
                if (!(c.weight[i] >= 0.0) || !std::isfinite(c.weight[i])) {
                    snprintf(buf, sizeof buf, "%s: the weight of row %lld is negative or not finite",
                             what, (long long)i);
                    FAIL(SPFM_ERR_INVALID, buf);
                }
    } else if (c.n > 0) {
        if (!c.out) FAIL(SPFM_ERR_INVALID, w + ": NULL output");
        if (c.what == BANK_ARGMAX && (!c.idx || !c.runner))
            FAIL(SPFM_ERR_INVALID, w + ": NULL output");
    }
    return SPFM_OK;
}

template <typename T, int M>
void spfm_engine::bank_launch_block(int64_t rows, int64_t e0, int q, int first) {
    hipLaunchKernelGGL((bank_predict_kernel<T, M>), dim3(cdiv(rows, kBlock / kWave)), dim3(kBlock),
                       0, stream, rows, e0, bk_S, bk_F, bk_rp.as<int64_t>(), bk_ri.as<int32_t>(),
                       bk_rv.as<T>(), bk_pt.as<double>() + (size_t)q * bk_d * bk_S,
                       bk_lams.as<double>(), bk_koff.as<int32_t>(),
                       (first && bk_lin) ? bk_w.as<double>() : (const double*)nullptr, first,
                       bk_sc.as<double>());
    ++bk_launches;
}

// rows [r0, r1): stage, the blocks in _get_output's order, the pass's reduction, copy back.
// part0: where this slab's loss partials start (one per 256 rows).
template <typename T>
int spfm_engine::bank_slab(const BankCall& c, int64_t r0, int64_t r1, int64_t part0) {
    const int64_t rows = r1 - r0, e0 = c.indptr[r0];
    const int F = bk_F;
    HIPC(bk_sc.alloc(sizeof(double) * (size_t)rows * F));
    if (c.what == BANK_ARGMAX) {
        HIPC(bk_oi.alloc(sizeof(int32_t) * (size_t)rows));
        HIPC(bk_o0.alloc(sizeof(double) * (size_t)rows));
        HIPC(bk_o1.alloc(sizeof(double) * (size_t)rows));
    }
    if (c.what == BANK_MEAN) HIPC(bk_o0.alloc(sizeof(double) * (size_t)rows));
    if (c.what == BANK_LOSSES || c.what == BANK_GROUPS || bank_sorts(c.what))
        HIPC(bk_y.alloc(sizeof(double) * (size_t)rows * (c.per_model ? F : 1)));
    const unsigned row_blocks = cdiv(rows, kBlock);
    const int cells = c.Q * c.G * F;  // group sums: the cells of one table
    if (c.what == BANK_GROUPS) {
        if (c.weight) HIPC(bk_gw.alloc(sizeof(double) * (size_t)rows));
        if (c.group) HIPC(bk_gg.alloc(sizeof(int32_t) * (size_t)rows));
        HIPC(bk_gpart.alloc(sizeof(double) * (size_t)row_blocks * cells));
    }
    if (bank_sorts(c.what) && c.group) HIPC(bk_gg.alloc(sizeof(int32_t) * (size_t)rows));
    std::vector<T> hv;  // staging of the values
    return run_staged([&]() -> int {
        SPFM_TRY(stage_csr_rows<T>(bk_rp, bk_ri, bk_rv, hv, c.indptr, c.indices, c.data, r0, r1));
        if (c.what == BANK_LOSSES || c.what == BANK_GROUPS || bank_sorts(c.what))
            SPFM_TRY(upload_to(bk_y.p, c.y + (size_t)r0 * (c.per_model ? F : 1),
                               (size_t)rows * (c.per_model ? F : 1)));
        if (c.what == BANK_GROUPS && c.weight)
            SPFM_TRY(upload_to(bk_gw.p, c.weight + r0, (size_t)rows));
        if ((c.what == BANK_GROUPS || bank_sorts(c.what)) && c.group)
            SPFM_TRY(upload_to(bk_gg.p, c.group + r0, (size_t)rows));
        for (int q = 0; q < bk_blocks; ++q) {
            (void)SPFM_DISPATCH_KIND(kind_of(bk_degree[q]), true,  // (2..6 or -1: bank_set)
                                     bank_launch_block<T, M>(rows, e0, q, q == 0));
        }
        const double* sc = bk_sc.as<double>();
        if (c.what == BANK_ARGMAX)
            hipLaunchKernelGGL(bank_argmax_kernel, dim3(row_blocks), dim3(kBlock), 0, stream, rows,
                               F, sc, bk_oi.as<int32_t>(), bk_o0.as<double>(), bk_o1.as<double>());
        if (c.what == BANK_MEAN)
            hipLaunchKernelGGL(bank_mean_kernel, dim3(row_blocks), dim3(kBlock), 0, stream, rows, F,
                               sc, bk_wt.as<double>(), bk_o0.as<double>());
        if (c.what == BANK_LOSSES)
            hipLaunchKernelGGL(bank_loss_partial_kernel, dim3(row_blocks), dim3(kBlock), 0, stream,
                               rows, F, sc, bk_y.as<double>(), c.per_model ? F : 1,
                               c.per_model ? 1 : 0, c.loss,
                               bk_part.as<double>() + (size_t)part0 * F);
        if (c.what == BANK_GROUPS) {
            // the slab's blocks (part0 .. part0 + row_blocks - 1 of the call) into partial tables,
            // then onto the call's running table in block order
            const int4 ids = {c.metrics[0], c.Q > 1 ? c.metrics[1] : 0, c.Q > 2 ? c.metrics[2] : 0,
                              c.Q > 3 ? c.metrics[3] : 0};
            hipLaunchKernelGGL(bank_group_partial_kernel, dim3(row_blocks), dim3(kBlock),
                               sizeof(double) * (kBlock / kWave) * c.G * F, stream, rows, F, sc,
                               bk_y.as<double>(), c.per_model ? F : 1, c.per_model ? 1 : 0,
                               c.weight ? bk_gw.as<double>() : (const double*)nullptr,
                               c.group ? bk_gg.as<int32_t>() : (const int32_t*)nullptr, c.G, c.Q,
                               ids, bk_gpart.as<double>());
            hipLaunchKernelGGL(bank_group_finish_kernel, dim3(cdiv(cells, kBlock)), dim3(kBlock), 0,
                               stream, (int64_t)row_blocks, cells, bk_gpart.as<double>(),
                               bk_gacc.as<double>());
        }
        if (bank_sorts(c.what)) auc_slab(c, r0, rows);
        HIPC(hipGetLastError());
        if (c.what == BANK_SCORES) SPFM_TRY(download(c.out + (size_t)r0 * F, sc, (size_t)rows * F));
        if (c.what == BANK_ARGMAX) {
            SPFM_TRY(download(c.idx + r0, bk_oi.p, (size_t)rows));
            SPFM_TRY(download(c.out + r0, bk_o0.p, (size_t)rows));
            SPFM_TRY(download(c.runner + r0, bk_o1.p, (size_t)rows));
        }
        if (c.what == BANK_MEAN) SPFM_TRY(download(c.out + r0, bk_o0.p, (size_t)rows));
        return SPFM_OK;
    });
}

template <typename T>
int spfm_engine::bank_run(const char* what, const BankCall& c) {
    SPFM_TRY(bank_check(what, c));
    if (bank_sorts(c.what)) SPFM_TRY(auc_check(what, c));
    struct AucScratch {  // the rank statistic's scratch does not outlive the call
        spfm_engine* e;
        ~AucScratch() {
            if (e) e->auc_release();
        }
    } auc_scratch{bank_sorts(c.what) ? this : nullptr};
    bk_slabs = bk_launches = 0;
    const int F = bk_F;
    if (c.n == 0) {
        if (bank_sorts(c.what)) auc_empty(c);
        if (c.what == BANK_LOSSES) std::fill(c.out, c.out + F, 0.0);
        if (c.what == BANK_GROUPS) std::fill(c.out, c.out + (size_t)c.Q * F * c.G, 0.0);
        return SPFM_OK;
    }
    const int64_t slab_nnz = bk_slab_nnz > 0 ? bk_slab_nnz : kBankSlabMax;
    const int64_t row_cap = std::max<int64_t>(1, kBankRowBudget / (16 * (int64_t)F));
    std::vector<int64_t> cut{0}, part{0};
    for (int64_t r0 = 0; r0 < c.n;) {
        const int64_t r1 = slab_end(r0, c.n, row_cap, {c.indptr, slab_nnz});
        cut.push_back(r1);
        part.push_back(part.back() + (r1 - r0 + kBlock - 1) / kBlock);
        r0 = r1;
    }
    if (c.what == BANK_LOSSES) {
        HIPC(bk_part.alloc(sizeof(double) * (size_t)part.back() * F));
        HIPC(bk_fin.alloc(sizeof(double) * (size_t)F));
    }
    if (c.what == BANK_GROUPS) {
        HIPC(bk_gacc.alloc(sizeof(double) * (size_t)c.Q * c.G * F));
        HIPC(hipMemsetAsync(bk_gacc.p, 0, sizeof(double) * (size_t)c.Q * c.G * F, stream));
    }
    if (bank_sorts(c.what)) SPFM_TRY(auc_begin(c));
    if (c.what == BANK_MEAN) {
        const std::vector<double> hw((size_t)F, 1.0 / (double)F);  // staging of the default
        HIPC(bk_wt.alloc(sizeof(double) * (size_t)F));
        const double* wt = c.wt ? c.wt : hw.data();
        SPFM_TRY(run_staged([&] { return upload_to(bk_wt.p, wt, (size_t)F); }));
    }
    for (size_t s = 0; s + 1 < cut.size(); ++s) {
        SPFM_TRY(bank_slab<T>(c, cut[s], cut[s + 1], part[s]));
        ++bk_slabs;
    }
    if (c.what == BANK_LOSSES) {
        hipLaunchKernelGGL(bank_loss_finish_kernel, dim3(F), dim3(kBlock), 0, stream, part.back(),
                           F, bk_part.as<double>(), bk_fin.as<double>());
        HIPC(hipGetLastError());
        SPFM_TRY(download(c.out, bk_fin.p, (size_t)F));
        SPFM_TRY(sync());
    }
    if (c.what == BANK_GROUPS) {  // the device table is [q][g][f] (lane = member), out is [q][f][g]
        std::vector<double> tab((size_t)c.Q * c.G * F);
        SPFM_TRY(download(tab.data(), bk_gacc.p, tab.size()));
        SPFM_TRY(sync());
        for (int q = 0; q < c.Q; ++q)
            for (int g = 0; g < c.G; ++g)
                for (int f = 0; f < F; ++f)
                    c.out[((size_t)q * F + f) * c.G + g] = tab[((size_t)q * c.G + g) * F + f];
    }
    if (bank_sorts(c.what)) SPFM_TRY(auc_finish(c));
    return SPFM_OK;
}

extern "C" {

int spfm_bank_set(spfm_handle h, int32_t d, int F, const int32_t* koff, int n_blocks,
                  const int32_t* degree, const double* Pt_bank, const double* lams_bank,
                  const double* w_bank) {
    SPFM_GUARD(h);
    return h->bank_set(d, F, koff, n_blocks, degree, Pt_bank, lams_bank, w_bank);
}

int spfm_bank_scores(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                     const int32_t* indices, const double* data, double* out) {
    SPFM_GUARD(h);
    const spfm_engine::BankCall c = {BANK_SCORES, n, d, indptr, indices, data, out, nullptr,
                                     nullptr, 0, nullptr, 0, nullptr};
    return SPFM_DISPATCH(h->dtype, return h->bank_run<T>("bank_scores", c));
}

int spfm_bank_argmax(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                     const int32_t* indices, const double* data, int32_t* idx, double* best,
                     double* runner) {
    SPFM_GUARD(h);
    const spfm_engine::BankCall c = {BANK_ARGMAX, n, d, indptr, indices, data, best, idx,
                                     runner, 0, nullptr, 0, nullptr};
    return SPFM_DISPATCH(h->dtype, return h->bank_run<T>("bank_argmax", c));
}

int spfm_bank_losses(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                     const int32_t* indices, const double* data, int loss, const double* y,
                     int per_model, double* out) {
    SPFM_GUARD(h);
    const spfm_engine::BankCall c = {BANK_LOSSES, n, d, indptr, indices, data, out, nullptr,
                                     nullptr, loss, y, per_model ? 1 : 0, nullptr};
    return SPFM_DISPATCH(h->dtype, return h->bank_run<T>("bank_losses", c));
}

int spfm_bank_mean(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                   const int32_t* indices, const double* data, const double* weights,
                   double* out) {
    SPFM_GUARD(h);
    const spfm_engine::BankCall c = {BANK_MEAN, n, d, indptr, indices, data, out, nullptr,
                                     nullptr, 0, nullptr, 0, weights};
    return SPFM_DISPATCH(h->dtype, return h->bank_run<T>("bank_mean", c));
}

int spfm_bank_group_sums(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                         const int32_t* indices, const double* data, const double* y,
                         int per_model, const double* weight, const int32_t* group, int G, int Q,
                         const int32_t* metrics, double* out) {
    SPFM_GUARD(h);
    const spfm_engine::BankCall c = {BANK_GROUPS, n, d, indptr, indices, data, out, nullptr,
                                     nullptr, 0, y, per_model ? 1 : 0, nullptr, weight, group, G,
                                     Q, metrics};
    return SPFM_DISPATCH(h->dtype, return h->bank_run<T>("bank_group_sums", c));
}

int spfm_bank_group_auc(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                        const int32_t* indices, const double* data, const double* y, int per_model,
                        const double* weight, const int32_t* group, int G, const uint32_t* sets,
                        int U, double* out, int64_t* pairs) {
    SPFM_GUARD(h);
    static const int32_t kMetric = SPFM_METRIC_SIGN_ERROR;  // (bank_check reads one metric id)
    const spfm_engine::BankCall c = {BANK_AUC, n, d, indptr, indices, data, out, nullptr,
                                     nullptr, 0, y, per_model ? 1 : 0, nullptr, weight, group, G,
                                     1, &kMetric, sets, U, pairs};
    return SPFM_DISPATCH(h->dtype, return h->bank_run<T>("bank_group_auc", c));
}

int spfm_bank_group_curve(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                          const int32_t* indices, const double* data, const double* y,
                          int per_model, const double* weight, const int32_t* group, int G,
                          const uint32_t* sets, int U, double* out, int64_t* counts,
                          double* auc_out, int64_t* auc_pairs) {
    SPFM_GUARD(h);
    static const int32_t kMetric = SPFM_METRIC_SIGN_ERROR;  // (bank_check reads one metric id)
    const spfm_engine::BankCall c = {BANK_CURVE, n, d, indptr, indices, data, auc_out, nullptr,
                                     nullptr, 0, y, per_model ? 1 : 0, nullptr, weight, group, G,
                                     1, &kMetric, sets, U, auc_out ? auc_pairs : nullptr, out,
                                     counts};
    return SPFM_DISPATCH(h->dtype, return h->bank_run<T>("bank_group_curve", c));
}

int spfm_bank_set_partition(spfm_handle h, int64_t slab_nnz) {
    if (!h) return SPFM_ERR_INVALID;
    if (slab_nnz < 0 || slab_nnz > kBankSlabMax) {
        h->err = "bank_set_partition: slab_nnz must be in [0, 2^23]";
        return SPFM_ERR_INVALID;
    }
    h->bk_slab_nnz = slab_nnz;
    return SPFM_OK;
}

int spfm_bank_info(spfm_handle h, int64_t* out4) {
    if (!h || !out4) return SPFM_ERR_INVALID;
    out4[0] = h->bk_slabs;
    out4[1] = h->bk_launches;
    out4[2] = (int64_t)h->bank_image_bytes();
    out4[3] = h->bk_S;
    return SPFM_OK;
}

int spfm_bank_release(spfm_handle h) {
    SPFM_GUARD(h);
    h->bank_release();
    return SPFM_OK;
}

}  // extern "C"
